// Direct gather form of the 3x3x3 sparse convolution: from a layer to its launch.  launch_ct<CT> (one per translation unit
// sparse_conv_direct_ct{1..4}.hip) picks the chunk count, launch_k asks select_direct_form (sparse_conv_direct_select.hpp) which
// form the layer gets, and launch_form maps that onto the instantiation — the only place that names them, so the `if constexpr`
// guards below are what bounds the set of kernels a unit holds.
#pragma once
#include "sparse_conv_direct_kernels.hpp"
#include "sparse_conv_direct_persist.hpp"

namespace epconv {
namespace {

template <int CT, int KCH>
int launch_form(const DirectForm &f, const ConvParams &p, dim3 grid, size_t lds, hipStream_t st)
{
    constexpr int G0 = stage_chunks(KCH), GA = alt_stage_chunks(KCH);
    if (f.persist) {
        // (instantiated only where a 27-offset packing can fit the LDS beside the eight job windows: <= 4.9 KB per offset)
        if constexpr (KCH * (CT * 1024 - 512) <= 4864) {
            if (f.tail) return launch_persist<CT, KCH, true>(p, st);
            if constexpr (KCH * CT * 1024 <= 4864) return launch_persist<CT, KCH, false>(p, st);
        }
        return EPRECON_ERR_UNSUPPORTED;
    }
    void (*kern)(ConvParams) = nullptr;
    auto with_tail = [&](auto tail) {
        constexpr bool TAIL = decltype(tail)::value;
        if (f.bf) {     // (padded tiles, the deepest stage)
            if constexpr (!TAIL)
                kern = f.mode == 2   ? spconv_direct16_kernel<CT, KCH, false, G0, true, 2>
                       : f.mode == 1 ? spconv_direct16_kernel<CT, KCH, false, G0, true, 1>
                                     : spconv_direct16_kernel<CT, KCH, false, G0, true>;
        } else if (f.g != G0) {     // (the alternative stage depth: MODE 0)
            if constexpr (GA != 0) kern = spconv_direct16_kernel<CT, KCH, TAIL, GA>;
        } else if (f.mode >= 3) {
            if constexpr (G0 == KCH)
                kern = f.mode == 4 ? spconv_direct16_kernel<CT, KCH, TAIL, G0, false, 4> : spconv_direct16_kernel<CT, KCH, TAIL, G0, false, 3>;
        } else {
            kern = f.mode == 2   ? spconv_direct16_kernel<CT, KCH, TAIL, G0, false, 2>
                   : f.mode == 1 ? spconv_direct16_kernel<CT, KCH, TAIL, G0, false, 1>
                                 : spconv_direct16_kernel<CT, KCH, TAIL, G0>;
        }
    };
    if (f.tail) with_tail(std::true_type{});
    else with_tail(std::false_type{});
    if (!kern) return EPRECON_ERR_UNSUPPORTED;      // (a form select_direct_form does not produce for this CT, KCH)
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, p);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// Workgroups per CU of the primary and the alternative stage depth, asked once per (CT, KCH, tail form).
template <int CT, int KCH>
void stage_occupancy(bool tail, size_t lds, int &occ_p, int &occ_a)
{
    constexpr int G0 = stage_chunks(KCH), GA = alt_stage_chunks(KCH);
    static int occ[2][2] = {{0, 0}, {0, 0}};      // [tail][primary, alternative]
    int *o = occ[tail ? 1 : 0];
    if (!o[0]) {
        const void *kp = tail ? reinterpret_cast<const void *>(spconv_direct16_kernel<CT, KCH, true, G0>)
                              : reinterpret_cast<const void *>(spconv_direct16_kernel<CT, KCH, false, G0>);
        const void *ka = tail ? reinterpret_cast<const void *>(spconv_direct16_kernel<CT, KCH, true, GA>)
                              : reinterpret_cast<const void *>(spconv_direct16_kernel<CT, KCH, false, GA>);
        int a = 0, b = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, kp, 256, lds) != hipSuccess || a <= 0) a = 1;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, ka, 256, lds) != hipSuccess || b <= 0) b = a;
        o[1] = b;
        o[0] = a;
    }
    occ_p = o[0];
    occ_a = o[1];
}

template <int CT, int KCH>
int launch_k(const ConvParams &p, hipStream_t st)
{
    const size_t lds = direct_lds_bytes(p.K, CT, KCH);
    const DirectSwitches sw = direct_switches();
    int occ_p = 1, occ_a = 1;
    if constexpr (alt_stage_chunks(KCH) != 0) stage_occupancy<CT, KCH>(direct_tail(p, sw), lds, occ_p, occ_a);
    const DirectForm f = select_direct_form(p, sw, device_cus(), occ_p, occ_a);
    return launch_form<CT, KCH>(f, p, dim3((unsigned)ceil_div(p.n_out, kDirectRows)), lds, st);
}

template <int CT>
int launch_ct(const ConvParams &p, hipStream_t st)
{
    const int kch = (p.Cin + 15) / 16;
    if (kch <= 6) return pick<1, 2, 3, 4, 5, 6>(kch, [&](auto k) { return launch_k<CT, decltype(k)::value>(p, st); });
    // any chunk count: the (offset, chunk) sequence is walked with run-time indices (DirectForm::g == 0)
    hipLaunchKernelGGL((spconv_direct16_generic_kernel<CT>), dim3((unsigned)ceil_div(p.n_out, kDirectRows)), dim3(256),
                       direct_lds_bytes(p.K, CT, kch), st, p, kch);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // namespace
}  // namespace epconv
