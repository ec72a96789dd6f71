// Dense 2D 3x3 'same' convolution on v_mfma_f32_16x16x4_f32 over the [V * H * W, C] pixel rows of the 2D fusion stack: the 2D
// twin of conv3d_tile16_kernel (sparse_conv_dense3d.hip).  The direct gather kernel runs these layers through the pixel map: nine index
// loads per row, each followed by a dependent 16-byte gather, and every input row read nine times through L1 (a 12 -> 12 layer
// on 172,800 pixels took 27-38 us for 8 us of padded MFMA work and 4 us of streaming).  Here the input is read once per tile:
//   - a workgroup owns 4 image rows x 16 pixels of one view; wave w owns row w (one 16-row MFMA tile) and all CT column tiles
//   - the 6 x 18 halo is staged in LDS in passes of 16 channels (8.6 KB whatever C_in is), the producer's pending BatchNorm
//     (+ ReLU) applied on the way in, zeros outside the image (no tap reaches into another view); the next pass's halo is loaded
//     into registers while the current pass's MFMAs run
//   - A operands: one ds_read_b128 per (offset, pass) at compile-time offsets (a last chunk of <= 8 channels: ds_read_b64 and
//     two MFMAs, the wq16 tail8 layout); B operands: straight from the wq16 packing (pack_weights16_kernel), one 1 KB buffer
//     load per (offset, pass, column tile), two offsets ahead, spread among the MFMAs with sched_group_barrier
//   - epilogue: tile16_epilogue (conv_common.hpp), one BatchNorm summary row per workgroup (or its accumulator-block add)
// Summation order: four channels per MFMA as the direct kernel, offsets in a different order: equal within fp32 round-off.
#include <stdint.h>
#include <stdlib.h>

#include "common.hpp"
#include "conv_common.hpp"

namespace epconv {
namespace {
using namespace ep;

constexpr int kT2H = 4, kT2W = 16;                                  // tile: image rows x pixels (one row per wave)
constexpr int kT2HaloW = kT2W + 2, kT2Halo = (kT2H + 2) * kT2HaloW; // 18, 108 pixels
constexpr int kT2P = 20;                                            // LDS pixel pitch in floats (16 channels + 4)
// (long pixel lists only: kT2MinRows, conv_common.hpp)

template <int CT, int KCH, bool TAIL8, bool BN>
__global__ __launch_bounds__(256) void conv2d_tile16_kernel(ConvParams p, int tiles_x, int tiles_per_map)
{
    __shared__ __attribute__((aligned(16))) float sX[kT2Halo * kT2P];   // [108][20]; (after the loop) the summaries' scratch
    static_assert(kWaves * 3 * 16 * CT <= kT2Halo * kT2P, "summary scratch overlays the halo");
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);   // (gridDim.x = the tile count)
    const int map = tile / tiles_per_map, rt = tile - map * tiles_per_map;
    const int ty = rt / tiles_x, tx = rt - ty * tiles_x;
    const int y0 = ty * kT2H, x0 = tx * kT2W;
    const int H = p.img_h, W = p.img_w;
    const size_t map_row0 = (size_t)map * H * W;

    // ---- halo staging: thread -> (halo pixel, 4-channel group g = tid % G); G = 4 groups per pixel, 2 for a <= 8-channel chunk.
    // Loads at clamped addresses first (in flight under the previous pass's MFMAs), the fix-ups and LDS stores after the barrier.
    float4 hv[2], sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
    auto load_halo = [&](int pass) {
        const int G = (TAIL8 && pass == KCH - 1) ? 2 : 4;
        const int c = min(16 * pass + 4 * (tid % G), p.Cin - 4);
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int px = min((tid + it * 256) / G, kT2Halo - 1);
            const int hy = px / kT2HaloW, hx = px - hy * kT2HaloW;
            const int y = min(max(y0 - 1 + hy, 0), H - 1), x = min(max(x0 - 1 + hx, 0), W - 1);
            hv[it] = *reinterpret_cast<const float4 *>(p.x + (map_row0 + (size_t)y * W + x) * p.ld_x + c);
        }
        if (BN) {   // (in_scale / in_shift may be slices of a concat buffer's vectors: no alignment assumed)
            sc = make_float4(p.in_scale[c], p.in_scale[c + 1], p.in_scale[c + 2], p.in_scale[c + 3]);
            sh = make_float4(p.in_shift[c], p.in_shift[c + 1], p.in_shift[c + 2], p.in_shift[c + 3]);
        }
    };
    auto store_halo = [&](int pass) {
        const int G = (TAIL8 && pass == KCH - 1) ? 2 : 4;
        const int g = tid % G;
        const bool cok = 16 * pass + 4 * g < p.Cin;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
            const int px = (tid + it * 256) / G;
            if (px >= kT2Halo) break;
            const int hy = px / kT2HaloW, hx = px - hy * kT2HaloW;
            const int y = y0 - 1 + hy, x = x0 - 1 + hx;
            float4 v = hv[it];
            if (BN) {
                v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y);
                v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
                if (p.in_relu) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
            }
            if (!(cok && y >= 0 && y < H && x >= 0 && x < W)) v = make_float4(0.f, 0.f, 0.f, 0.f);   // zero padding
            *reinterpret_cast<float4 *>(sX + px * kT2P + 4 * g) = v;
        }
    };

    f32x4 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const bool work = y0 + wave < H;   // (wave-uniform) a ragged last tile row: the wave only takes part in the barriers

    constexpr unsigned kStepBytes = CT * 1024u, kOffBytes = KCH * kStepBytes;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq16), 0, (int)(9 * kOffBytes), 0x00020000);
    const unsigned wlane = (unsigned)lane * 16u;
    constexpr int kAheadB = 2;
    load_halo(0);
#pragma unroll
    for (int pass = 0; pass < KCH; ++pass) {
        const bool tail = TAIL8 && pass == KCH - 1;    // (compile time after unrolling)
        if (pass > 0) __syncthreads();  // every wave is done reading the previous pass's channels
        store_halo(pass);
        __syncthreads();
        if (pass + 1 < KCH) load_halo(pass + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (!work) continue;
        // this lane's A row: tile row `wave`, pixel l16; offset k = 3 dy + dx reads halo pixel (wave + dy, l16 + dx)
        const float *xa = sX + (wave * kT2HaloW + l16) * kT2P + (tail ? 2 * q : 4 * q);
        float4 bq[kAheadB + 1][CT];
        float4 aq[2];
        auto load_b = [&](int k, float4(&dst)[CT]) {
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)t * 1024u,
                                                                      (unsigned)k * kOffBytes + (unsigned)pass * kStepBytes, 0);
                dst[t] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
        };
        auto load_a = [&](int k) {
            const float *src = xa + ((k / 3) * kT2HaloW + (k % 3)) * kT2P;
            if (tail) {
                const float2 v = *reinterpret_cast<const float2 *>(src);
                return make_float4(v.x, v.y, 0.0f, 0.0f);
            }
            return *reinterpret_cast<const float4 *>(src);
        };
#pragma unroll
        for (int k = 0; k < kAheadB; ++k) load_b(k, bq[k]);
        aq[0] = load_a(0);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            if (k + kAheadB < 9) load_b(k + kAheadB, bq[(k + kAheadB) % (kAheadB + 1)]);
            if (k + 1 < 9) aq[(k + 1) & 1] = load_a(k + 1);
            const float4 av = aq[k & 1];
            const float4(&bk)[CT] = bq[k % (kAheadB + 1)];
            // the CT accumulators alternate (a 16x16x4 MFMA issues every 32 cycles but returns after 40)
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bk[t].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bk[t].y, acc[t], 0, 0, 0);
            if (!tail) {
#pragma unroll
                for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bk[t].z, acc[t], 0, 0, 0);
#pragma unroll
                for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bk[t].w, acc[t], 0, 0, 0);
            }
            // this offset's loads (B two offsets ahead, the next offset's A) spread among its MFMAs
#pragma unroll
            for (int sg = 0; sg < CT; ++sg) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                if (tail) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                else __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();  // every wave is done with the halo: the summaries' scratch overlays it

    int orow[4];   // output rows of this lane's accumulator rows 4 q + j: pixel (y0 + wave, x0 + 4 q + j)
    const int y = y0 + wave;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + 4 * q + j;
        orow[j] = (y < H && x < W) ? (int)(map_row0 + (size_t)y * W + x) : -1;
    }
    tile16_epilogue<CT, true>(p, acc, orow, sX, tile);
}

int tiles_x_of(const ConvParams &p) { return (p.img_w + kT2W - 1) / kT2W; }
int tiles_per_map_of(const ConvParams &p) { return tiles_x_of(p) * ((p.img_h + kT2H - 1) / kT2H); }

template <int CT, int KCH, bool TAIL8, bool BN>
int launch_t2(const ConvParams &p, hipStream_t st)
{
    const int per_map = tiles_per_map_of(p);
    hipLaunchKernelGGL((conv2d_tile16_kernel<CT, KCH, TAIL8, BN>), dim3((unsigned)((int64_t)per_map * p.img_maps)), dim3(256), 0, st, p,
                       tiles_x_of(p), per_map);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
template <int CT, int KCH, bool TAIL8>
int launch_t2_bn(const ConvParams &p, hipStream_t st)
{
    return p.in_scale ? launch_t2<CT, KCH, TAIL8, true>(p, st) : launch_t2<CT, KCH, TAIL8, false>(p, st);
}
template <int CT, int KCH>
int launch_t2_tail(const ConvParams &p, hipStream_t st)
{
    // (pack_weights16_body's rule: a last chunk of <= 8 channels is laid out for two MFMAs)
    return p.Cin - 16 * (KCH - 1) <= 8 ? launch_t2_bn<CT, KCH, true>(p, st) : launch_t2_bn<CT, KCH, false>(p, st);
}
template <int CT>
int launch_t2_kch(const ConvParams &p, hipStream_t st)
{
    switch ((p.Cin + 15) / 16) {
        case 1: return launch_t2_tail<CT, 1>(p, st);
        case 2: return launch_t2_tail<CT, 2>(p, st);
        default: return launch_t2_tail<CT, 3>(p, st);
    }
}
}  // namespace

// EPRECON_CONV_TILE2D16=0: the 3x3 layers of the 2D stack on the kernels of the previous rule (read per launch: tests flip it).
// Declines — the caller falls back to the direct gather kernel — for an input whose pending BatchNorm is an accumulator block of
// the opt-in form (c) (in_acc), LayerNorm / accumulate, C_in or C_out above 48, unaligned inputs, and short pixel lists.  The
// PRODUCER side of form (c) (bn_acc) is taken: a layer's rows are the same bits under either BatchNorm form.
bool tile2d16_ok(const ConvParams &p)
{
    if (switch_off("EPRECON_CONV_TILE2D16")) return false;
    if (p.K != 9 || p.img_h <= 0 || p.img_w <= 0 || p.img_maps <= 0 || (int64_t)p.img_maps * p.img_h * p.img_w != p.n_out)
        return false;
    if (p.n_out < kT2MinRows || p.ln || p.accumulate || p.in_acc) return false;
    if (p.Cin > 48 || p.Cout > 48 || p.Cin % 4 != 0 || p.ld_x % 4 != 0 || (reinterpret_cast<uintptr_t>(p.x) & 15) != 0) return false;
    if (!p.wq16 || (reinterpret_cast<uintptr_t>(p.wq16) & 15) != 0) return false;
    // every pixel row of the images must be readable (n_in >= n_out)
    if (p.x_bytes < ((int64_t)(p.n_out - 1) * p.ld_x + p.Cin) * 4) return false;
    return true;
}

int64_t tile2d16_partial_rows(const ConvParams &p) { return (int64_t)tiles_per_map_of(p) * p.img_maps; }

int launch_tile2d16(const ConvParams &p, hipStream_t st)
{
    switch ((p.Cout + 15) / 16) {
        case 1: return launch_t2_kch<1>(p, st);
        case 2: return launch_t2_kch<2>(p, st);
        default: return launch_t2_kch<3>(p, st);
    }
}

}  // namespace epconv
