// Direct gather form of the 3x3x3 sparse convolution: which kernel a layer gets.  Host only — no kernel and no device object —
// so that sparse_conv_direct.hip (eligibility, dispatch, summary-block rows) can include it without the kernels; the launcher
// (sparse_conv_direct_launch.hpp) maps a DirectForm onto its instantiation.  DESIGN.md 3b has the rule as a table.
#pragma once
#include "common.hpp"
#include "conv_common.hpp"

namespace epconv {
namespace {
using namespace ep;

constexpr int kRT = 2;   // 16-row tiles per wave
constexpr int kPersistWaves = 8;            // waves of the persistent form's one workgroup per CU,
constexpr int kJobRows = 16 * kRT;          // each pulling jobs of this many rows (the rows of its BatchNorm summary blocks)
constexpr int kShares = 8, kCtrStride = 16;  // its job counters: one per share of the jobs, 16 uints = 64 B apart,
constexpr size_t kPersistCtrBytes = (size_t)kShares * kCtrStride * sizeof(unsigned int);   // at the head of ConvParams::ws
constexpr size_t kLdsBytes = 160 * 1024;

// chunks per stage for a layer of KCH chunks: the stages of an offset are KCH / G
#ifndef EP_STAGE_CAP       // (probe builds: -DEP_STAGE_CAP=2 / 1 caps the chunks per stage — fewer registers, more waves per SIMD)
#define EP_STAGE_CAP 3
#endif
constexpr int stage_chunks(int kch) { return kch % 3 == 0 && EP_STAGE_CAP >= 3 ? 3 : (kch % 2 == 0 && EP_STAGE_CAP >= 2 ? 2 : 1); }
// ... and of the alternative with one more workgroup per CU (0: none; see select_direct_form).  (One chunk per stage for every
// layer — 80 registers, six waves per SIMD instead of three — measured no faster: 266 vs 250 us on 48 -> 24.)
constexpr int alt_stage_chunks(int kch) { return kch == 6 ? 2 : (kch == 3 ? 1 : 0); }

// dynamic LDS of the per-tile kernels: the map slice, the waves' BatchNorm summaries, the input's pending affine, the liveness flags
static size_t direct_lds_bytes(int K, int ct, int kch)
{
    return (size_t)K * kDirectRows * sizeof(int) + (size_t)kWaves * 3 * 16 * ct * sizeof(float) + (size_t)2 * 16 * kch * sizeof(float) +
           (size_t)K * kWaves * sizeof(int);
}

// ... and of the persistent form: the whole packing, the eight job windows, the affine
static size_t persist_lds_bytes(const ConvParams &p)
{
    const int kch = (p.Cin + 15) / 16, ct = (p.Cout + 15) / 16;
    const bool tail = p.Cout - 16 * (ct - 1) <= 8;
    const size_t quads = (size_t)(tail ? ct - 1 : ct) * 64 + (tail ? 32 : 0);
    return (size_t)p.K * kch * quads * 16 + (size_t)kPersistWaves * p.K * kJobRows * sizeof(int) + (size_t)2 * 16 * kch * sizeof(float);
}

static int device_cus()
{
    static int n = 0;
    if (!n) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        if (n <= 0) n = 256;
    }
    return n;
}

// The switches of the selection, read at every launch: tests flip them.  (The fifth, EPRECON_CONV_PERSIST, is read by persist_shape_ok,
// which the family selection asks at every convolution call: it reads nothing else while the opt-in is off.)
struct DirectSwitches {
    // EPRECON_CONV_TAIL8=0: C_out = 16 m + 8 on padded 16-column tiles (the round-5 form)
    bool tail8;
    // EPRECON_CONV_INTERLEAVE=0: the fenced schedule (loads of a stage, then the previous stage's MFMAs) for every launch of the
    // template kernel; default: branch-free layers spread the loads among the MFMAs.  Same arithmetic in the same order.
    bool interleave;
    // EPRECON_CONV_STAGE_DEPTH=0: always the deepest prefetch stage (the round-5 rule)
    bool stage_depth;
    // EPRECON_CONV_BF16X3=1: the template kernel's bf16x3 operand form (C_in <= 96, C_out <= 64).  OFF by default: the library's
    // results are exact-fp32 products; this is the opt-in with a stated error budget.
    bool bf16x3;
};
static DirectSwitches direct_switches()
{
    return {!switch_off("EPRECON_CONV_TAIL8"), !switch_off("EPRECON_CONV_INTERLEAVE"), !switch_off("EPRECON_CONV_STAGE_DEPTH"),
            switch_on("EPRECON_CONV_BF16X3")};
}

// the last column tile holds <= 8 columns and runs on the 4x4x1 MFMAs (also the row of the launcher's occupancy cache)
static bool direct_tail(const ConvParams &p, const DirectSwitches &sw)
{
    return p.Cout - 16 * ((p.Cout + 15) / 16 - 1) <= 8 && sw.tail8;
}

// (opt-in: any list with a job per wave of a few workgroups may take it)
constexpr int kPersistMinRows = 8192;

// EPRECON_CONV_PERSIST=1: long lists with LDS-sized weights on the persistent kernel.  OFF by default: measured equal to the
// per-tile kernel on the cfg4-leading layer (48 -> 24 on 320,868 rows: 203.6 against 203.3 us) and 10-19 % slower on the
// 198k-row layers, whose 24.2 jobs per CU are 2.02 per wave of three resident ones — a third round for 1 % of the jobs
// (profiles/r06/conv_forms_ab.txt).
// Shape rule, independent of the workspace: the selection and the summary-block rows ask this one.
static bool persist_shape_ok(const ConvParams &p)
{
    const int kch = (p.Cin + 15) / 16, ct = (p.Cout + 15) / 16;
    const bool rem8 = p.Cout - 16 * (ct - 1) <= 8;
    if (!switch_on("EPRECON_CONV_PERSIST") || kch > 6) return false;
    if (rem8 && switch_off("EPRECON_CONV_TAIL8")) return false; // (its 8-column tail is the 4x4x1 form)
    if (p.bn_partial && !p.flex_partial) return false;          // its summaries are per 32-row job
    if (persist_lds_bytes(p) > kLdsBytes) return false;
    // (the instantiated forms: only where a 27-offset packing can fit the LDS beside the eight job windows, <= 4.9 KB per offset;
    // the launcher's compile-time guards are this bound at rem8 = true / false)
    if (kch * ((rem8 ? ct - 1 : ct) * 1024 + (rem8 ? 512 : 0)) > 4864) return false;
    return p.n_out >= kPersistMinRows;
}
// ... and with the job counters the launch needs in its workspace (launch_persist refuses the launch without them)
static bool persist_ok(const ConvParams &p)
{
    return persist_shape_ok(p) && p.ws && (reinterpret_cast<uintptr_t>(p.ws) & 3) == 0 && p.ws_bytes >= kPersistCtrBytes;
}

// One instantiation: spconv_persist16_kernel<CT, KCH, tail> when `persist`, spconv_direct16_generic_kernel<CT> when g == 0,
// spconv_direct16_kernel<CT, KCH, tail, g, bf, mode> otherwise.
struct DirectForm {
    bool persist, tail, bf;
    int g, mode;
};

// occ_p / occ_a: workgroups per CU of the primary (stage_chunks) and the alternative (alt_stage_chunks) instantiation at this
// layer's tail form — equal where there is no alternative.
static DirectForm select_direct_form(const ConvParams &p, const DirectSwitches &sw, int cus_in, int occ_p, int occ_a)
{
    const int kch = (p.Cin + 15) / 16;
    DirectForm f = {false, false, false, 0, 0};
    if (kch > 6) return f;                      // any chunk count: run-time indices
    const int g0 = stage_chunks(kch);
    f.g = g0;
    // 1. the persistent form (its tail rule is persist_shape_ok's: with the 4x4x1 form switched off it is not eligible)
    if (persist_shape_ok(p)) {
        f.persist = true;
        f.tail = direct_tail(p, sw);
        return f;
    }
    // Branch-free layers (no ragged last chunk) take the interleaved instantiations: 1 without, 2 with a pending BatchNorm of
    // the input (profiles/r06/conv_interleave_ab.txt: -10 ... -12 % on 48 -> 24 / 80 -> 40 / 32 -> 24 / 48 -> 48 without,
    // -5 ... -18 % with); 3 / 4 the same for an 8-channel last chunk (C_in = 8, 24, 40) where it is part of every stage.
    int mode = 0;
    if (sw.interleave && (p.Cin & 3) == 0) {
        if (p.Cin - 16 * (kch - 1) > 8) mode = p.in_scale ? 2 : 1;
        else if (g0 == kch) mode = p.in_scale ? 4 : 3;
    }
    // 2. bf16x3 operands: padded tiles whatever the last tile holds (a half-empty tile costs 17 cycles there), modes 0 / 1 / 2
    if (sw.bf16x3) {
        f.bf = true;
        f.mode = mode > 2 ? 0 : mode;
        return f;
    }
    f.tail = direct_tail(p, sw);
    // 3. Medium lists (a few workgroups per CU): the kernel's registers allow two workgroups per CU for the wide layers (96 -> 48,
    // 48 -> 48: three chunks per stage), so 583 workgroups (74,568 rows) run as one full wave of 512 and a second one that is
    // 14 % full.  The same kernel with FEWER chunks per stage (fewer prefetch registers, one more workgroup per CU) is ~6 % slower
    // per workgroup and holds them all at once: 96 -> 48 on 74,568 rows 246 -> 199 us, 48 -> 48 on 93,513 rows 139 -> 116 us
    // (profiles/r06/conv_stage_depth_ab.txt).  Its instantiations are MODE 0: the layers WITH a pending BatchNorm stay on this
    // shallow fenced form (48 -> 48 on 93,513 rows 132.7 against 140.0 us), those without (modes 1, 3) keep the interleaved one.
    if (alt_stage_chunks(kch) != 0 && sw.stage_depth && occ_a > occ_p && mode != 1 && mode != 3) {
        const int64_t wgs = (unsigned)ceil_div(p.n_out, kDirectRows), cus = cus_in;
        // waves of workgroups x workgroups sharing a SIMD: what a launch costs in units of one workgroup running alone
        const double cost_p = (double)ceil_div(wgs, cus * occ_p) * occ_p;
        const double cost_a = (double)ceil_div(wgs, cus * occ_a) * occ_a * 1.06;
        if (cost_a < 0.85 * cost_p) {
            f.g = alt_stage_chunks(kch);
            return f;
        }
    }
    // 4. modes 4, 3, 2, 1, 0 at the deepest stage, with or without the tail
    f.mode = mode;
    return f;
}

}  // namespace
}  // namespace epconv
