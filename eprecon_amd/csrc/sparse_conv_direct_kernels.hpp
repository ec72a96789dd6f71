// Direct gather form of the 3x3x3 sparse convolution on v_mfma_f32_16x16x4_f32 for long lists (C_out <= 64): NO operand goes
// through LDS and there is no barrier in the loop, so the waves of a CU drift apart instead of staging, gathering and
// multiplying in lockstep (the phases of the LDS-resident kernel add up).
//   A operand (lane l: row l & 15, k index q = l >> 4): one 16-byte buffer gather x[nbr[k][row]][16 kc + 4 q .. + 3] per
//     (offset, 16-channel chunk) feeds four MFMAs; a missing neighbour is sent past the end of the buffer (zeros).
//   B operand: the weights pre-packed by pack_weights16_kernel in operand order (wq16), one coalesced 1 KB buffer load per
//     (offset, chunk, 16-column tile), served by L1 / L2 — every wave of the launch walks the same sequence.
//   A wave owns 2 x 16 rows and all CT column tiles (2 x CT accumulators of 4 VGPRs); the loads of the next stage (1..3
//   chunks) are in flight while the current one runs its MFMAs, unconditionally, so the waits are `vmcnt(<loads of a stage>)`.
// Timing ablations (profiles/r03/conv_direct_ablate.txt): with the gathers switched off and every weight load an L1 hit the
// first version of this kernel lost 8 % of its time — not memory but the instruction stream around the MFMAs (run-time
// (offset, chunk) arithmetic, masks) kept the matrix pipe at ~70 %: a 16x16x4 MFMA is 32 cycles, eight issue slots.  The
// chunk count is therefore a template parameter: offsets inside a stage are instruction immediates, one multiply + select
// per (offset, row tile), nothing else between the MFMAs.
// Summation order differs from the 32x32x2 kernels: equal within fp32 round-off, not bit for bit.
// (Instantiated per column-tile count by sparse_conv_direct_ct{1..4}.hip: four translation units compile side by side instead of
// one for two minutes.  Which instantiation a layer gets: sparse_conv_direct_select.hpp.)
#pragma once
#include "sparse_conv_direct_device.hpp"

namespace epconv {
namespace {

// TAIL: the last column tile holds <= 8 columns and runs on the 4x4x1 MFMAs (tail_to_tile); its B operands are the tail
// section of the packing (pack_weights16_kernel: behind the CT tiles, 512 B per (offset, chunk)).
// BF: the bf16x3 operand form (opt-in; padded 16-column tiles only: a half-empty tile costs 17 cycles there).
// MODE (select_direct_form's choice): 0 any layer; 1 / 2 branch-free layers without / with a pending BatchNorm of the input;
// 3 / 4 the same for layers whose last chunk holds <= 8 channels (C_in = 8, 24, 40) when an offset is one stage
// (see `consume` and the main loop)
template <int CT, int KCH, bool TAIL = false, int G = stage_chunks(KCH), bool BF = false, int MODE = 0>
__global__ __launch_bounds__(256) void spconv_direct16_kernel(ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RT = kRT, ROWS = kDirectRows;
    constexpr int CTM = TAIL ? CT - 1 : CT;          // full 16-column tiles on the 16x16x4 MFMA
    constexpr int CTA = CTM > 0 ? CTM : 1;           // (array extent: no zero-length arrays)
    constexpr int PARTS = KCH / G;
    constexpr int cpad = 16 * KCH;
    int *sNbr = reinterpret_cast<int *>(smem);                        // [K][ROWS]
    float *sStat = reinterpret_cast<float *>(sNbr + p.K * ROWS);      // [4 waves][3][16 CT]
    float *sAff = sStat + kWaves * 3 * 16 * CT;                       // [2][cpad]
    int *sFlag = reinterpret_cast<int *>(sAff + 2 * cpad);            // [K][4 waves] the wave has a neighbour at the offset
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    const int row0 = (int)blockIdx.x * ROWS;

    stage_in_affine<256>(p, sAff, cpad, tid);
    // Offsets none of the wave's 32 rows has a neighbour at are skipped altogether (no gathers, no weight loads, no MFMAs):
    // an output-stationary kernel otherwise multiplies zeros for every missing neighbour.  On the surface-shaped sets of a
    // fragment 12-25 % of the (32-row, offset) groups are dead; on the second voxelisation of ConvGRU's convr — already
    // scaled coordinates divided by the resolution again, models/modules.py:216-217: no two voxels are adjacent — 26 of the
    // 27 offsets are (profiles/r04/conv_tile_liveness.txt).
    const unsigned live = stage_map(p, row0, sNbr, sFlag, tid);

    // One full tile per row tile (C_out = 16, 24) leaves TWO independent 16x16x4 accumulators: consecutive MFMAs on one
    // accumulator issue 32 cycles apart but the result returns after 40 — a quarter of the matrix pipe's time in bubbles
    // (the compiler groups the 16x16x4s whatever order the source puts them in: ISA of round 6).  The channels of such a layer
    // are split over NS = 2 accumulator sets (components x, z / y, w of every gathered quad), summed once before the epilogue.
    static_assert(!(BF && TAIL), "the bf16x3 form runs on padded column tiles");
    static_assert(MODE < 3 || (G == KCH && !BF), "modes 3 / 4: one stage per offset, exact-fp32 form");

    constexpr int NS = (CTM == 1 && !BF) ? 2 : 1;
    f32x4 acc[NS][RT][CTA];
    f32x4 acct[RT][2];      // TAIL: per-k-slot partials of the last 8 columns (two groups of 4)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns)
#pragma unroll
            for (int t = 0; t < CTA; ++t) acc[ns][rt][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        acct[rt][0] = acct[rt][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, (int)p.x_bytes, 0x00020000);
    const unsigned row_bytes = (unsigned)p.ld_x * 4u, oob = (unsigned)p.x_bytes;
    const int U = __builtin_popcount(live) * PARTS;   // stages: (live offset, part)
    constexpr unsigned kChunkBytes = (unsigned)CT * 1024u;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq16), 0, (int)((unsigned)p.K * KCH * kChunkBytes), 0x00020000);
    const unsigned wlane = (unsigned)lane * 16u;
    // tail section: [K][KCH][2 column groups][4 k slots][4 columns] float4 = 512 B per (offset, chunk)
    const __amdgpu_buffer_rsrc_t wtrsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.wq16) + (size_t)p.K * KCH * CT * 256, 0, (int)((unsigned)p.K * KCH * 512u), 0x00020000);
    const unsigned tlane = (unsigned)(4 * q + (lane & 3)) * 16u;
    const int *myNbr = sNbr + wave * 16 * RT + l16;
    // a last chunk of <= 8 channels (C_in = 8, 24, 40): lane group q takes channels 2 q, 2 q + 1 and the chunk is two MFMAs
    const int last_c = p.Cin - 16 * (KCH - 1);      // channels of the last chunk
    const bool tail8 = last_c <= 8;
    const unsigned cq = 16u * (unsigned)q;
    const unsigned cq_last = tail8 ? 8u * (unsigned)q : cq;
    const bool last_ok = (tail8 ? 2 : 4) * q < last_c;

    struct Stage {
        float4 a[G][RT];
        float4 b[G][CTA];
        float4 bt[G][TAIL ? 2 : 1];
    };
    // stage u = (offset k = u / PARTS, chunks kc0 .. kc0 + G - 1 with kc0 = (u % PARTS) * G)
    auto fetch = [&](const LiveCursor &c, Stage &g) {
        const int k = c.k, part = c.part;                                // (wave-uniform: the weight offset below is a scalar)
        const unsigned xs = 64u * (unsigned)(part * G);                 // (scalar) byte offset of the stage's first chunk
        const unsigned ws = (EP_DIRECT_ABL & 8) ? 0u : (unsigned)(k * KCH + part * G) * kChunkBytes;
        const bool has_last = part == PARTS - 1;                         // (uniform) the stage holds the layer's last chunk
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            int j = myNbr[k * ROWS + 16 * rt];
            if (EP_DIRECT_ABL & 2) j = j >= 0 ? l16 : j;
            const unsigned rowsel = j >= 0 ? __umul24((unsigned)j, row_bytes) : oob;
            const unsigned v0 = rowsel + cq;
#pragma unroll
            for (int i = 0; i < G; ++i) {
                unsigned off = v0 + 64u * i;
                if (i == G - 1 && has_last) off = last_ok ? rowsel + cq_last + 64u * i : oob;
                if (EP_DIRECT_ABL & 4) {
                    g.a[i][rt] = make_float4(__uint_as_float(off), 1.0f, 2.0f, 3.0f);
                    continue;
                }
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, xs, 0);
                g.a[i][rt] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
#pragma unroll
            for (int t = 0; t < CTM; ++t) {
                if (EP_DIRECT_ABL & 32) {
                    g.b[i][t] = make_float4(__uint_as_float(ws), 1.0f, 2.0f, 3.0f);
                    continue;
                }
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)t * 1024u, ws + (unsigned)i * kChunkBytes, 0);
                g.b[i][t] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
            if constexpr (TAIL && (EP_DIRECT_ABL & 32)) {
                g.bt[i][0] = g.bt[i][1] = make_float4(__uint_as_float(ws), 1.0f, 2.0f, 3.0f);
            } else if constexpr (TAIL) {
                const unsigned wts = (EP_DIRECT_ABL & 8) ? 0u : (unsigned)(k * KCH + part * G + i) * 512u;
#pragma unroll
                for (int cg = 0; cg < 2; ++cg) {
                    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wtrsrc, tlane + (unsigned)cg * 256u, wts, 0);
                    g.bt[i][cg] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
                }
            }
        }
    };
    // MODE (compile time): 0 = every layer (launch-uniform branches on a pending BatchNorm of the input, an 8-channel or ragged
    // last chunk); 1 = C_in a multiple of 16... precisely: no 8-channel last chunk, no ragged count, no pending BatchNorm;
    // 2 = the same with a pending BatchNorm (+ ReLU, applied without a branch).  Modes 1 and 2 are ONE basic block: the main loop
    // below can then spread the next stage's loads among this stage's MFMAs.
    const unsigned relu_mask = p.in_relu ? 0xffffffffu : 0u;
    auto consume = [&](const LiveCursor &c, const Stage &g) {
        const int k = c.k, part = c.part;
        const bool has_last = part == PARTS - 1;
        BfQuad qa[BF ? G : 1][RT], qb[BF ? G : 1][CTA];                // BF: the stage's operands as bf16 (hi, lo) pairs
#pragma unroll
        for (int i = 0; i < G; ++i) {
            // (MODE 3 / 4: an 8-channel last chunk as a compile-time fact — the selection takes them only when an offset is ONE stage,
            // PARTS == 1, so that the last chunk of every stage is the layer's last)
            const bool t8 = MODE >= 3 ? i == G - 1 : (MODE == 0 && tail8 && i == G - 1 && has_last);   // .z / .w of the gathered values are not used
            float4 av[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) av[rt] = g.a[i][rt];
            if (MODE == 0 && (p.Cin & 3) && i == G - 1 && has_last) {   // (uniform) ragged channel count on a padded pitch: the pad lanes stay out
                const int c = 16 * (KCH - 1) + (t8 ? 2 : 4) * q;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    if (c + 1 >= p.Cin) av[rt].y = 0.0f;
                    if (c + 2 >= p.Cin) av[rt].z = 0.0f;
                    if (c + 3 >= p.Cin) av[rt].w = 0.0f;
                }
            }
            if (MODE == 2 || MODE == 4 || (MODE == 0 && p.in_scale)) {  // (uniform) the producer's pending BatchNorm (+ ReLU) on the gathered values
                const int kc = part * G + i;
                const int ca = 16 * kc + (t8 ? 2 : 4) * q;
                const float4 sc = make_float4(sAff[ca], sAff[ca + 1], sAff[ca + 2], sAff[ca + 3]);
                const float4 sh = make_float4(sAff[cpad + ca], sAff[cpad + ca + 1], sAff[cpad + ca + 2], sAff[cpad + ca + 3]);
                const bool cok = (i == G - 1 && has_last) ? last_ok : true;
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const bool ok = myNbr[k * ROWS + 16 * rt] >= 0 && cok;
                    float4 x = av[rt];
                    x.x = fmaf(x.x, sc.x, sh.x); x.y = fmaf(x.y, sc.y, sh.y); x.z = fmaf(x.z, sc.z, sh.z); x.w = fmaf(x.w, sc.w, sh.w);
                    if constexpr (MODE == 2 || MODE == 4) {      // (no branch: v_max + v_bfi per value; a NaN stays a NaN without the ReLU)
                        x.x = relu_sel(x.x, relu_mask); x.y = relu_sel(x.y, relu_mask);
                        x.z = relu_sel(x.z, relu_mask); x.w = relu_sel(x.w, relu_mask);
                    } else {
                        if (p.in_relu) { x.x = relu_nc(x.x); x.y = relu_nc(x.y); x.z = relu_nc(x.z); x.w = relu_nc(x.w); }
                        if (p.Cin & 3) {
                            const int c = ca;
                            if (c + 1 >= p.Cin) x.y = 0.0f;
                            if (c + 2 >= p.Cin) x.z = 0.0f;
                            if (c + 3 >= p.Cin) x.w = 0.0f;
                        }
                    }
                    av[rt] = ok ? x : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
            }
            if constexpr (BF) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    if (t8) av[rt].z = av[rt].w = 0.0f;     // (the fp32 form skips these two k slots; their weights are zeros)
                    qa[i][rt] = bf_split(av[rt]);
                }
#pragma unroll
                for (int t = 0; t < CTM; ++t) qb[i][t] = bf_split(g.b[i][t]);
                continue;
            }
            // independent accumulators alternate: a 16x16x4 MFMA issues every 32 cycles and returns after 40
#define EP_DIRECT_STEP(comp, set)                                                                                                    \
    do {                                                                                                                             \
        if (EP_DIRECT_ABL & 16) {                                                                                                    \
            _Pragma("unroll") for (int rt = 0; rt < RT; ++rt) {                                                                      \
                _Pragma("unroll") for (int t = 0; t < CTM; ++t) acc[0][rt][t][0] += av[rt].comp + g.b[i][t].comp;                    \
                if constexpr (TAIL) acct[rt][0][0] += av[rt].comp + g.bt[i][0].comp + g.bt[i][1].comp;                               \
            }                                                                                                                        \
            break;                                                                                                                   \
        }                                                                                                                            \
        _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                                                            \
            _Pragma("unroll") for (int t = 0; t < CTM; ++t)                                                                          \
                acc[(set) % NS][rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].comp, g.b[i][t].comp, acc[(set) % NS][rt][t], 0, 0, 0); \
        if constexpr (TAIL) {                                                                                                        \
            _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                                                        \
                _Pragma("unroll") for (int cg = 0; cg < 2; ++cg)                                                                     \
                    acct[rt][cg] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[rt].comp, g.bt[i][cg].comp, acct[rt][cg], 0, 0, 0);         \
        }                                                                                                                            \
    } while (0)
            EP_DIRECT_STEP(x, 0);
            EP_DIRECT_STEP(y, 1);
            if (!t8) {
                EP_DIRECT_STEP(z, 0);
                EP_DIRECT_STEP(w, 1);
            }
#undef EP_DIRECT_STEP
        }
        if constexpr (BF) {     // chunks in pairs on the K = 32 instruction, an odd last one on K = 16; three products each
#pragma unroll
            for (int i = 0; i + 1 < G; i += 2)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int t = 0; t < CTM; ++t) {
                        f32x4 c = acc[0][rt][t];
                        c = bf_mfma32(qa[i][rt].lo, qa[i + 1][rt].lo, qb[i][t].hi, qb[i + 1][t].hi, c);    // (small terms first)
                        c = bf_mfma32(qa[i][rt].hi, qa[i + 1][rt].hi, qb[i][t].lo, qb[i + 1][t].lo, c);
                        c = bf_mfma32(qa[i][rt].hi, qa[i + 1][rt].hi, qb[i][t].hi, qb[i + 1][t].hi, c);
                        acc[0][rt][t] = c;
                    }
            if constexpr (G & 1) {
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int t = 0; t < CTM; ++t) {
                        f32x4 c = acc[0][rt][t];
                        c = bf_mfma16(qa[G - 1][rt].lo, qb[G - 1][t].hi, c);
                        c = bf_mfma16(qa[G - 1][rt].hi, qb[G - 1][t].lo, c);
                        c = bf_mfma16(qa[G - 1][rt].hi, qb[G - 1][t].hi, c);
                        acc[0][rt][t] = c;
                    }
            }
        }
    };
    // Main loop.  The loads of stage u + 1 are in flight while stage u runs its MFMAs.  MODE 0: a scheduling fence between the two,
    // i.e. a burst of <= 15 loads, then <= 72 MFMAs.  MODE 1 / 2 (the consume step is one basic block): no fence — the loads are
    // spread among the MFMAs, one VMEM read per kMixMfma matrix instructions (sched_group_barrier), so a wave keeps feeding the
    // matrix pipe while its loads issue, and the registers of the stage in flight fill as they are needed (100 + 40 instead of
    // 144 + 24 on 48 -> 24): 5-8 % on the long lists (profiles/r06/conv_interleave_ab.txt).  An odd last stage is peeled off so
    // that the paired body holds no branch.  (One kernel holding both forms of the loop needs 236 + 44 registers: they are
    // separate instantiations.)
    if constexpr (MODE == 0) {
        if (!(p.debug & 1) && U > 0) {
            Stage s_a, s_b;
            LiveCursor cf(live), cc(live);     // the fetches run one to two stages ahead of the MFMAs
            fetch(cf, s_a);
            for (int u = 0; u < U; u += 2) {
                cf.next(PARTS);
                fetch(cf, s_b);
                __builtin_amdgcn_sched_barrier(0);
                consume(cc, s_a);
                cc.next(PARTS);
                __builtin_amdgcn_sched_barrier(0);
                cf.next(PARTS);
                fetch(cf, s_a);
                __builtin_amdgcn_sched_barrier(0);
                if (u + 1 < U) consume(cc, s_b);
                cc.next(PARTS);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    } else if (U > 0) {
        constexpr int kStageLoads = RT * G + G * CTM + (TAIL ? 2 * G : 0);
        constexpr int kStageMfma = BF ? 3 * RT * CTM * ((G + 1) / 2) : (G * 4 - (MODE >= 3 ? 2 : 0)) * (RT * CTM + (TAIL ? 2 * RT : 0));
        constexpr int kMixMfma = (kStageMfma + kStageLoads - 1) / kStageLoads + EP_MIX_EXTRA;
        Stage s_a, s_b;
        LiveCursor cf(live), cc(live);
        fetch(cf, s_a);
        auto mix = [&]() {
#pragma unroll
            for (int sg = 0; sg < kStageLoads; ++sg) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, kMixMfma, 0);
            }
        };
        int u = 0;
        for (; u + 1 < U; u += 2) {
            cf.next(PARTS);
            fetch(cf, s_b);
            consume(cc, s_a);
            mix();
            cc.next(PARTS);
            __builtin_amdgcn_sched_barrier(0);
            cf.next(PARTS);
            fetch(cf, s_a);
            consume(cc, s_b);
            mix();
            cc.next(PARTS);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (u < U) consume(cc, s_a);
    }
    if constexpr (NS == 2) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int t = 0; t < CTM; ++t) acc[0][rt][t] += acc[1][rt][t];
    }
    if constexpr (TAIL) {
        f32x4 full[RT][CT];
        f32x4 last[RT];
        tail_to_tile(acct, last, lane);
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int t = 0; t < CTM; ++t) full[rt][t] = acc[0][rt][t];
            full[rt][CT - 1] = last[rt];
        }
        direct_epilogue<CT>(p, full, row0, sStat);
    } else {
        direct_epilogue<CT>(p, acc[0], row0, sStat);
    }
}

// Any chunk count (C_in > 96): the (offset, chunk) sequence is walked with run-time indices, two chunks per stage.
template <int CT>
__global__ __launch_bounds__(256) void spconv_direct16_generic_kernel(ConvParams p, int kch)
{
    constexpr int RT = kRT, G = 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int ROWS = 64 * RT;
    int *sNbr = reinterpret_cast<int *>(smem);                        // [K][ROWS]
    float *sStat = reinterpret_cast<float *>(sNbr + p.K * ROWS);      // [4 waves][3][16 CT]
    const int cpad = 16 * kch;
    float *sAff = sStat + kWaves * 3 * 16 * CT;                       // [2][cpad]
    int *sFlag = reinterpret_cast<int *>(sAff + 2 * cpad);            // [K][4 waves] the wave has a neighbour at the offset
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    const int row0 = (int)blockIdx.x * ROWS;

    stage_in_affine<256>(p, sAff, cpad, tid);
    // (live offsets of the wave's 32 rows: see the template kernel)
    const unsigned live = stage_map(p, row0, sNbr, sFlag, tid);

    constexpr int NS = CT == 1 ? 2 : 1;       // (two accumulator sets for a single column tile: see the template kernel)
    f32x4 acc[NS][RT][CT];
#pragma unroll
    for (int ns = 0; ns < NS; ++ns)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[ns][rt][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, (int)p.x_bytes, 0x00020000);
    const unsigned row_bytes = (unsigned)p.ld_x * 4u, oob = (unsigned)p.x_bytes;
    const int S = __builtin_popcount(live) * kch;  // (live offset, chunk) steps
    const unsigned step_bytes = (unsigned)CT * 1024u;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq16), 0, (int)((unsigned)p.K * kch * step_bytes), 0x00020000);
    const unsigned wlane = (unsigned)lane * 16u;
    const int *myNbr = sNbr + wave * 16 * RT + l16;
    const unsigned cq = 16u * (unsigned)q;         // byte offset of this lane's four channels inside a chunk
    // a last chunk of <= 8 channels (C_in = 8, 24, 40): lane group q takes channels 2 q, 2 q + 1 and the chunk is two MFMAs
    const bool tail8 = p.Cin - 16 * (kch - 1) <= 8;

    struct Stage {
        float4 a[G][RT];
        float4 b[G][CT];
        unsigned live;      // bit (i * RT + rt): the neighbour of step i, row tile rt exists (only read with in_scale)
    };
    // the G steps at the cursor, which moves on (and stays on the last step: a step fetched past the end is not used)
    auto fetch = [&](LiveCursor &c, Stage &g) {
        g.live = 0u;
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int k = c.k, kc = c.part;
            c.next(kch);
            const bool t8 = tail8 && kc == kch - 1;                         // (uniform)
            const unsigned cbytes = 64u * (unsigned)kc + (t8 ? cq >> 1 : cq);
            const bool cok = 16 * kc + (t8 ? 2 : 4) * q < p.Cin;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int j = myNbr[k * ROWS + 16 * rt];
                const bool ok = j >= 0 && cok;
                const unsigned off = ok ? __umul24((unsigned)j, row_bytes) + cbytes : oob;
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0);
                g.a[i][rt] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
                g.live |= (ok ? 1u : 0u) << (i * RT + rt);
            }
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)t * 1024u, (unsigned)(k * kch + kc) * step_bytes, 0);
                g.b[i][t] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
        }
    };
    auto consume = [&](int s0, const Stage &g) {
#pragma unroll
        for (int i = 0; i < G; ++i) {
            if (s0 + i < S) {      // (uniform)
                float4 av[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) av[rt] = g.a[i][rt];
                const int kc = (s0 + i) % kch;
                const bool t8 = tail8 && kc == kch - 1;      // (uniform) .z / .w of the gathered values are not used
                if (p.Cin & 3) {   // (uniform) ragged channel count on a padded pitch: whatever sits in the pad lanes stays out
                    const int c = 16 * kc + (t8 ? 2 : 4) * q;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        if (c + 1 >= p.Cin) av[rt].y = 0.0f;
                        if (c + 2 >= p.Cin) av[rt].z = 0.0f;
                        if (c + 3 >= p.Cin) av[rt].w = 0.0f;
                    }
                }
                if (p.in_scale) {  // (uniform) the producer's pending BatchNorm (+ ReLU) on the gathered values
                    const int ca = 16 * kc + (t8 ? 2 : 4) * q;   // (8-byte aligned in the tail form: read as scalars)
                    const float4 sc = make_float4(sAff[ca], sAff[ca + 1], sAff[ca + 2], sAff[ca + 3]);
                    const float4 sh = make_float4(sAff[cpad + ca], sAff[cpad + ca + 1], sAff[cpad + ca + 2], sAff[cpad + ca + 3]);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        const bool ok = (g.live >> (i * RT + rt)) & 1u;
                        float4 x = av[rt];
                        x.x = fmaf(x.x, sc.x, sh.x); x.y = fmaf(x.y, sc.y, sh.y); x.z = fmaf(x.z, sc.z, sh.z); x.w = fmaf(x.w, sc.w, sh.w);
                        if (p.in_relu) { x.x = relu_nc(x.x); x.y = relu_nc(x.y); x.z = relu_nc(x.z); x.w = relu_nc(x.w); }
                        av[rt] = ok ? x : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    }
                }
                // independent accumulators alternate: a 16x16x4 MFMA issues every 32 cycles and returns after 40
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int t = 0; t < CT; ++t) acc[0 % NS][rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].x, g.b[i][t].x, acc[0 % NS][rt][t], 0, 0, 0);
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int t = 0; t < CT; ++t) acc[1 % NS][rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].y, g.b[i][t].y, acc[1 % NS][rt][t], 0, 0, 0);
                if (!t8) {
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int t = 0; t < CT; ++t) acc[0 % NS][rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].z, g.b[i][t].z, acc[0 % NS][rt][t], 0, 0, 0);
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int t = 0; t < CT; ++t) acc[1 % NS][rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].w, g.b[i][t].w, acc[1 % NS][rt][t], 0, 0, 0);
                }
            }
        }
    };
    if (!(p.debug & 1) && S > 0) {
        Stage s_a, s_b;
        LiveCursor cf(live);
        fetch(cf, s_a);
        for (int s0 = 0; s0 < S; s0 += 2 * G) {
            fetch(cf, s_b);
            __builtin_amdgcn_sched_barrier(0);
            consume(s0, s_a);
            __builtin_amdgcn_sched_barrier(0);
            fetch(cf, s_a);
            __builtin_amdgcn_sched_barrier(0);
            consume(s0 + G, s_b);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (NS == 2) {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[0][rt][0] += acc[1][rt][0];
    }
    direct_epilogue<CT>(p, acc[0], row0, sStat);
}

}  // namespace
}  // namespace epconv
