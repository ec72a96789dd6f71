// ---------------------------------------------------------------------------------------------
// Persistent form for long lists whose packed weights fit the LDS (round 6).  What the ablations of the template kernel say about
// the cfg4-leading layer (48 -> 24 on 320,868 rows, profiles/r06/conv_direct_ablate.txt): without its MFMAs the launch still
// takes 72 % of its time, without its weight loads 13 % less, without its gathers 13 % less — every wave re-reads the SAME
// operand-order weights through the vector L1 (9 of its 15 16-byte loads per offset; 64 B/clk/CU), and a wave stuck issuing
// loads cannot issue MFMAs.  Here ONE workgroup of 8 waves per CU copies the whole packing into LDS once (124 KB for 48 -> 24;
// ds_read_b128 delivers 256 B/clk/CU, no L1 traffic), and its waves then pull 32-row jobs from a device counter until the list
// is exhausted: no barrier after the prologue, no per-workgroup launch / staging cost, the dispatch balanced at the granularity
// of a wave's job whatever else runs on the chip.  The map slice of a job is staged by the wave itself in its own LDS window
// (the ballots of the staging passes are its live-offset mask); gathers, MFMA loop and epilogue are the direct kernel's; the
// BatchNorm summaries are per job (32 rows; the caller sizes them through eprecon_conv_desc_partial_rows).
// Job counters: same-address device atomics retire one per ~21 ns on this part (tools/probes/atomic_probe.hip), so ONE counter
// for the launch's ~12k pulls would cost more than the convolution (measured: 278 us).  The jobs are split into 8 contiguous
// shares — workgroup b pulls from share b % 8, the XCD the dispatcher puts it on when the chip is free; nothing depends on that —
// each with its own counter (next job) 64 bytes apart.  The counters are the first kPersistCtrBytes of the descriptor's
// workspace (eprecon_conv_desc_workspace_bytes asks for them) and launch_persist zeroes them on the stream in front of every
// launch: a launch polls only memory its caller handed it, and a captured launch replays the zeroing with it.  (A fill launch,
// not the runtime's memset: a captured hipMemsetAsync of more than four bytes replays its pattern correctly ONCE on this runtime
// and garbage from then on — profiles/r21/memset_node_probe.txt — and a garbage counter skips every job.)
// (kPersistWaves, kJobRows, the counters' layout and persist_lds_bytes sit in the selection header: the eligibility rule needs them
// without the kernel.)
// ---------------------------------------------------------------------------------------------
#pragma once
#include "sparse_conv_direct_device.hpp"

namespace epconv {
namespace {

template <int CT, int KCH, bool TAIL, int G = stage_chunks(KCH)>
__global__ __launch_bounds__(64 * kPersistWaves) void spconv_persist16_kernel(ConvParams p, int njobs, unsigned int *ctr)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int RT = kRT, ROWS = kJobRows;
    constexpr int CTM = TAIL ? CT - 1 : CT;
    constexpr int CTA = CTM > 0 ? CTM : 1;
    constexpr int PARTS = KCH / G;
    constexpr int cpad = 16 * KCH;
    constexpr int kQuads = CTM * 64 + (TAIL ? 32 : 0);      // float4s of one (offset, chunk) block in LDS
    float4 *sW = reinterpret_cast<float4 *>(smem);                                  // [K][KCH][kQuads]
    int *sNbr = reinterpret_cast<int *>(sW + (size_t)p.K * KCH * kQuads);           // [waves][K][32]
    float *sAff = reinterpret_cast<float *>(sNbr + kPersistWaves * p.K * ROWS);     // [2][cpad]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;

    {   // the packing -> LDS, once per CU
        const float4 *wm = reinterpret_cast<const float4 *>(p.wq16);
        const float4 *wt = wm + (size_t)p.K * KCH * CT * 64;
        const int blocks = p.K * KCH;
        for (int e = tid; e < blocks * kQuads; e += 64 * kPersistWaves) {
            const int blk = e / kQuads, r = e - blk * kQuads;
            sW[e] = r < CTM * 64 ? wm[(size_t)blk * CT * 64 + r] : wt[(size_t)blk * 32 + (r - CTM * 64)];
        }
    }
    stage_in_affine<64 * kPersistWaves>(p, sAff, cpad, tid);
    __syncthreads();

    const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, (int)p.x_bytes, 0x00020000);
    const unsigned row_bytes = (unsigned)p.ld_x * 4u, oob = (unsigned)p.x_bytes;
    int *wNbr = sNbr + wave * p.K * ROWS;
    const int *myNbr = wNbr + l16;
    const int last_c = p.Cin - 16 * (KCH - 1);
    const bool tail8 = last_c <= 8;
    const unsigned cq = 16u * (unsigned)q;
    const unsigned cq_last = tail8 ? 8u * (unsigned)q : cq;
    const bool last_ok = (tail8 ? 2 : 4) * q < last_c;
    const int tq = CTM * 64 + 4 * q + (lane & 3);       // this lane's float4 of a block's tail section (+ 16 cg)
    const int total = p.K * ROWS;

    struct Stage {
        float4 a[G][RT];
        float4 b[G][CTA];
        float4 bt[G][TAIL ? 2 : 1];
    };

    // this workgroup's share of the jobs: [job_lo, job_hi)
    const unsigned share = blockIdx.x % (unsigned)kShares;
    ctr += share * kCtrStride;
    const unsigned per = ((unsigned)njobs + kShares - 1) / kShares;
    const unsigned job_lo = share * per, job_hi = min(job_lo + per, (unsigned)njobs);
    unsigned job = 0;
    if (lane == 0) job = atomicAdd(ctr, 1u);
    job = (unsigned)__builtin_amdgcn_readfirstlane((int)job) + job_lo;
    while (job < job_hi) {
        const int row0 = (int)job * ROWS;
        // the job's slice of the kernel map -> the wave's LDS window [K][32]; pass `it` covers offsets 2 it (lanes 0 .. 31) and
        // 2 it + 1: the halves of its ballot are those offsets' liveness
        unsigned live = 0u;
        {
            int jv[kMapLoads];
#pragma unroll
            for (int it = 0; it < kMapLoads; ++it) {
                const int e = lane + 64 * it;
                const int k = e >> 5, row = row0 + (e & 31);
                int j = -1;
                if (e < total && row < p.n_out) j = p.nbr ? p.nbr[(size_t)k * p.n_out + row] : row;
                jv[it] = j;
            }
#pragma unroll
            for (int it = 0; it < kMapLoads; ++it) {
                const int e = lane + 64 * it;
                if (e < total) wNbr[e] = jv[it];
                const unsigned long long b = __ballot(jv[it] >= 0);
                live |= ((unsigned)b != 0u ? 1u : 0u) << (2 * it);
                live |= ((unsigned)(b >> 32) != 0u ? 1u : 0u) << (2 * it + 1);
            }
        }
        live = (unsigned)__builtin_amdgcn_readfirstlane((int)live);
        unsigned next = 0;
        if (lane == 0) next = atomicAdd(ctr, 1u);            // the next job's index travels while this one runs
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the window is written before any lane reads another lane's entry

        constexpr int NS = CTM == 1 ? 2 : 1;       // (two accumulator sets when a row tile has one full column tile: see the template kernel)
        f32x4 acc[NS][RT][CTA];
        f32x4 acct[RT][2];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
            for (int ns = 0; ns < NS; ++ns)
#pragma unroll
                for (int t = 0; t < CTA; ++t) acc[ns][rt][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            acct[rt][0] = acct[rt][1] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
        const int U = __builtin_popcount(live) * PARTS;

        auto fetch = [&](const LiveCursor &c, Stage &g) {
            const int k = c.k, part = c.part;
            const unsigned xs = 64u * (unsigned)(part * G);
            const bool has_last = part == PARTS - 1;
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const int j = myNbr[k * ROWS + 16 * rt];
                const unsigned rowsel = j >= 0 ? __umul24((unsigned)j, row_bytes) : oob;
                const unsigned v0 = rowsel + cq;
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    unsigned off = v0 + 64u * i;
                    if (i == G - 1 && has_last) off = last_ok ? rowsel + cq_last + 64u * i : oob;
                    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, xs, 0);
                    g.a[i][rt] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
                }
            }
            const float4 *wb = sW + (size_t)(k * KCH + part * G) * kQuads;
#pragma unroll
            for (int i = 0; i < G; ++i) {
#pragma unroll
                for (int t = 0; t < CTM; ++t) g.b[i][t] = wb[i * kQuads + t * 64 + lane];
                if constexpr (TAIL) {
                    g.bt[i][0] = wb[i * kQuads + tq];
                    g.bt[i][1] = wb[i * kQuads + tq + 16];
                }
            }
        };
        auto consume = [&](const LiveCursor &c, const Stage &g) {
            const int k = c.k, part = c.part;
            const bool has_last = part == PARTS - 1;
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const bool t8 = tail8 && i == G - 1 && has_last;
                float4 av[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) av[rt] = g.a[i][rt];
                if ((p.Cin & 3) && i == G - 1 && has_last) {
                    const int c = 16 * (KCH - 1) + (t8 ? 2 : 4) * q;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        if (c + 1 >= p.Cin) av[rt].y = 0.0f;
                        if (c + 2 >= p.Cin) av[rt].z = 0.0f;
                        if (c + 3 >= p.Cin) av[rt].w = 0.0f;
                    }
                }
                if (p.in_scale) {
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
                        if (p.in_relu) { x.x = relu_nc(x.x); x.y = relu_nc(x.y); x.z = relu_nc(x.z); x.w = relu_nc(x.w); }
                        if (p.Cin & 3) {
                            if (ca + 1 >= p.Cin) x.y = 0.0f;
                            if (ca + 2 >= p.Cin) x.z = 0.0f;
                            if (ca + 3 >= p.Cin) x.w = 0.0f;
                        }
                        av[rt] = ok ? x : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    }
                }
#define EP_PERSIST_STEP(comp, set)                                                                                                   \
    do {                                                                                                                             \
        _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                                                            \
            _Pragma("unroll") for (int t = 0; t < CTM; ++t)                                                                          \
                acc[(set) % NS][rt][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[rt].comp, g.b[i][t].comp, acc[(set) % NS][rt][t], 0, 0, 0); \
        if constexpr (TAIL) {                                                                                                        \
            _Pragma("unroll") for (int rt = 0; rt < RT; ++rt)                                                                        \
                _Pragma("unroll") for (int cg = 0; cg < 2; ++cg)                                                                     \
                    acct[rt][cg] = __builtin_amdgcn_mfma_f32_4x4x1f32(av[rt].comp, g.bt[i][cg].comp, acct[rt][cg], 0, 0, 0);         \
        }                                                                                                                            \
    } while (0)
                EP_PERSIST_STEP(x, 0);
                EP_PERSIST_STEP(y, 1);
                if (!t8) {
                    EP_PERSIST_STEP(z, 0);
                    EP_PERSIST_STEP(w, 1);
                }
#undef EP_PERSIST_STEP
            }
        };
        if (U > 0) {
            Stage s_a, s_b;
            LiveCursor cf(live), cc(live);
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
            direct_epilogue<CT, true>(p, full, row0, nullptr, (int)job);
        } else {
            direct_epilogue<CT, true>(p, acc[0], row0, nullptr, (int)job);
        }
        job = (unsigned)__builtin_amdgcn_readfirstlane((int)next) + job_lo;
    }
}

template <int CT, int KCH, bool TAIL>
int launch_persist(const ConvParams &p, hipStream_t st)
{
    // (the caller sized its summaries for 32-row jobs: no other kernel can stand in for a launch that came without its counters)
    if (!persist_ok(p)) return EPRECON_ERR_WORKSPACE;
    static bool attr_set = false;
    auto kern = spconv_persist16_kernel<CT, KCH, TAIL>;
    if (!attr_set) {
        EP_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
        attr_set = true;
    }
    unsigned int *ctr = static_cast<unsigned int *>(p.ws);
    const FillRegion zero = {ctr, kPersistCtrBytes, 0u};
    const int rc = multi_fill(&zero, 1, st);
    if (rc != EPRECON_OK) return rc;
    const int njobs = ceil_div(p.n_out, kJobRows);
    const int grid = max(kShares, min(device_cus(), ceil_div(njobs, kPersistWaves)));    // (every share has a workgroup)
    hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(64 * kPersistWaves), persist_lds_bytes(p), st, p, njobs, ctr);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // namespace
}  // namespace epconv
