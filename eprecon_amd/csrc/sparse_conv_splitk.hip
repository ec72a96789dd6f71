// ---------------------------------------------------------------------------------------------
// Short lists with wide inputs (a few thousand voxels / the 10,800 pixels of the 1/16 maps, C_in > 64):
// there are too few 128-row tiles to fill the chip, nothing overlaps, and the slab kernel's time is the
// LENGTH of its dependent chain: K * ceil(C_in / 32) staged slabs, each a global round trip + barrier
// (108 for a 27-offset 128-channel layer, ~130 us).  Here a workgroup owns 32 rows x 32 columns and its
// four waves split the (offset, slab) list round-robin, each staging its own slabs into a wave-private LDS
// buffer (no workgroup barrier in the loop); the four partial accumulators are summed in fixed order
// through LDS at the end.  4x the workgroups, 1/4 of the chain.
// ---------------------------------------------------------------------------------------------
#include "common.hpp"
#include "conv_common.hpp"
#include "conv_gather.hpp"

namespace {
using namespace ep;
using namespace epconv;

// RT = 2: the workgroup owns 64 rows (two 32-row tiles per wave, two accumulators) and every staged weight slab feeds
// both — half the slab round trips per row and half the weight traffic; taken when the list is still long enough to
// fill the chip with 64-row workgroups.
constexpr int splitk_w_floats(int rt, int nw)
{
    return rt * (nw - 1) * 16 * 64 > nw * 32 * 32 ? rt * (nw - 1) * 16 * 64 : nw * 32 * 32;
}

// NW: waves per workgroup (4, or 8 / 16 when the 32-row x 32-column workgroups alone leave most SIMDs idle)
// ACC: the BatchNorm accumulator-block forms of prologue and epilogue (EPRECON_BN_ACC=1) are their own instantiations — compiled
// into the default ones they cost split-K<true, 1, 8> twelve registers and a wave per SIMD (43 -> 53 us on 7,561 rows 80 -> 48)
// FAST (16-byte gathers + packed weights, the launcher's choice): the stage loop holds NO launch-uniform branch — packed weights
// are a compile-time fact, every slab runs its four 8-channel chunks (a chunk past C_in multiplies zeros: the gathered values are
// masked, the weight loads clamped), the pending BatchNorm of the input is the AFF instantiation — so a stage's loads and its
// 16 RT MFMAs are ONE basic block the compiler schedules together (round 6: 128 -> 96 on 9,324 rows 115.6 -> 91.5 us, 48 -> 48 on
// 7,561 rows 41.9 -> 31.7, 32 -> 32 on 10,121 rows 29.7 -> 20.9; profiles/r06/conv_splitk_flat_ab.txt).  The same products in
// the same order as the general form: bit-identical.
template <bool VEC4, int RT, int NW, bool ACC = false, bool FAST = false, bool AFF = false>
__global__ __launch_bounds__(64 * NW) void spconv_splitk_kernel(ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TN = 32;
    constexpr int ROWS = 32 * RT;
    float *sW = reinterpret_cast<float *>(smem);                  // [NW waves][32][32] wave-private weight slabs
    float *sRed = sW;                                             // overlay after the loop: [RT][NW - 1][16][64] partial accumulators
    constexpr int THREADS = 64 * NW;
    constexpr int w_floats = splitk_w_floats(RT, NW);
    int *sNbr = reinterpret_cast<int *>(sW + w_floats);           // [K][ROWS]
    int *sActive = sNbr + p.K * ROWS;                             // [K]
    int *sLive = sActive + ((p.K + 3) & ~3);                      // [K] live offsets in order, [K]: their number
    const int cinA = (p.Cin + 3) & ~3;
    float *sAff = reinterpret_cast<float *>(sLive + ((p.K + 4) & ~3));  // [2][cinA]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int row0 = blockIdx.x * ROWS;
    const int col0 = blockIdx.y * TN;

    for (int k = tid; k < p.K; k += THREADS) sActive[k] = 0;
    stage_in_affine<THREADS, ACC>(p, sAff, cinA, tid);
    __syncthreads();
    for (int e = tid; e < p.K * ROWS; e += THREADS) {
        const int k = e / ROWS, r = e - k * ROWS;
        const int row = row0 + r;
        int j = -1;
        if (row < p.n_out) j = p.nbr ? p.nbr[(size_t)k * p.n_out + row] : row;
        sNbr[e] = j;
        if (j >= 0) sActive[k] = 1;  // benign race: every writer stores 1
    }
    __syncthreads();

    f32x16 acc[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int nslab = (p.Cin + 31) / 32;
    float *myW = sW + wave * 32 * TN;
    // Pipelined form (16-byte gathers, 16-byte weight rows): the (live offset, slab) stages of this wave are walked with the
    // NEXT stage's weight slab and neighbour values already in flight while the current one runs its 16 x RT MFMAs.  Every
    // prefetch is unconditional (addresses clamped, values masked at use) so that the waits stay `vmcnt(<loads of one stage>)`.
    const bool w_v4 = (p.Cout & 3) == 0 && ((p.Cout - col0) & 3) == 0 && (reinterpret_cast<uintptr_t>(p.w) & 15) == 0;
    // bdirect: the caller packed the weights in MFMA operand order (pack_weights_kernel, p.wq): the B operands of a stage are
    // four 16-byte loads straight into registers — no slab in LDS, no ds_read per MFMA pair, no wave barrier
    // (the 1,024-thread form sits at its 128-register cap: its 16-byte instantiation is launched with packed weights only and
    // compiles the LDS-slab stages and the unpipelined loop out — with them it spilled eight registers to scratch)
    static_assert(!FAST || (VEC4 && !ACC), "the branch-free form: 16-byte gathers, packed weights, per-workgroup summaries");
    constexpr bool BD_ONLY = VEC4 && (NW == 16 || FAST);
    const bool bdirect = BD_ONLY || (p.wq != nullptr && p.splitk_pipe == 2);
    if (BD_ONLY || (VEC4 && (w_v4 || bdirect) && p.splitk_pipe)) {
        if (tid == 0) {
            int n = 0;
            for (int k = 0; k < p.K; ++k)
                if (sActive[k]) sLive[n++] = k;
            sLive[p.K] = n;
        }
        __syncthreads();
        const int nst = sLive[p.K] * nslab;
        const int nq = min(p.Cout - col0, TN) / 4;
        struct Stage {
            float4 w4[4];
            float4 a[RT][4];
            int j[RT];
            int c0;
        };
        // packed layout (pack_weights_kernel): wq[(((((cb * K + k) * NCH8 + ch) * 2 + half) * NTP + t) * 32 + col) * 4 + s]
        const int nch8 = (p.Cin + 7) / 8;
        const int ntp = p.Cout <= 32 ? 1 : 2;
        const int cbp = (int)blockIdx.y / ntp, tp = (int)blockIdx.y - cbp * ntp;
        const float *wq_lane = p.wq ? p.wq + ((size_t)half * ntp + tp) * 128 + (size_t)r32 * 4 : nullptr;
        auto fetch = [&](int st, Stage &g) {
            const int k = sLive[st / nslab];
            g.c0 = (st % nslab) * 32;
            if (bdirect) {
                const float *wb = wq_lane + ((size_t)(cbp * p.K + k) * nch8) * (2 * ntp * 128);
#pragma unroll
                for (int it = 0; it < 4; ++it)   // chunk it of the slab (clamped: a chunk past C_in multiplies zeros)
                    g.w4[it] = *reinterpret_cast<const float4 *>(wb + (size_t)min(g.c0 / 8 + it, nch8 - 1) * (2 * ntp * 128));
            } else {
                const float *wk = p.w + (size_t)k * p.Cin * p.Cout + col0;
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int e = lane + it * 64, r = e >> 3, q = e & 7;
                    g.w4[it] = *reinterpret_cast<const float4 *>(wk + (size_t)min(g.c0 + r, p.Cin - 1) * p.Cout + 4 * min(q, nq - 1));
                }
            }
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                g.j[t] = sNbr[k * ROWS + t * 32 + r32];
                const float *xrow = p.x + (size_t)max(g.j[t], 0) * p.ld_x;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int c = g.c0 + ch * 8 + 4 * half;
                    g.a[t][ch] = *reinterpret_cast<const float4 *>(xrow + min(c, cinA - 4));
                }
            }
        };
        // (two stages ahead — 247 registers at RT = 2 — measured no faster: 165 vs 161 us on 9,415 rows 192 -> 96; the 64-row
        // workgroups of that launch run in two rounds of ~80 us on one workgroup per CU, which is what sets its time)
        const unsigned relu_mask = p.in_relu ? 0xffffffffu : 0u;
        Stage cur, nxt;
        if (wave < nst) fetch(wave, cur);
        if constexpr (FAST) {
            // Branch-free form: the pending BatchNorm (AFF) and the masks are applied to a stage's gathered values ONE STAGE AHEAD —
            // to `nxt`, behind the MFMAs of `cur` in program order, so that the vector ALU works in the shadow of the matrix pipe
            // instead of between a stage's loads and its first MFMA.  Same values, same products, same order.
            auto prep = [&](Stage &g) {
                const int c0 = g.c0;
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int c = c0 + ch * 8 + 4 * half;
                    float sc[4] = {1.f, 1.f, 1.f, 1.f}, sh[4] = {0.f, 0.f, 0.f, 0.f};
                    if constexpr (AFF) {
                        const int cc = min(c, cinA - 4);
                        const float4 sc4 = *reinterpret_cast<const float4 *>(sAff + cc);
                        const float4 sh4 = *reinterpret_cast<const float4 *>(sAff + cinA + cc);
                        sc[0] = sc4.x; sc[1] = sc4.y; sc[2] = sc4.z; sc[3] = sc4.w;
                        sh[0] = sh4.x; sh[1] = sh4.y; sh[2] = sh4.z; sh[3] = sh4.w;
                    }
#pragma unroll
                    for (int t = 0; t < RT; ++t) {
                        float v[4] = {g.a[t][ch].x, g.a[t][ch].y, g.a[t][ch].z, g.a[t][ch].w};
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            if constexpr (AFF) {
                                const float x = fmaf(v[q], sc[q], sh[q]);
                                const unsigned r = __float_as_uint(fmaxf(x, 0.0f)), b = __float_as_uint(x);
                                v[q] = __uint_as_float((r & relu_mask) | (b & ~relu_mask));
                            }
                            v[q] = (g.j[t] >= 0 && c + q < p.Cin) ? v[q] : 0.0f;
                        }
                        g.a[t][ch] = make_float4(v[0], v[1], v[2], v[3]);
                    }
                }
            };
            if (wave < nst) prep(cur);
            for (int st = wave; st < nst; st += NW) {
                fetch(min(st + NW, nst - 1), nxt);
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const float bw[4] = {cur.w4[ch].x, cur.w4[ch].y, cur.w4[ch].z, cur.w4[ch].w};
#pragma unroll
                    for (int t = 0; t < RT; ++t) {
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[t][ch].x, bw[0], acc[t], 0, 0, 0);
                    }
#pragma unroll
                    for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[t][ch].y, bw[1], acc[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[t][ch].z, bw[2], acc[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(cur.a[t][ch].w, bw[3], acc[t], 0, 0, 0);
                }
                // (the stage fetched past the end is not consumed: with sixteen waves — a few stages each — and a BatchNorm to apply,
                // skipping its preparation is worth the branch; everywhere else the branch costs more than the work it saves)
                if constexpr (AFF && NW == 16) {
                    if (st + NW < nst) prep(nxt);
                } else {
                    prep(nxt);
                }
                cur = nxt;
            }
        } else
        for (int st = wave; st < nst; st += NW) {
            fetch(min(st + NW, nst - 1), nxt);
            const int c0 = cur.c0;
            if (!bdirect) {
#pragma unroll
                for (int it = 0; it < 4; ++it) {
                    const int e = lane + it * 64, r = e >> 3, q = e & 7;
                    reinterpret_cast<float4 *>(myW)[e] = (c0 + r < p.Cin && q < nq) ? cur.w4[it] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            float a[RT][4][4];
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    a[t][ch][0] = cur.a[t][ch].x; a[t][ch][1] = cur.a[t][ch].y;
                    a[t][ch][2] = cur.a[t][ch].z; a[t][ch][3] = cur.a[t][ch].w;
                }
            if (FAST ? AFF : p.in_scale != nullptr) {   // the producer's pending BatchNorm (+ ReLU): this lane's 16 channels of the slab
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int cc = min(c0 + ch * 8 + 4 * half, cinA - 4);
                    const float4 sc4 = *reinterpret_cast<const float4 *>(sAff + cc);
                    const float4 sh4 = *reinterpret_cast<const float4 *>(sAff + cinA + cc);
                    const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
#pragma unroll
                    for (int t = 0; t < RT; ++t)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const float x = fmaf(a[t][ch][q], sc[q], sh[q]);
                            if constexpr (FAST) {   // (no branch: the ReLU's result chosen by a launch-uniform bit mask — same bits)
                                const unsigned r = __float_as_uint(fmaxf(x, 0.0f)), b = __float_as_uint(x);
                                a[t][ch][q] = __uint_as_float((r & relu_mask) | (b & ~relu_mask));
                            } else {
                                a[t][ch][q] = p.in_relu ? fmaxf(x, 0.0f) : x;
                            }
                        }
                }
            }
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int c = c0 + ch * 8 + 4 * half;
#pragma unroll
                    for (int q = 0; q < 4; ++q) a[t][ch][q] = (cur.j[t] >= 0 && c + q < p.Cin) ? a[t][ch][q] : 0.0f;
                }
            const int nch = FAST ? 4 : min(4, (p.Cin - c0 + 7) / 8);
            if (bdirect) {
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    if (FAST || ch < nch) {
                        const float bw[4] = {cur.w4[ch].x, cur.w4[ch].y, cur.w4[ch].z, cur.w4[ch].w};
#pragma unroll
                        for (int q = 0; q < 4; ++q)
#pragma unroll
                            for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][ch][q], bw[q], acc[t], 0, 0, 0);
                    }
                }
            } else {
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {   // (unrolled with a uniform guard: register indices stay static)
                    if (ch < nch) {
                        float bw[4];
#pragma unroll
                        for (int q = 0; q < 4; ++q) bw[q] = myW[(ch * 8 + 4 * half + q) * TN + r32];
#pragma unroll
                        for (int q = 0; q < 4; ++q)
#pragma unroll
                            for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][ch][q], bw[q], acc[t], 0, 0, 0);
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
            cur = nxt;
        }
    } else {
    int stage = 0;  // counts (live offset, slab) pairs; this wave takes those with stage % NW == wave
    for (int k = 0; k < p.K; ++k) {
        if (!sActive[k]) continue;  // block-uniform
        int j[RT];
        const float *xrow[RT];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            j[t] = sNbr[k * ROWS + t * 32 + r32];
            xrow[t] = p.x + (size_t)(j[t] >= 0 ? j[t] : 0) * p.ld_x;
        }
        const float *wk = p.w + (size_t)k * p.Cin * p.Cout + col0;
        for (int sl = 0; sl < nslab; ++sl, ++stage) {
            if (stage % NW != wave) continue;  // wave-uniform
            const int c0 = sl * 32;
            // ---- this wave's weight slab W[k][c0 : c0+32][col0 : col0+32] -> its private LDS buffer ----
            {
                const int ncols = p.Cout - col0;
                const bool v4 = (p.Cout & 3) == 0 && (ncols & 3) == 0 && (reinterpret_cast<uintptr_t>(wk) & 15) == 0;
                if (v4) {
                    const int nq = min(ncols, TN) / 4;
                    float4 w4[4];
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int e = lane + it * 64, r = e >> 3, q = e & 7;
                        w4[it] = *reinterpret_cast<const float4 *>(wk + (size_t)min(c0 + r, p.Cin - 1) * p.Cout + 4 * min(q, nq - 1));
                    }
#pragma unroll
                    for (int it = 0; it < 4; ++it) {
                        const int e = lane + it * 64, r = e >> 3, q = e & 7;
                        reinterpret_cast<float4 *>(myW)[e] = (c0 + r < p.Cin && q < nq) ? w4[it] : make_float4(0.f, 0.f, 0.f, 0.f);
                    }
                } else {
#pragma unroll 4
                    for (int e = lane; e < 32 * TN; e += 64) {
                        const int r = e >> 5, col = e & 31;
                        const float v = wk[(size_t)min(c0 + r, p.Cin - 1) * p.Cout + min(col, ncols - 1)];
                        myW[e] = (c0 + r < p.Cin && col < ncols) ? v : 0.0f;
                    }
                }
            }
            // ---- this lane's A values: per row tile 4 chunks of 8 channels, 4 floats each ----
            float a[RT][4][4];
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int c = c0 + ch * 8 + 4 * half;
                    if (VEC4) {
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (j[t] >= 0 && c < p.Cin) v = *reinterpret_cast<const float4 *>(xrow[t] + c);
                        if (p.Cin & 3) {
                            if (c + 1 >= p.Cin) v.y = 0.0f;
                            if (c + 2 >= p.Cin) v.z = 0.0f;
                            if (c + 3 >= p.Cin) v.w = 0.0f;
                        }
                        a[t][ch][0] = v.x; a[t][ch][1] = v.y; a[t][ch][2] = v.z; a[t][ch][3] = v.w;
                    } else {
#pragma unroll
                        for (int q = 0; q < 4; ++q) a[t][ch][q] = (j[t] >= 0 && c + q < p.Cin) ? xrow[t][c + q] : 0.0f;
                    }
                }
            if (p.in_scale) {
#pragma unroll
                for (int t = 0; t < RT; ++t)
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) {
                        const int c = c0 + ch * 8 + 4 * half;
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const bool ok = j[t] >= 0 && c + q < p.Cin;
                            float v = fmaf(a[t][ch][q], sAff[min(c + q, cinA - 1)], sAff[cinA + min(c + q, cinA - 1)]);
                            if (p.in_relu) v = fmaxf(v, 0.0f);
                            a[t][ch][q] = ok ? v : 0.0f;
                        }
                    }
            }
            __builtin_amdgcn_wave_barrier();  // the slab stores above precede the loads below (same wave, LDS is in order)
            const int nch = min(4, (p.Cin - c0 + 7) / 8);
            for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float bw = myW[(ch * 8 + 4 * half + q) * TN + r32];
#pragma unroll
                    for (int t = 0; t < RT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t][ch][q], bw, acc[t], 0, 0, 0);
                }
            }
            __builtin_amdgcn_wave_barrier();  // the next stage overwrites myW
        }
    }
    }
    // ---- fixed-order sum of the NW partial accumulators (waves 1.. -> LDS, wave 0 adds them in order) ----
    __syncthreads();
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                sRed[((t * (NW - 1) + wave - 1) * 16 + r) * 64 + lane] = acc[t][r];
                acc[t][r] = 0.0f;
            }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int w = 0; w < NW - 1; ++w)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] += sRed[((t * (NW - 1) + w) * 16 + r) * 64 + lane];
    }
    __syncthreads();  // sRed is read; the epilogue reuses the region for the BatchNorm summaries
    // waves 1.. hold no rows: an empty row map keeps them out of the stores and the statistics (the shared epilogue has
    // kWaves summary slots: the extra waves of a wide workgroup all write the same empty summary into the last one)
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        if (t > 0 && row0 + 32 * t >= p.n_out) break;  // (block-uniform) no second tile in the last workgroup
        f32x16 one[1] = {acc[t]};
        const LinearRows rm{row0 + 32 * t, wave == 0 ? p.n_out : 0};
        conv_epilogue<1, ACC>(p, one, rm, col0, r32, half, min(wave, kWaves - 1), sW, (int)blockIdx.x * RT + t, (int)gridDim.y);
        if (t + 1 < RT) __syncthreads();  // the next tile's summaries reuse the scratch
    }
}

template <bool VEC4>
int launch_splitk_v(ConvParams &p, hipStream_t st)
{
    // software-pipelined stages; with the caller's operand-order packing (p.wq) the B operands bypass LDS
    p.splitk_pipe = (p.wq && (reinterpret_cast<uintptr_t>(p.wq) & 15) == 0) ? 2 : 1;
    const int colb = (int)ceil_div(p.Cout, 32);
    // (3D kernel maps only: the K = 9 layers of the 10,800-pixel maps measured slower with 64-row workgroups, 52 vs 47 us)
    const bool rt2 = p.K >= 27 && ceil_div(p.n_out, 64) * colb >= 320;
    const int rows = rt2 ? 64 : 32;
    const dim3 grid((unsigned)ceil_div(p.n_out, rows), (unsigned)colb);
    // waves per workgroup: four; more when four per workgroup leave SIMDs without a wave and the chain is long enough to split
    const int64_t wgs = (int64_t)grid.x * grid.y;
    const int stages = p.K * ((p.Cin + 31) / 32);
    int nw = 4;
    // (a pending BatchNorm held as an accumulator block, EPRECON_BN_ACC=1, is finished in the prologue: the 1,024-thread form
    // has no registers to spare for that — its instantiation compiles the block path out — and takes eight waves then)
    if (!rt2 && wgs * 16 <= 4096 && stages >= 32 && !p.in_acc && !p.bn_acc && (!VEC4 || p.splitk_pipe == 2)) nw = 16;
    else if (wgs * 8 <= 4096 && stages >= 16) nw = 8;
    const size_t w_floats = (size_t)splitk_w_floats(rt2 ? 2 : 1, nw);
    const size_t lds = w_floats * sizeof(float) + (size_t)p.K * rows * sizeof(int) +
                       (size_t)(((p.K + 3) & ~3) + ((p.K + 4) & ~3)) * sizeof(int) + (size_t)2 * ((p.Cin + 3) & ~3) * sizeof(float) + 16;
    // (128-row workgroups — every staged slab feeding four row tiles, half the weight traffic again — measured 157 vs 169 us on
    // 9,415 rows 192 -> 96 with 576 bytes of spills per lane: the weight traffic is not what limits these launches; not kept)
    if (p.in_acc || p.bn_acc) {      // (opt-in form: its own instantiations, at most eight waves)
        if (rt2 && nw == 8) hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 2, 8, true>), grid, dim3(512), lds, st, p);
        else if (rt2) hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 2, 4, true>), grid, dim3(256), lds, st, p);
        else if (nw == 8) hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 1, 8, true>), grid, dim3(512), lds, st, p);
        else hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 1, 4, true>), grid, dim3(256), lds, st, p);
        EP_LAUNCH_CHECK();
        return EPRECON_OK;
    }
    // 16-byte gathers on packed weights: the branch-free instantiations (EPRECON_CONV_SPLITK_FAST=0: the general form)
    if constexpr (VEC4) {
        if (p.splitk_pipe == 2 && !switch_off("EPRECON_CONV_SPLITK_FAST")) {      // (read per launch: tests flip it)
            const bool aff = p.in_scale != nullptr;
#define EP_SPLITK_FAST_LAUNCH(RTv, NWv)                                                                                              \
    do {                                                                                                                             \
        if (aff) hipLaunchKernelGGL((spconv_splitk_kernel<true, RTv, NWv, false, true, true>), grid, dim3(64 * NWv), lds, st, p);    \
        else hipLaunchKernelGGL((spconv_splitk_kernel<true, RTv, NWv, false, true, false>), grid, dim3(64 * NWv), lds, st, p);       \
    } while (0)
            if (rt2 && nw == 8) EP_SPLITK_FAST_LAUNCH(2, 8);
            else if (rt2) EP_SPLITK_FAST_LAUNCH(2, 4);
            else if (nw == 16) {
                static const hipError_t attr_a = hipFuncSetAttribute(reinterpret_cast<const void *>(&spconv_splitk_kernel<true, 1, 16, false, true, true>),
                                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
                static const hipError_t attr_b = hipFuncSetAttribute(reinterpret_cast<const void *>(&spconv_splitk_kernel<true, 1, 16, false, true, false>),
                                                                     hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
                EP_HIP_CHECK(attr_a);
                EP_HIP_CHECK(attr_b);
                EP_SPLITK_FAST_LAUNCH(1, 16);
            } else if (nw == 8) EP_SPLITK_FAST_LAUNCH(1, 8);
            else EP_SPLITK_FAST_LAUNCH(1, 4);
#undef EP_SPLITK_FAST_LAUNCH
            EP_LAUNCH_CHECK();
            return EPRECON_OK;
        }
    }
    if (rt2 && nw == 8)
        hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 2, 8>), grid, dim3(512), lds, st, p);
    else if (rt2)
        hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 2, 4>), grid, dim3(256), lds, st, p);
    else if (nw == 16) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&spconv_splitk_kernel<VEC4, 1, 16>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        EP_HIP_CHECK(attr);
        hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 1, 16>), grid, dim3(1024), lds, st, p);
    }
    else if (nw == 8)
        hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 1, 8>), grid, dim3(512), lds, st, p);
    else
        hipLaunchKernelGGL((spconv_splitk_kernel<VEC4, 1, 4>), grid, dim3(256), lds, st, p);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // namespace

namespace epconv {
// short list + long (offset, slab) chain + a caller that can take 32-row BatchNorm summary blocks
bool splitk_ok(const ConvParams &p)
{
    if (switch_off("EPRECON_CONV_SPLITK") || p.accumulate) return false;   // (per launch, like the other selection switches)
    if (p.bn_partial && !p.flex_partial) return false;
    const int nt_full = (p.Cout + 31) / 32;
    if (p.ln && nt_full > 1) return false;
    const int cin_pad = (p.Cin + 7) / 8 * 8;
    const int64_t wg128 = ceil_div(p.n_out, kRowsPerBlock) * nt_full;
    const int stages = p.K * ((p.Cin + 31) / 32);
    constexpr int max_wg = 256, narrow_wg = 256;   // 128-row blocks x column tiles up to which the list counts as short
    // narrow inputs on very short lists (SPVCNN's stride-2 / stride-4 levels: 200..1,500 rows): the chain of a 32-row wave
    // (27 offsets x C_in / 2 MFMAs per column tile), not the weights, is what takes the time
    if (cin_pad <= 64) return wg128 <= narrow_wg && stages >= 8;
    return wg128 <= max_wg && stages >= 8;
}

int launch_splitk(ConvParams &p, hipStream_t st) { return gather_vec4(p) ? launch_splitk_v<true>(p, st) : launch_splitk_v<false>(p, st); }

}  // namespace epconv
