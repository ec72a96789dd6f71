// Direct gather form of the 3x3x3 sparse convolution: the device helpers its kernels share (sparse_conv_direct_kernels.hpp,
// sparse_conv_direct_persist.hpp) — operand helpers, epilogue, map staging, the live-offset cursor — and the probe-build macros.
// (kRT and stage_chunks come from the selection header, which the host side shares.)
#pragma once
#include "sparse_conv_direct_select.hpp"

namespace epconv {
namespace {

// Timing ablations of the probe builds only (python -m eprecon_amd.build --variant X -DEP_DIRECT_ABL=N sparse_conv_direct.hip;
// 0 in the library): 2 every gather reads one of 16 L1-resident rows, 4 no gathers, 8 every weight load reads the first
// (offset, chunk) block, 16 no MFMAs (the operands are summed on the VALU instead, so the loads stay), 32 no weight loads.
// Wrong results by design.
#ifndef EP_DIRECT_ABL
#define EP_DIRECT_ABL 0
#endif

// ReLU of a gathered value without the canonicalising `v_max_f32 x, x, x` clang puts in front of every llvm.maxnum (it must
// quiet signalling NaNs): 8 extra VALU instructions per gathered quad next to its 8 MFMAs.  The instruction itself is written
// out: v_max_f32 returns the non-NaN operand, so ReLU(NaN) = 0 as with fmaxf.  Rounds 4-5 got the same instruction count from
// a translation-unit-wide -fno-honor-nans (and the compiler folds v_med3_f32(x, 0, inf) back into maxnum + canonicalise);
// this keeps every other floating-point operation of the file under the strict rules.
__device__ __forceinline__ float relu_nc(float x)
{
    float r;
    asm("v_max_f32 %0, 0, %1" : "=v"(r) : "v"(x));
    return r;
}
// ... chosen by a launch-uniform bit mask instead of a branch (all ones: ReLU, zero: x unchanged — bit for bit what the branch gives)
__device__ __forceinline__ float relu_sel(float x, unsigned mask)
{
    const unsigned r = __float_as_uint(relu_nc(x)), b = __float_as_uint(x);
    return __uint_as_float((r & mask) | (b & ~mask));
}

// ---- opt-in bf16x3 operands (EPRECON_CONV_BF16X3=1; DESIGN.md 3b, SURVEY.md section 7 "with an error budget") ---------------
// x = hi + lo + e with hi = the top 16 bits of x (a bf16 by truncation), lo = bf16(x - hi) (round to nearest even; x - hi is exact)
// and |e| <= 2^-17 |x|.  A product a * w is taken as a_hi w_hi + a_hi w_lo + a_lo w_hi on the bf16 matrix pipe (fp32 accumulate):
// what is dropped is a_lo w_lo and the two e terms, <= ~2^-15 |a w| in all against fp32's 2^-24.  Both operands are split in
// registers from the SAME fp32 gathers and the same operand-order packing (wq16) the fp32 path loads: no second weight format.
// The 16-byte quad of a lane (four consecutive input channels, the k slot of v_mfma_f32_16x16x4_f32) is also the lane's four k
// values of v_mfma_f32_16x16x16_bf16, and two quads side by side are its eight of v_mfma_f32_16x16x32_bf16 — A and B agree on
// which channel sits in which k position, which is all a dot product over k needs.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct BfQuad { unsigned hi[2], lo[2]; };       // four values as two packed bf16 pairs each
__device__ __forceinline__ BfQuad bf_split(const float4 &v)
{
    const unsigned b0 = __float_as_uint(v.x), b1 = __float_as_uint(v.y), b2 = __float_as_uint(v.z), b3 = __float_as_uint(v.w);
    BfQuad r;
    r.hi[0] = __builtin_amdgcn_perm(b1, b0, 0x07060302u);       // (upper halves of two registers side by side)
    r.hi[1] = __builtin_amdgcn_perm(b3, b2, 0x07060302u);
    const f32x2 r01 = {v.x - __uint_as_float(b0 & 0xffff0000u), v.y - __uint_as_float(b1 & 0xffff0000u)};
    const f32x2 r23 = {v.z - __uint_as_float(b2 & 0xffff0000u), v.w - __uint_as_float(b3 & 0xffff0000u)};
    r.lo[0] = __builtin_bit_cast(unsigned, __builtin_convertvector(r01, bf16x2));      // v_cvt_pk_bf16_f32
    r.lo[1] = __builtin_bit_cast(unsigned, __builtin_convertvector(r23, bf16x2));
    return r;
}
__device__ __forceinline__ f32x4 bf_mfma32(const unsigned (&a0)[2], const unsigned (&a1)[2], const unsigned (&b0)[2],
                                           const unsigned (&b1)[2], f32x4 acc)
{
    union { bf16x8 v; unsigned u[4]; } a, b;
    a.u[0] = a0[0]; a.u[1] = a0[1]; a.u[2] = a1[0]; a.u[3] = a1[1];
    b.u[0] = b0[0]; b.u[1] = b0[1]; b.u[2] = b1[0]; b.u[3] = b1[1];
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.v, b.v, acc, 0, 0, 0);
}
__device__ __forceinline__ f32x4 bf_mfma16(const unsigned (&a0)[2], const unsigned (&b0)[2], f32x4 acc)
{
    union { s16x4 v; unsigned u[2]; } a, b;
    a.u[0] = a0[0]; a.u[1] = a0[1];
    b.u[0] = b0[0]; b.u[1] = b0[1];
    return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a.v, b.v, acc, 0, 0, 0);
}

// Epilogue for the 16x16 accumulator layout (column l & 15, rows 4 (l >> 4) + reg): bias, ReLU, residual with its pending
// BatchNorm, row-wise LayerNorm (16-lane xor-shuffles), BatchNorm summaries of the 128-row block (fixed-order Chan merges: rows
// in the lane, lane groups, waves).
// PERWAVE (the persistent kernel, sparse_conv_direct_persist.hpp): row0 is the first of the WAVE's 32 rows and `block` its job
// index; the wave's own summary (count, mean, M2 of 32 rows) is the partial row — no workgroup merge, no barrier.
template <int CT, bool PERWAVE = false>
__device__ __forceinline__ void direct_epilogue(const ConvParams &p, f32x4 (&acc)[kRT][CT], int row0, float *sStat, int block = 0)
{
    constexpr int RT = kRT, NR = 4 * kRT;
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = PERWAVE ? 0 : tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    int orow[NR];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int row = row0 + wave * 16 * RT + 16 * rt + 4 * q + j;
            orow[4 * rt + j] = row < p.n_out ? row : -1;
        }
    float v[CT][NR];
    bool colok[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const int col = 16 * t + l16;
        colok[t] = col < p.Cout;
        const float b = (p.bias && colok[t]) ? p.bias[col] : 0.0f;
        const float rs = (p.res_scale && colok[t]) ? p.res_scale[col] : 1.0f;
        const float rb = (p.res_scale && colok[t]) ? p.res_shift[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float val = 0.0f;
            if (colok[t] && orow[r] >= 0) {
                val = acc[r >> 2][t][r & 3] + b;
                if (p.relu) val = fmaxf(val, 0.0f);
                if (p.res) {
                    float rv = p.res[(size_t)orow[r] * p.ld_res + col];
                    if (p.res_scale) {
                        rv = fmaf(rv, rs, rb);
                        if (p.res_relu) rv = fmaxf(rv, 0.0f);
                    }
                    val += rv;
                }
            }
            v[t][r] = val;
        }
    }
    if (p.ln) {  // (uniform) row-wise LayerNorm over the C_out columns: 16 lanes x CT tiles hold a row
        const float inv_c = 1.0f / (float)p.Cout;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            float sum = 0.0f;
#pragma unroll
            for (int t = 0; t < CT; ++t) sum += v[t][r];
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) sum += __shfl_xor(sum, m);
            const float mean = sum * inv_c;
            float sq = 0.0f;
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const float d = colok[t] ? v[t][r] - mean : 0.0f;
                v[t][r] = d;
                sq = fmaf(d, d, sq);
            }
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) sq += __shfl_xor(sq, m);
            const float inv = 1.0f / sqrtf(sq * inv_c + p.ln_eps);
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int col = 16 * t + l16;
                float y = fmaf(v[t][r] * inv, (p.ln_gamma && colok[t]) ? p.ln_gamma[col] : 1.0f, (p.ln_beta && colok[t]) ? p.ln_beta[col] : 0.0f);
                if (p.ln_post_relu) y = fmaxf(y, 0.0f);
                v[t][r] = y;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (colok[t] && orow[r] >= 0) p.out[(size_t)orow[r] * p.ld_out + 16 * t + l16] = v[t][r];
    if (p.bn_partial || p.bn_acc) {  // (uniform) (count, mean, M2) of the stored values per column: rows in the lane, lane groups, waves
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            float n = 0.0f, sum = 0.0f;
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (orow[r] >= 0) { n += 1.0f; sum += v[t][r]; }
            float mean = n > 0.0f ? sum / n : 0.0f, m2 = 0.0f;
#pragma unroll
            for (int r = 0; r < NR; ++r)
                if (orow[r] >= 0) { const float d = v[t][r] - mean; m2 = fmaf(d, d, m2); }
#pragma unroll
            for (int m = 16; m < 64; m <<= 1) {  // lane groups q in order: the lower group is the left operand
                const float on = __shfl_xor(n, m), om = __shfl_xor(mean, m), oq = __shfl_xor(m2, m);
                const bool lower = (lane & m) == 0;
                float a_n = lower ? n : on, a_mean = lower ? mean : om, a_m2 = lower ? m2 : oq;
                chan_merge(a_n, a_mean, a_m2, lower ? on : n, lower ? om : mean, lower ? oq : m2);
                n = a_n; mean = a_mean; m2 = a_m2;
            }
            if constexpr (PERWAVE) {
                if (q == 0 && colok[t]) {
                    if (p.bn_partial) bn_partial_store(p, block, 16 * t + l16, n, mean, m2);
                    if (p.bn_acc) bn_acc_publish(p, 16 * t + l16, block, block == 0, n, mean, m2);
                }
                continue;
            }
            if (q == 0) {
                float *d = sStat + (wave * 3) * 16 * CT + 16 * t + l16;
                d[0] = n; d[16 * CT] = mean; d[2 * 16 * CT] = m2;
            }
        }
        if constexpr (PERWAVE) return;
        __syncthreads();
        if (tid < 16 * CT && tid < p.Cout) {
            float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
                chan_merge(a_n, a_mean, a_m2, sStat[(w * 3) * 16 * CT + tid], sStat[(w * 3 + 1) * 16 * CT + tid], sStat[(w * 3 + 2) * 16 * CT + tid]);
            if (p.bn_partial) bn_partial_store(p, (int)blockIdx.x, tid, a_n, a_mean, a_m2);
            if (p.bn_acc) bn_acc_publish(p, tid, (int)blockIdx.x, blockIdx.x == 0, a_n, a_mean, a_m2);
        }
    }
}

// C_out = 16 m + 8 (8, 24, 40, 56: the ConvGRU / SPVCNN channel plans at the finest level): the last 8 columns run on
// v_mfma_f32_4x4x1_16B_f32 instead of a half-empty 16-column tile.  That instruction multiplies 16 independent 4x1 by 1x4
// blocks (lane 4 b + i holds A_b[i] / B_b[i], register r of lane 4 b + j holds D_b[r][j]); fed with the SAME A register as the
// 16x16x4 MFMA (lane = row l & 15, k slot g = l >> 4), block b = 4 g + (row >> 2) is rows 4 (row >> 2) .. + 3 at the ONE input
// channel of k slot g, so with B_b[j] = W[channel of slot g][column 16 m + 4 cg + j] one instruction adds a k slot's product
// into a per-slot partial of 16 rows x 4 columns: 512 flops in 8 cycles, the fp32 rate of every MFMA shape.  Two of them (cg =
// 0, 1: 16 cycles) replace one 16x16x4 (32 cycles) per gathered register; the four k-slot partials are summed once, here, in
// fixed order, and handed to the shared epilogue in the 16x16 accumulator layout (column l & 15, rows 4 (l >> 4) + reg;
// columns 8 .. 15 zero: the epilogue masks them by C_out anyway).
__device__ __forceinline__ void tail_to_tile(const f32x4 (&acct)[kRT][2], f32x4 (&dst)[kRT], int lane)
{
    const int l16 = lane & 15, q = lane >> 4;
    const int src = 4 * q + (l16 & 3);      // k slot 0's lane of (rows 4 q .. 4 q + 3, column l16 & 3): after the sums every slot holds the total
#pragma unroll
    for (int rt = 0; rt < kRT; ++rt)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v0 = acct[rt][0][j], v1 = acct[rt][1][j];
            v0 += __shfl_xor(v0, 16); v1 += __shfl_xor(v1, 16);
            v0 += __shfl_xor(v0, 32); v1 += __shfl_xor(v1, 32);
            const float t0 = __shfl(v0, src), t1 = __shfl(v1, src);
            dst[rt][j] = l16 < 4 ? t0 : (l16 < 8 ? t1 : 0.0f);
        }
}

// The workgroup's slice of the kernel map -> LDS ([K][128 rows]), and for every wave the offsets at which at least one of its
// 32 rows has a neighbour, as a bit mask (wave-uniform: it lives in scalar registers, and the walk below — lowest set bit,
// clear it — is scalar arithmetic).  All loads of a thread are issued before the first is used (K <= 27: at most 14 per
// thread).  Load pass `it` of wave w covers offset 2 it + w / 2, rows 64 (w % 2) .. + 63: the two halves of its ballot are
// the flags of consumer waves 2 (w % 2) and 2 (w % 2) + 1, left in sFlag[offset][consumer wave].  Ends with the barrier that
// publishes the table (and whatever the caller staged before the call).
constexpr int kMapLoads = 14;
__device__ __forceinline__ unsigned stage_map(const ConvParams &p, int row0, int *sNbr, int *sFlag, int tid)
{
    static_assert(kDirectRows == 128 && kRT == 2 && kWaves == 4, "the pass -> (offset, row half) arithmetic below");
    const int total = p.K * kDirectRows;
    const int lane = tid & 63, wave = tid >> 6;
    int jv[kMapLoads];
#pragma unroll
    for (int it = 0; it < kMapLoads; ++it) {
        const int e = tid + it * 256;
        const int k = e >> 7, row = row0 + (e & 127);
        int j = -1;
        if (e < total && row < p.n_out) j = p.nbr ? p.nbr[(size_t)k * p.n_out + row] : row;
        jv[it] = j;
    }
#pragma unroll
    for (int it = 0; it < kMapLoads; ++it) {
        const int e = tid + it * 256;
        if (e < total) sNbr[e] = jv[it];
        const unsigned long long b = __ballot(jv[it] >= 0);
        const int k = 2 * it + (wave >> 1);
        if (lane < 2 && k < p.K) sFlag[k * kWaves + 2 * (wave & 1) + lane] = (lane ? (unsigned)(b >> 32) : (unsigned)b) != 0u;
    }
    __syncthreads();
    const bool mine = lane < p.K && sFlag[lane * kWaves + wave] != 0;
    return (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)__ballot(mine));
}

// Position in the (live offset, part) sequence of a wave: `k` the current offset, `rest` the live offsets after it.
// next() stays on the last position once the sequence is exhausted (a stage fetched past the end is not consumed).
struct LiveCursor {
    unsigned rest;
    int k, part;
    __device__ __forceinline__ explicit LiveCursor(unsigned mask) : rest(mask & (mask - 1u)), k(__builtin_ctz(mask)), part(0) {}
    __device__ __forceinline__ void next(int parts)
    {
        if (part + 1 < parts) ++part;
        else if (rest) { k = __builtin_ctz(rest); rest &= rest - 1u; part = 0; }
    }
};

// EPRECON_CONV_INTERLEAVE=0: the fenced schedule for every launch (read per launch; see the main loop of the template kernel)
#ifndef EP_MIX_EXTRA       // (probe builds: matrix instructions per load group beyond ceil(MFMAs / loads) of a stage)
#define EP_MIX_EXTRA 1
#endif

}  // namespace
}  // namespace epconv
