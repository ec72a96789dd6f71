// Sparse 3D convolution for gfx950 as an output-stationary gather-GEMM on the fp32 matrix cores.
//
// Replaces (reference call sites; the CUDA kernels themselves live in the un-vendored torchsparse /
// spconv extensions, so the semantics below are this build's restatement — SURVEY.md appendix A):
//   spnn.Conv3d k=3 s=1, k=2 s=2, k=2 s=2 transposed, k=1     models/modules.py:19-64,90-122,181
//   spconv.SubMConv3d k=1 / k=3 (+bias)                         models/modules.py:252,444
//
//   out[i, :] = bias + sum_k  x[nbr[k][i], :] @ W[k]          (rows with nbr == -1 contribute 0)
//
// nbr is the kernel map int32[K][n_out] built once per coordinate set by kernel_map.hip and shared
// by every layer on that set (stride-1 k=3: K = 27, out coords = in coords; k2s2 down: K = 8 children
// of each coarse voxel; transposed: K = 8 with one live entry per fine voxel; k=1: identity map).
// There is no scatter-add and no atomic: every output row is produced by exactly one wave, so the
// result is deterministic.
//
// Mapping to CDNA4: a wave owns 32 output rows x (32*NT) output channels in NT accumulators of
// v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma chain).  A operand: each lane holds 4 consecutive
// input channels of its row, one VGPR per MFMA step.  B operand: weights from LDS.  Four kernels share
// the prologue / epilogue fusions and differ in how the operands reach the wave:
//   spconv_resident_kernel   C_in <= 64: the weights of a group of offsets resident per barrier, the
//                            neighbour tile in LDS, rows gathered from global memory in software-pipelined
//                            batches (a fixed number of loads in flight -> vmcnt(N) waits);
//   spconv_mfma_kernel       wide layers: 32-channel weight slabs double-buffered in LDS, one barrier per slab;
//   spconv_splitk_kernel     short lists with wide inputs: 32-row workgroups whose four waves split the
//                            (offset, slab) chain, wave-private slabs, fixed-order sum of the partials;
//   conv2d_tile_kernel       dense 2D 3x3 layers with C_in <= 40: halo tile + all nine weight matrices in
//                            LDS, no kernel map, no global access in the MFMA loop.
// Prologue: the producer's pending BatchNorm (+ReLU) applied while loading (in_scale / in_shift).
// Epilogues (conv_epilogue): bias, ReLU, residual (with its own pending BatchNorm), per-workgroup
// BatchNorm summaries (count, mean, M2) of the stored values, or a row-wise LayerNorm over C_out.
// Roofline: fp32 MFMA (157 TFLOP/s) for wide layers on long lists (measured 41 % on 32->32, K = 27);
// narrow or short layers are bound by their dependent chain (staging round trips), see DESIGN.md 3b.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.hpp"
#include "conv_common.hpp"

namespace {
using namespace ep;
using namespace epconv;

typedef float f32x16 __attribute__((ext_vector_type(16)));


// Stage `rows` x TN weights (zero padded) from w[row0 + r][0:ncols] (row stride `stride`, rows valid
// while row0 + r < row_end) into LDS.  Branch-free: addresses are clamped into the valid range and
// the value is selected afterwards, so the compiler can keep many loads in flight (a guarded load
// per element compiled to load / s_waitcnt vmcnt(0) pairs: ~500 cycles each).
template <int TN>
__device__ __forceinline__ void stage_weights(float *dst, const float *w, int row0, int row_end, int stride,
                                              int ncols, int rows, int tid)
{
    // w points at column col0 of row 0; `stride` floats per row, `ncols` valid columns from there
    const int total = rows * TN;
    if (stride == TN && ncols >= TN && (reinterpret_cast<uintptr_t>(w) & 15) == 0) {
        // padded layout == source layout: straight 16-byte copies
        const float4 *src = reinterpret_cast<const float4 *>(w + (size_t)row0 * stride);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        const int valid4 = max(0, min(rows, row_end - row0)) * (TN / 4);
#pragma unroll 4
        for (int e = tid; e < total / 4; e += 256) d4[e] = e < valid4 ? src[min(e, max(valid4 - 1, 0))] : make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    if ((stride & 3) == 0 && (ncols & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == 0) {
        // 16-byte loads along the rows whenever the row pitch allows it (C_out = 12, 20, 24, 40, ...: the
        // element-wise path below took ~7 dependent round trips per staged group)
        constexpr int Q = TN / 4;
        const int nq = min(ncols, TN) / 4;  // valid 16-byte groups per row
        float4 *d4 = reinterpret_cast<float4 *>(dst);
#pragma unroll 4
        for (int e = tid; e < rows * Q; e += 256) {
            const int r = e / Q, q = e - r * Q;
            const bool ok = (row0 + r < row_end) && (q < nq);
            const float4 v = *reinterpret_cast<const float4 *>(w + (size_t)min(row0 + r, row_end - 1) * stride + 4 * min(q, nq - 1));
            d4[e] = ok ? v : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
#pragma unroll 4
    for (int e = tid; e < total; e += 256) {
        const int r = e / TN, col = e - r * TN;
        const bool ok = (row0 + r < row_end) && (col < ncols);
        const int rr = min(row0 + r, row_end - 1), cc = min(col, ncols - 1);
        const float v = w[(size_t)rr * stride + cc];
        dst[e] = ok ? v : 0.0f;
    }
}

constexpr int kRowsPerWave = 32;
constexpr int kRowsPerBlock = kRowsPerWave * kWaves;
constexpr int kSlabC = 32;  // input channels per staged weight slab

// Shared epilogue.  C/D layout of v_mfma_f32_32x32x2_f32: col = lane & 31,
// row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
//   v = acc + bias; [v += out]; [v = max(v, 0)]; [v += res]; out = v
// and, when p.bn_partial is set, the (count, mean, M2) summary of the stored values of this
// workgroup's rows per column (lane-local two-pass over its 16 rows, then fixed-order Chan merges:
// lane halves, then the four waves through LDS) -> bn_partial[blockIdx.x][3][Cout]: the
// statistics pass of the train-mode BatchNorm that follows every convolution of the reference,
// without re-reading the tensor.  sStat: >= kWaves * 3 * 32 * NT floats of LDS, free to overwrite.
// Epilogue with the row-wise LayerNorm the reference wires behind its spconv layers
// (models/modules.py:447-452,473-482, models/occupancy_initialization.py:141-169) fused in:
//   v = acc + bias; [relu]; [+ residual];  y = LN_row(v) * gamma + beta; [relu]
// A row's Cout values sit in the 32 lanes of one half-wave (column = lane & 31, NT tiles per lane), so
// the two row reductions are five xor-shuffles each; 16 rows per lane are reduced independently.
// Row mappers: global output row of the wave's i-th tile row (0..31), or -1 if there is none.
struct LinearRows {  // 32 consecutive rows
    int base, n;
    __device__ __forceinline__ int operator()(int i) const { return base + i < n ? base + i : -1; }
};
struct ImageRows {  // 2 image rows x 16 pixels of one map (conv2d_tile_kernel)
    int row00, y0, x0, H, W;  // row of pixel (y0, x0); tile origin may lie past the image edge
    __device__ __forceinline__ int operator()(int i) const
    {
        const int y = y0 + (i >> 4), x = x0 + (i & 15);
        return (y < H && x < W) ? row00 + (i >> 4) * W + (i & 15) : -1;
    }
};

template <int NT, class RowMap>
__device__ __forceinline__ void conv_epilogue_ln(const ConvParams &p, f32x16 (&acc)[NT], RowMap rm, int r32, int half)
{
    float gam[NT], bet[NT];
    bool colok[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = t * 32 + r32;
        colok[t] = col < p.Cout;
        const float b = (p.bias && colok[t]) ? p.bias[col] : 0.0f;
        const float rs = (p.res_scale && colok[t]) ? p.res_scale[col] : 1.0f;
        const float rb = (p.res_scale && colok[t]) ? p.res_shift[col] : 0.0f;
        gam[t] = (p.ln_gamma && colok[t]) ? p.ln_gamma[col] : 1.0f;
        bet[t] = (p.ln_beta && colok[t]) ? p.ln_beta[col] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rm((r & 3) + 8 * (r >> 2) + 4 * half);
            float v = 0.0f;
            if (colok[t] && row >= 0) {
                v = acc[t][r] + b;
                if (p.relu) v = fmaxf(v, 0.0f);
                if (p.res) {
                    float rv = p.res[(size_t)row * p.ld_res + col];
                    if (p.res_scale) {
                        rv = fmaf(rv, rs, rb);
                        if (p.res_relu) rv = fmaxf(rv, 0.0f);
                    }
                    v += rv;
                }
            }
            acc[t][r] = v;
        }
    }
    const float inv_c = 1.0f / (float)p.Cout;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t) s += acc[t][r];
#pragma unroll
        for (int m = 16; m > 0; m >>= 1) s += __shfl_xor(s, m);
        const float mean = s * inv_c;
        float q = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const float d = colok[t] ? acc[t][r] - mean : 0.0f;
            acc[t][r] = d;
            q = fmaf(d, d, q);
        }
#pragma unroll
        for (int m = 16; m > 0; m >>= 1) q += __shfl_xor(q, m);
        const float inv = 1.0f / sqrtf(q * inv_c + p.ln_eps);
        const int row = rm((r & 3) + 8 * (r >> 2) + 4 * half);
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float y = fmaf(acc[t][r] * inv, gam[t], bet[t]);
            if (p.ln_post_relu) y = fmaxf(y, 0.0f);
            if (colok[t] && row >= 0) p.out[(size_t)row * p.ld_out + t * 32 + r32] = y;
        }
    }
}

// ACC = false compiles the accumulator-block form of the summaries out (the 1,024-thread split-K instantiation sits at its
// register cap: the extra kernel arguments alone pushed it into scratch; its launcher steps down to eight waves instead)
template <int NT, bool ACC = true, class RowMap>
__device__ __forceinline__ void conv_epilogue(const ConvParams &p, f32x16 (&acc)[NT], RowMap rm, int col0, int r32,
                                              int half, int wave, float *sStat, int partial_row, int ncb)
{
    constexpr int TN = 32 * NT;
    if (p.ln) {  // uniform; the launcher guarantees a single column block and no BatchNorm summaries
        conv_epilogue_ln<NT>(p, acc, rm, r32, half);
        return;
    }
    const bool stats = p.bn_partial != nullptr || (ACC && p.bn_acc != nullptr);
    if (stats) __syncthreads();  // every wave is done reading the weights that sStat overlays
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = col0 + t * 32 + r32;
        const bool colok = col < p.Cout;
        const float b = (p.bias && colok) ? p.bias[col] : 0.0f;
        const float rs = (p.res_scale && colok) ? p.res_scale[col] : 1.0f;
        const float rb = (p.res_scale && colok) ? p.res_shift[col] : 0.0f;
        float vals[16];
        float cnt = 0.0f, sum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = rm((r & 3) + 8 * (r >> 2) + 4 * half);
            float v = 0.0f;
            if (colok && row >= 0) {
                float *o = p.out + (size_t)row * p.ld_out + col;
                v = acc[t][r] + b;
                if (p.accumulate) v += *o;
                if (p.relu) v = fmaxf(v, 0.0f);
                if (p.res) {
                    float rv = p.res[(size_t)row * p.ld_res + col];
                    if (p.res_scale) {
                        rv = fmaf(rv, rs, rb);
                        if (p.res_relu) rv = fmaxf(rv, 0.0f);
                    }
                    v += rv;
                }
                *o = v;
                cnt += 1.0f;
            }
            vals[r] = v;
            sum += v;
        }
        if (stats) {
            float mean = cnt > 0.0f ? sum / cnt : 0.0f;
            float m2 = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rm((r & 3) + 8 * (r >> 2) + 4 * half);
                if (row >= 0) {
                    const float d = vals[r] - mean;
                    m2 = fmaf(d, d, m2);
                }
            }
            // halves: lanes l and l ^ 32 hold the two row sets of one column; merge as (half 0, half 1)
            const float on = __shfl_xor(cnt, 32), omean = __shfl_xor(mean, 32), om2 = __shfl_xor(m2, 32);
            float a_n = half ? on : cnt, a_mean = half ? omean : mean, a_m2 = half ? om2 : m2;
            chan_merge(a_n, a_mean, a_m2, half ? cnt : on, half ? mean : omean, half ? m2 : om2);
            if (half == 0) {
                float *d = sStat + (wave * 3) * TN + t * 32 + r32;
                d[0] = a_n; d[TN] = a_mean; d[2 * TN] = a_m2;
            }
        }
    }
    if (stats) {
        __syncthreads();
        const int tid = threadIdx.x;
        if (tid < TN && col0 + tid < p.Cout) {
            float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w)
                chan_merge(a_n, a_mean, a_m2, sStat[(w * 3) * TN + tid], sStat[(w * 3 + 1) * TN + tid],
                           sStat[(w * 3 + 2) * TN + tid]);
            if (!ACC || p.bn_partial) bn_partial_store(p, partial_row, col0 + tid, a_n, a_mean, a_m2);
            if (ACC && p.bn_acc) bn_acc_publish(p, col0 + tid, partial_row, partial_row == 0, a_n, a_mean, a_m2);
        }
    }
}

template <int NT, bool VEC4>
__global__ __launch_bounds__(256) void spconv_mfma_kernel(ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TN = 32 * NT;
    float *sW = reinterpret_cast<float *>(smem);                     // [2][kSlabC][TN]
    int *sNbr = reinterpret_cast<int *>(sW + 2 * kSlabC * TN);       // [K][128]
    int *sActive = sNbr + p.K * kRowsPerBlock;                       // [K] live-row flags
    const int cinA = (p.Cin + 3) & ~3;
    float *sAff = reinterpret_cast<float *>(sActive + ((p.K + 3) & ~3));  // [2][cinA] input scale / shift

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int row0 = blockIdx.x * kRowsPerBlock;
    const int col0 = blockIdx.y * TN;  // short lists: the output columns are split over blockIdx.y

    // neighbour tile + live-offset flags
    for (int k = tid; k < p.K; k += 256) sActive[k] = 0;
    stage_in_affine<256>(p, sAff, cinA, tid);
    __syncthreads();
    for (int e = tid; e < p.K * kRowsPerBlock; e += 256) {
        const int k = e / kRowsPerBlock, r = e - k * kRowsPerBlock;
        const int row = row0 + r;
        int j = -1;
        if (row < p.n_out) j = p.nbr ? p.nbr[(size_t)k * p.n_out + row] : row;
        sNbr[e] = j;
        if (j >= 0) sActive[k] = 1;  // benign race: every writer stores 1
    }
    __syncthreads();

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int nslab = (p.Cin + kSlabC - 1) / kSlabC;
    // stage counter over (live k, slab); the double buffer flips per staged slab
    int buf = 0;
    bool have_prev = false;
    for (int k = 0; k < p.K; ++k) {
        if (!sActive[k]) continue;  // block-uniform
        const int j = sNbr[k * kRowsPerBlock + wave * kRowsPerWave + r32];
        const float *xrow = p.x + (size_t)(j >= 0 ? j : 0) * p.ld_x;
        const float *wk = p.w + (size_t)k * p.Cin * p.Cout + col0;
        for (int sl = 0; sl < nslab; ++sl) {
            const int c0 = sl * kSlabC;
            // ---- stage W[k][c0 : c0+32][0 : TN] into sW[buf] (zero padded) ----
            float *dstW = sW + buf * kSlabC * TN;
            stage_weights<TN>(dstW, wk, c0, p.Cin, p.Cout, p.Cout - col0, kSlabC, tid);
            // ---- gather this lane's A values: 4 chunks of 8 channels, 4 floats each ----
            float a[4][4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const int c = c0 + ch * 8 + 4 * half;
                if (VEC4) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (j >= 0 && c < p.Cin) v = *reinterpret_cast<const float4 *>(xrow + c);
                    if (p.Cin & 3) {  // ragged channel count: whatever follows the row's last channel is not input
                        if (c + 1 >= p.Cin) v.y = 0.0f;
                        if (c + 2 >= p.Cin) v.z = 0.0f;
                        if (c + 3 >= p.Cin) v.w = 0.0f;
                    }
                    a[ch][0] = v.x; a[ch][1] = v.y; a[ch][2] = v.z; a[ch][3] = v.w;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) a[ch][s] = (j >= 0 && c + s < p.Cin) ? xrow[c + s] : 0.0f;
                }
            }
            __syncthreads();  // sW[buf] complete; the other buffer is free again after this barrier
            (void)have_prev;
            const float *srcW = sW + buf * kSlabC * TN;
            const int nch = min(4, (p.Cin - c0 + 7) / 8);
            if (p.in_scale) {
                // BatchNorm (+ReLU) of the producer applied to the gathered values; padding stays 0
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int c = c0 + ch * 8 + 4 * half;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const bool ok = j >= 0 && c + s < p.Cin;
                        float v = fmaf(a[ch][s], sAff[min(c + s, cinA - 1)], sAff[cinA + min(c + s, cinA - 1)]);
                        if (p.in_relu) v = fmaxf(v, 0.0f);
                        a[ch][s] = ok ? v : 0.0f;
                    }
                }
            }
            for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float *brow = srcW + (ch * 8 + 4 * half + s) * TN + r32;
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch][s], brow[t * 32], acc[t], 0, 0, 0);
                }
            }
            buf ^= 1;
            have_prev = true;
        }
    }

    conv_epilogue<NT>(p, acc, LinearRows{row0 + wave * kRowsPerWave, p.n_out}, col0, r32, half, wave, sW, (int)blockIdx.x, (int)gridDim.y);
}


// ---------------------------------------------------------------------------------------------
// Group-resident variant for narrow layers (Cin <= 64): the weights of a GROUP of kernel offsets
// (up to ~24 KB, e.g. 9 offsets of a 32x32 layer) are staged per barrier instead of one 32-channel
// slab, so a 27-offset layer needs 3 barriers instead of 27, and four workgroups fit a CU.
// The gathers are issued in BATCHES of KB offsets (KB * NCH 16-byte loads per lane in flight)
// before the first MFMA of the batch: the per-offset loop with one offset of prefetch paid one
// memory latency (~1.5 us) per offset - 27 us of the 30 us a 20->20 3x3 layer took on 43,200 pixels,
// 40 of the 76 us of a 27-offset 32->32 layer.  Offsets with no live row in a wave's 32 rows are skipped.
// ---------------------------------------------------------------------------------------------
struct ARows {
    float v[8][4];  // up to 8 chunks of 8 input channels; this lane's 4 consecutive channels per chunk
};

template <bool VEC4, int NCH>
__device__ __forceinline__ void gather_rows(const ConvParams &p, int j, int half, ARows &a, int cbase = 0)
{
    const float *xrow = p.x + (size_t)(j >= 0 ? j : 0) * p.ld_x;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const int c = cbase + ch * 8 + 4 * half;
        if (VEC4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j >= 0 && c < p.Cin) v = *reinterpret_cast<const float4 *>(xrow + c);
            if (p.Cin & 3) {
                if (c + 1 >= p.Cin) v.y = 0.0f;
                if (c + 2 >= p.Cin) v.z = 0.0f;
                if (c + 3 >= p.Cin) v.w = 0.0f;
            }
            a.v[ch][0] = v.x; a.v[ch][1] = v.y; a.v[ch][2] = v.z; a.v[ch][3] = v.w;
        } else {
#pragma unroll
            for (int s = 0; s < 4; ++s) a.v[ch][s] = (j >= 0 && c + s < p.Cin) ? xrow[c + s] : 0.0f;
        }
    }
}

// pipelined form: unconditional loads from clamped addresses (a fixed number of loads in flight lets the
// compiler wait with vmcnt(N) for the older batch only); the made-up values are zeroed by fix_rows at use
// (the row pitch covers the channel count rounded up to 4 — the launcher checks it — so the last 16-byte group
// of a ragged row may be loaded; fix_rows zeroes what lies past Cin)
template <int NCH>
__device__ __forceinline__ void gather_rows_nb(const ConvParams &p, int j, int half, ARows &a, int cbase = 0)
{
    const float *xrow = p.x + (size_t)max(j, 0) * p.ld_x;
    const int last = ((p.Cin + 3) & ~3) - 4;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const float4 v = *reinterpret_cast<const float4 *>(xrow + min(cbase + ch * 8 + 4 * half, last));
        a.v[ch][0] = v.x; a.v[ch][1] = v.y; a.v[ch][2] = v.z; a.v[ch][3] = v.w;
    }
}
template <int NCH>
__device__ __forceinline__ void fix_rows(const ConvParams &p, int j, int half, ARows &a, int cbase = 0)
{
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (!(j >= 0 && cbase + ch * 8 + 4 * half + s < p.Cin)) a.v[ch][s] = 0.0f;
}

// Gather through a buffer resource over x: the byte offset of a row is ONE 24-bit multiply, the chunk offsets are
// instruction immediates and the slab offset is the scalar offset, and a missing neighbour (j < 0) is sent past the end
// of the buffer, where the hardware returns zeros — no 64-bit address arithmetic and no per-value select afterwards.
// (PMC, 27-offset 32 -> 32 layer: 11 VALU instructions per MFMA with pointer gathers + fix_rows.)
template <int NCH>
__device__ __forceinline__ void gather_rows_buf(__amdgpu_buffer_rsrc_t rsrc, unsigned row_bytes, unsigned oob, int j, int half,
                                                ARows &a, int cbase_bytes)
{
    const unsigned off = (j >= 0 ? __umul24((unsigned)j, row_bytes) : oob) + 16u * half;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
        const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + 32u * ch, cbase_bytes, 0);
        a.v[ch][0] = __uint_as_float(v.x); a.v[ch][1] = __uint_as_float(v.y);
        a.v[ch][2] = __uint_as_float(v.z); a.v[ch][3] = __uint_as_float(v.w);
    }
}

// Weights of `kn` offsets for the resident kernel, laid out for 16-byte B-operand reads: a lane (half, column) uses the
// four consecutive input channels ch*8 + 4*half + {0..3} of its column for four consecutive MFMAs, so they sit together:
//   sW[((((kk * NCH + ch) * 2 + half) * NT + t) * 32 + col) * 4 + s]  =  W[k0 + kk][cbase + ch*8 + 4*half + s][col0 + 32 t + col]
// (zero where the channel or the column does not exist).  One ds_read_b128 per (chunk, column block) instead of four
// ds_read_b32; branch-free clamped global loads, 16 bytes along the columns when the pitch allows it.
template <int NT, int NCH>
__device__ __forceinline__ void stage_weights_quads(float *dst, const ConvParams &p, int k0, int kn, int cbase, int col0, int tid)
{
    constexpr int TN = 32 * NT, cin_pad = NCH * 8;
    const int ncols = p.Cout - col0;
    const bool v4 = (p.Cout & 3) == 0 && (col0 & 3) == 0 && (reinterpret_cast<uintptr_t>(p.w) & 15) == 0;
    if (v4) {
        constexpr int Q = TN / 4;
        for (int e = tid; e < kn * cin_pad * Q; e += 256) {
            const int q = e % Q, rc = e / Q;
            const int c = rc % cin_pad, kk = rc / cin_pad;
            const bool ok = (cbase + c < p.Cin) && (4 * q < ncols);
            const size_t row = (size_t)(k0 + kk) * p.Cin + min(cbase + c, p.Cin - 1);
            const float4 v = *reinterpret_cast<const float4 *>(p.w + row * p.Cout + col0 + min(4 * q, max(ncols - 4, 0)));
            const int ch = c >> 3, half = (c >> 2) & 1, sidx = c & 3;
            const int t = (4 * q) >> 5, col = (4 * q) & 31;
            float *d = dst + ((((size_t)(kk * NCH + ch) * 2 + half) * NT + t) * 32 + col) * 4 + sidx;
            d[0] = ok ? v.x : 0.0f; d[4] = ok ? v.y : 0.0f; d[8] = ok ? v.z : 0.0f; d[12] = ok ? v.w : 0.0f;
        }
        return;
    }
    for (int e = tid; e < kn * cin_pad * TN; e += 256) {
        const int cg = e % TN, rc = e / TN;
        const int c = rc % cin_pad, kk = rc / cin_pad;
        const bool ok = (cbase + c < p.Cin) && (cg < ncols);
        const size_t row = (size_t)(k0 + kk) * p.Cin + min(cbase + c, p.Cin - 1);
        const float v = p.w[row * p.Cout + col0 + min(cg, max(ncols - 1, 0))];
        const int ch = c >> 3, half = (c >> 2) & 1, sidx = c & 3;
        dst[((((size_t)(kk * NCH + ch) * 2 + half) * NT + (cg >> 5)) * 32 + (cg & 31)) * 4 + sidx] = ok ? v : 0.0f;
    }
}

// gather batch size: KB * NCH <= 16 float4 per lane in flight (<= 64 VGPRs of A operands)
constexpr int resident_kb(int nch) { return nch <= 1 ? 9 : nch == 2 ? 8 : nch == 3 ? 5 : nch == 4 ? 4 : nch == 5 ? 3 : 2; }

template <int NT, bool VEC4, int NCH, bool PIPE>
__global__ __launch_bounds__(256) void spconv_resident_kernel(ConvParams p, int kgroup, int nslab)
{
    // nslab > 1: wide inputs.  The input channels are walked in `nslab` slabs of cin_pad = 8 * NCH channels; per
    // slab the kernel is the narrow-layer kernel (offset groups resident in LDS, software-pipelined gathers), the
    // accumulators carry over.  One flat sequence of (slab, offset batch) steps, so the gather pipeline never drains.
    constexpr int cin_pad = NCH * 8;
    constexpr int KB = PIPE ? (resident_kb(NCH) + 1) / 2 : resident_kb(NCH);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TN = 32 * NT;
    float *sW = reinterpret_cast<float *>(smem);  // [kgroup][cin_pad][TN], zero padded; kgroup % KB == 0
    constexpr int per_k = cin_pad * TN;
    int *sNbr = reinterpret_cast<int *>(sW + kgroup * per_k);  // [K][128] neighbour tile
    const int cin_all = nslab * cin_pad;
    float *sAff = reinterpret_cast<float *>(sNbr + p.K * kRowsPerBlock);  // [2][cin_all] input scale / shift
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int wrow0 = blockIdx.x * kRowsPerBlock + wave * kRowsPerWave;
    const int col0 = blockIdx.y * TN;
    const float *wbase = p.w + col0;
    stage_in_affine<256>(p, sAff, cin_all, tid);
    // the neighbour indices of the whole tile go to LDS up front: a gather then depends on ONE
    // memory latency (the rows), not two (index, then rows)
    for (int e = tid; e < p.K * kRowsPerBlock; e += 256) {
        const int k = e / kRowsPerBlock, r = e - k * kRowsPerBlock;
        const int row = blockIdx.x * kRowsPerBlock + r;
        sNbr[e] = row < p.n_out ? (p.nbr ? p.nbr[(size_t)k * p.n_out + row] : row) : -1;
    }
    __syncthreads();

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int nb = (p.K + KB - 1) / KB;  // offset batches per slab
    const int total = nb * nslab;
    const int *nbr_row = sNbr + wave * kRowsPerWave + r32;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, PIPE ? (int)p.x_bytes : 0, 0x00020000);
    const unsigned row_bytes = (unsigned)p.ld_x * 4u, oob = (unsigned)p.x_bytes;
    auto issue = [&](int b, ARows(&a)[KB], int(&jj)[KB]) {
        const int sl = min(b / nb, nslab - 1);
        const int kb = (b - (b / nb) * nb) * KB;
        const bool in = b < total;
#pragma unroll
        for (int u = 0; u < KB; ++u) jj[u] = (in && kb + u < p.K) ? nbr_row[min(kb + u, p.K - 1) * kRowsPerBlock] : -1;
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            if (PIPE) gather_rows_buf<NCH>(rsrc, row_bytes, oob, jj[u], half, a[u], sl * cin_pad * 4);
            else gather_rows<VEC4, NCH>(p, jj[u], half, a[u], sl * cin_pad);
        }
    };
    auto consume = [&](int b, ARows(&a)[KB], int(&jj)[KB]) {
        const int sl = b / nb;
        const int kb = (b - sl * nb) * KB;
        const int cbase = sl * cin_pad;
        if (PIPE && cbase + cin_pad > p.Cin) {  // ragged channel count: what the last chunk read past C_in is not data
#pragma unroll
            for (int u = 0; u < KB; ++u) fix_rows<NCH>(p, jj[u], half, a[u], cbase);
        }
        // ---- weights of the group this batch belongs to (loads above stay in flight) ----
        const int k0 = kb / kgroup * kgroup;
        if (kb == k0) {
            const int kn = min(kgroup, p.K - k0);
            __syncthreads();  // every wave is done with the previous group's weights
            stage_weights_quads<NT, NCH>(sW, p, k0, kn, cbase, col0, tid);
            __syncthreads();
        }
        // ---- MFMAs of the batch ----
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            if (kb + u >= p.K) break;
            const bool live = __ballot(jj[u] >= 0) != 0ull;
            if (!live) continue;
            const float *wk = sW + (kb + u - k0) * per_k + (half * NT * 32 + r32) * 4;
            if (p.in_scale) {
                // BatchNorm (+ReLU) of the producer applied to the gathered values; padding stays 0
                const bool ok = jj[u] >= 0;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const float4 sc = *reinterpret_cast<const float4 *>(sAff + cbase + ch * 8 + 4 * half);
                    const float4 sh = *reinterpret_cast<const float4 *>(sAff + cin_all + cbase + ch * 8 + 4 * half);
                    const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float v = fmaf(a[u].v[ch][s], scv[s], shv[s]);
                        if (p.in_relu) v = fmaxf(v, 0.0f);
                        a[u].v[ch][s] = (ok && cbase + ch * 8 + 4 * half + s < p.Cin) ? v : 0.0f;
                    }
                }
            }
            // B operands: one 16-byte LDS read per (chunk, column block) gives the four channel steps of this lane.  The
            // reads of the first two chunks are issued ahead of the first MFMAs and the rest between MFMA groups
            // (sched_group_barrier: left alone the scheduler sinks each read to just in front of its MFMA pair and
            // every pair then sits behind an LDS round trip).
            float4 bq[NCH][NT];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    bq[ch][t] = *reinterpret_cast<const float4 *>(wk + (ch * 2 * NT + t) * 128);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][0], bq[ch][t].x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][1], bq[ch][t].y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][2], bq[ch][t].z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][3], bq[ch][t].w, acc[t], 0, 0, 0);
                }
            __builtin_amdgcn_sched_group_barrier(0x100, NCH >= 2 ? 2 * NT : NT, 0);   // DS reads of the first two chunks
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT, 0);               // MFMAs of chunk ch
                if (ch + 2 < NCH) __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);   // reads of chunk ch + 2
            }
        }
    };
    if (PIPE) {
        // software pipeline: the gathers of step b+1 are always issued (clamped past the end) before the
        // MFMAs of step b, so exactly KB * NCH loads are younger than the ones being waited for
        ARows a0[KB], a1[KB];
        int j0[KB], j1[KB];
        issue(0, a0, j0);
        for (int b = 0; b < total; b += 2) {
            issue(b + 1, a1, j1);
            consume(b, a0, j0);
            issue(b + 2, a0, j0);
            if (b + 1 < total) consume(b + 1, a1, j1);
        }
    } else {
        for (int b = 0; b < total; ++b) {
            ARows a[KB];
            int jj[KB];
            issue(b, a, jj);
            consume(b, a, jj);
        }
    }
    conv_epilogue<NT>(p, acc, LinearRows{wrow0, p.n_out}, col0, r32, half, wave, sW, (int)blockIdx.x, (int)gridDim.y);
}

template <int NT, int NCH>
int launch_resident_nch(const ConvParams &p, bool vec4, hipStream_t st, int nslab = 1)
{
    // weights of `kgroup` offsets resident at a time (a multiple of the gather batch, ~24 KB -> 4 workgroups per CU)
    // vec4: 16-byte aligned rows whose pitch covers Cin rounded up to 4; the buffer-load gathers address x with
    // 32-bit byte offsets formed by a 24-bit multiply
    const bool pipe = vec4 && p.x_bytes > 0 && p.x_bytes < 0x7fffffffll && (int64_t)p.ld_x * 4 < (1 << 24) &&
                      p.x_bytes / ((int64_t)p.ld_x * 4) < (1 << 24);
    const int KB = pipe ? (resident_kb(NCH) + 1) / 2 : resident_kb(NCH);  // the kernel's batch size: kgroup % KB == 0
    const size_t per_k = (size_t)NCH * 8 * 32 * NT * sizeof(float);
    constexpr int group_kb = 24;   // (36 KB: -1 %, 48 KB = two workgroups per CU: +37 %)
    int kgroup = (int)max((size_t)KB, (size_t)(group_kb * 1024) / per_k / KB * KB);
    kgroup = min(kgroup, (p.K + KB - 1) / KB * KB);
    const size_t lds = max((size_t)kgroup * per_k + (size_t)p.K * kRowsPerBlock * sizeof(int) +
                               (size_t)2 * nslab * NCH * 8 * sizeof(float),
                           max((size_t)kWaves * 3 * 32 * NT, (size_t)3 * 256) * sizeof(float));
    const dim3 grid((unsigned)ceil_div(p.n_out, kRowsPerBlock), (unsigned)ceil_div(p.Cout, 32 * NT));
    if (pipe)
        hipLaunchKernelGGL((spconv_resident_kernel<NT, true, NCH, true>), grid, dim3(256), lds, st, p, kgroup, nslab);
    else if (vec4)
        hipLaunchKernelGGL((spconv_resident_kernel<NT, true, NCH, false>), grid, dim3(256), lds, st, p, kgroup, nslab);
    else
        hipLaunchKernelGGL((spconv_resident_kernel<NT, false, NCH, false>), grid, dim3(256), lds, st, p, kgroup, nslab);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

template <int NT>
int launch_resident(const ConvParams &p, bool vec4, int cin_pad, hipStream_t st)
{
    // wide inputs: the fewest slabs of at most 64 channels, all of the same width (8 * NCH)
    const int chunks = cin_pad / 8;
    const int nslab = (chunks + 7) / 8;
    const int nch = (chunks + nslab - 1) / nslab;
    switch (nch) {
        case 1: return launch_resident_nch<NT, 1>(p, vec4, st, nslab);
        case 2: return launch_resident_nch<NT, 2>(p, vec4, st, nslab);
        case 3: return launch_resident_nch<NT, 3>(p, vec4, st, nslab);
        case 4: return launch_resident_nch<NT, 4>(p, vec4, st, nslab);
        case 5: return launch_resident_nch<NT, 5>(p, vec4, st, nslab);
        case 6: return launch_resident_nch<NT, 6>(p, vec4, st, nslab);
        case 7: return launch_resident_nch<NT, 7>(p, vec4, st, nslab);
        default: return launch_resident_nch<NT, 8>(p, vec4, st, nslab);
    }
}

template <int NT>
int launch_conv(const ConvParams &p, bool vec4, hipStream_t st)
{
    const dim3 grid((unsigned)ceil_div(p.n_out, kRowsPerBlock), (unsigned)ceil_div(p.Cout, 32 * NT));
    const size_t lds = (size_t)2 * kSlabC * 32 * NT * sizeof(float) +
                       (size_t)p.K * kRowsPerBlock * sizeof(int) + (size_t)((p.K + 3) & ~3) * sizeof(int) +
                       (size_t)2 * ((p.Cin + 3) & ~3) * sizeof(float) + 16;
    if (vec4)
        hipLaunchKernelGGL((spconv_mfma_kernel<NT, true>), grid, dim3(256), lds, st, p);
    else
        hipLaunchKernelGGL((spconv_mfma_kernel<NT, false>), grid, dim3(256), lds, st, p);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// ---------------------------------------------------------------------------------------------
// Dense 2D 3x3 'same' convolution, narrow layers (9 * cin_pad * 32 NT floats of weights fit LDS):
// implicit GEMM on an image tile.  A workgroup owns 8 rows x 16 pixels of one map; the 10 x 18 halo
// tile of the input is staged ONCE in LDS with coalesced 16-byte loads (the producer's pending
// BatchNorm + ReLU applied on the way in, zero padding outside the image), together with all nine
// weight matrices; the nine offsets then read their A operands from LDS (one ds_read_b128 per chunk),
// so the inner loop has no global memory access at all.  The gather form of the same layer re-reads
// every input row nine times through L1/L2 and pays a memory latency per batch of offsets:
// 53 us for 24->24 on 172,800 pixels (1.8 GFLOP).  Epilogue: the shared one (bias, ReLU, residual,
// BatchNorm summaries).
//   wave w -> tile rows 2w, 2w+1 (32 pixels); MFMA row r32 -> pixel (2w + r32 / 16, r32 % 16)
// ---------------------------------------------------------------------------------------------
constexpr int kTileH = 8, kTileW = 16;
constexpr int kHaloH = kTileH + 2, kHaloW = kTileW + 2;

template <int NT, int NCH>
__global__ __launch_bounds__(256) void conv2d_tile_kernel(ConvParams p, int tiles_x, int tiles_y)
{
    constexpr int cin_pad = NCH * 8;
    constexpr int P = cin_pad + 4;  // LDS pixel pitch in floats: 16 consecutive pixels hit 16 distinct bank quads
    constexpr int TN = 32 * NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sW = reinterpret_cast<float *>(smem);               // [9][cin_pad][TN], zero padded
    float *sX = sW + 9 * cin_pad * TN;                         // [kHaloH][kHaloW][P]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, map = blockIdx.y;
    const int col0 = blockIdx.z * TN;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const size_t map_row0 = (size_t)map * p.img_h * p.img_w;

    // (BatchNorm form (c): the input's pending BatchNorm comes as an accumulator block -> its affine form in LDS first)
    __shared__ __attribute__((aligned(16))) float sInAff[2 * cin_pad];
    if (p.in_acc) {
        stage_in_affine<256>(p, sInAff, cin_pad, tid);
        __syncthreads();
    }
    // ---- stage the weights of all nine offsets and the halo tile; one barrier ----
    if (cin_pad == p.Cin) {
        stage_weights<TN>(sW, p.w + col0, 0, 9 * p.Cin, p.Cout, p.Cout - col0, 9 * cin_pad, tid);
    } else {  // rows of an offset are not contiguous in the padded layout
        for (int k = 0; k < 9; ++k)
            stage_weights<TN>(sW + k * cin_pad * TN, p.w + col0, k * p.Cin, (k + 1) * p.Cin, p.Cout, p.Cout - col0, cin_pad, tid);
    }
    constexpr int C4 = cin_pad / 4;
    constexpr int kHaloItems = kHaloH * kHaloW * C4;
    constexpr int kHaloIter = (kHaloItems + 255) / 256;
    float4 hv[kHaloIter];
#pragma unroll
    for (int it = 0; it < kHaloIter; ++it) {  // all loads first (clamped addresses), then the fix-ups and LDS stores
        const int e = min(tid + it * 256, kHaloItems - 1);
        const int px = e / C4, c4 = e - px * C4;
        const int hy = px / kHaloW, hx = px - hy * kHaloW;
        const int y = min(max(y0 - 1 + hy, 0), p.img_h - 1), x = min(max(x0 - 1 + hx, 0), p.img_w - 1);
        hv[it] = *reinterpret_cast<const float4 *>(p.x + (map_row0 + (size_t)y * p.img_w + x) * p.ld_x + min(c4 * 4, p.Cin - 4));
    }
#pragma unroll
    for (int it = 0; it < kHaloIter; ++it) {
        const int e = tid + it * 256;
        if (e >= kHaloItems) break;
        const int px = e / C4, c4 = e - px * C4;
        const int hy = px / kHaloW, hx = px - hy * kHaloW;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        const int c = c4 * 4;
        float4 v = hv[it];
        if (p.in_scale) {
            float4 sc, sh;
            if (p.in_acc) {
                sc = *reinterpret_cast<const float4 *>(sInAff + min(c, cin_pad - 4));
                sh = *reinterpret_cast<const float4 *>(sInAff + cin_pad + min(c, cin_pad - 4));
            } else {
                sc = *reinterpret_cast<const float4 *>(p.in_scale + min(c, p.Cin - 4));
                sh = *reinterpret_cast<const float4 *>(p.in_shift + min(c, p.Cin - 4));
            }
            v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y);
            v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
            if (p.in_relu) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
        }
        if (!(y >= 0 && y < p.img_h && x >= 0 && x < p.img_w && c < p.Cin)) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(sX + px * P + c) = v;
    }
    __syncthreads();

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int ry = 2 * wave + (r32 >> 4), rx = r32 & 15;  // this lane's pixel inside the tile
    const float *xa = sX + (ry * kHaloW + rx) * P + 4 * half;
    const float *wb = sW + r32 + 4 * half * TN;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float *xk = xa + ((k / 3) * kHaloW + (k % 3)) * P;
        const float *wk = wb + k * cin_pad * TN;
        float4 av[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) av[ch] = *reinterpret_cast<const float4 *>(xk + ch * 8);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            float b[4][NT];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < NT; ++t) b[q][t] = wk[(ch * 8 + q) * TN + t * 32];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].x, b[0][t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].y, b[1][t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].z, b[2][t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].w, b[3][t], acc[t], 0, 0, 0);
            }
        }
    }
    const int wy0 = y0 + 2 * wave;
    const ImageRows rm{(int)(map_row0 + (size_t)wy0 * p.img_w + x0), wy0, x0, p.img_h, p.img_w};
    const int partial_row = ((int)blockIdx.y * tiles_y + ty) * tiles_x + tx;
    conv_epilogue<NT>(p, acc, rm, col0, r32, half, wave, sW, partial_row, (int)gridDim.z);
}

size_t conv2d_tile_lds(int nt, int nch) { return ((size_t)9 * nch * 8 * 32 * nt + (size_t)kHaloH * kHaloW * (nch * 8 + 4)) * sizeof(float); }

// eligibility of the tile kernel; on success *blocks = workgroups per column block (= BatchNorm summary rows)
bool conv2d_tile_ok(const ConvParams &p, int *nt_out, int *nch_out, int64_t *blocks)
{
    if (p.K != 9 || p.img_h <= 0 || p.img_w <= 0 || p.img_maps <= 0 || p.ln || p.accumulate)
        return false;
    if ((int64_t)p.img_maps * p.img_h * p.img_w != p.n_out) return false;
    if (p.Cin % 4 != 0 || p.ld_x % 4 != 0 || (reinterpret_cast<uintptr_t>(p.x) & 15) != 0) return false;
    if (p.in_scale && ((reinterpret_cast<uintptr_t>(p.in_scale) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.in_shift) & 15) != 0))
        return false;
    const int nch = (p.Cin + 7) / 8;
    if (nch > 5) return false;
    const int nt = 1;  // 32-column blocks over blockIdx.z keep the nine weight matrices within LDS
    if (conv2d_tile_lds(nt, nch) > 96 * 1024) return false;
    const int tiles = ((p.img_h + kTileH - 1) / kTileH) * ((p.img_w + kTileW - 1) / kTileW);
    if ((int64_t)tiles * p.img_maps < 256) return false;  // short lists: the column-split gather form fills the chip better
    *nt_out = nt; *nch_out = nch; *blocks = (int64_t)tiles * p.img_maps;
    return true;
}

template <int NCH>
int launch_conv2d_tile(const ConvParams &p, hipStream_t st)
{
    const int tiles_x = (p.img_w + kTileW - 1) / kTileW, tiles_y = (p.img_h + kTileH - 1) / kTileH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)p.img_maps, (unsigned)ceil_div(p.Cout, 32));
    const size_t lds = max(conv2d_tile_lds(1, NCH), (size_t)3 * 256 * sizeof(float));
    if (lds > 64 * 1024) {  // above the default dynamic-LDS limit: opt in once per instantiation
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv2d_tile_kernel<1, NCH>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        if (attr != hipSuccess) return EPRECON_ERR_HIP_BASE - (int)attr;
    }
    hipLaunchKernelGGL((conv2d_tile_kernel<1, NCH>), grid, dim3(256), lds, st, p, tiles_x, tiles_y);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// ---------------------------------------------------------------------------------------------
// Dense-grid 3x3x3 stride-1 convolution: the 3D twin of conv2d_tile_kernel, for voxel sets that fill most of their
// bounding grid (the initialisation stack runs on 85 % of the dense 48^3 grid, models/occupancy_initialization.py:131-174).
// The gather form re-reads every input row 27 times through L1/L2 behind a [27][N] kernel map and pays a memory
// latency per batch of offsets (73 us for 32 -> 32 on 94k voxels, 0.40 of the MFMA bound; ablation: gathers alone 53 us).
// Here a workgroup owns a 4 x 4 x 8 block of grid cells (x slowest, z fastest = the row order of a raster-ordered set):
//   1. the rank volume gives the row of each of the 6 x 6 x 10 halo cells (-1: no voxel)          -> LDS (360 ints)
//   2. the halo rows are staged ONCE with coalesced 16-byte loads, the producer's pending BatchNorm (+ReLU) applied on
//      the way in, zeros where there is no voxel                                                   -> LDS (360 x (C_in + 4) floats)
//   3. the 27 offsets read their A operands from LDS with one ds_read_b128 per 8-channel chunk at compile-time offsets
//      (no address arithmetic in the loop).  B operands do NOT go through LDS: the weights are pre-packed in operand
//      order (pack_weights_kernel), so a wave fetches the four channel steps of a chunk with ONE coalesced 1 KB
//      global_load_dwordx4 (L1 / L2 hits: every wave of the chip reads the same 27 * C_in * C_out * 4 bytes), issued two
//      chunks ahead of its MFMAs.  No weight staging, no barrier inside the MFMA loop, 53 KB of LDS at C_in = 32:
//      three workgroups per CU, so one workgroup's staging overlaps the others' MFMAs.
//   4. the shared epilogue (bias, ReLU, residual, BatchNorm summaries or row-wise LayerNorm); rows are addressed
//      through the ranks, cells without a voxel are computed and dropped.
// Bit-identical to the gather kernels: the same k-ordered fma chain per output element, zeros for missing neighbours.
// No kernel map and no hash grid are needed for such layers.
//   wave w -> x = x0 + w; MFMA row r32 -> (y, z) = (y0 + r32 / 8, z0 + r32 % 8)
// ---------------------------------------------------------------------------------------------
// tile = WV x 4 x 8 cells, one wave per x slice (WV waves per workgroup).  WV = 2 for the MFMA kernel: what balances the
// chip is the number of 32-row wave jobs (11.5 us of MFMAs each at C_in = C_out = 32) per SIMD, and 64-cell workgroups
// with a 35 KB halo fit four to a CU where 128-cell workgroups with 52 KB fit three and ran the 94k-voxel layer in two
// rounds (measured 88 us against 73 us for the gather form; profiles/r03/conv3d_probe.txt)
constexpr int kD3Y = 4, kD3Z = 8;
constexpr int kD3HY = kD3Y + 2, kD3HZ = kD3Z + 2;
constexpr int d3_halo(int wv) { return (wv + 2) * kD3HY * kD3HZ; }
constexpr int kD3WvNarrow = 4;

// Weights [K][Cin][Cout] -> MFMA operand order, zero padded, one slab per block of 32 * nt output columns:
//   wq[(((((cb * K + k) * NCH + ch) * 2 + half) * NT + t) * 32 + col) * 4 + s] = W[k][ch*8 + 4*half + s][cb*32*NT + 32 t + col]
// (the float4 a lane (half, col) multiplies with its four consecutive input channels of chunk ch)
__device__ __forceinline__ void pack_weights_body(const float *w, int K, int Cin, int Cout, int nch, int nt, int ncb, float *wq,
                                                  int first, int step)
{
    const int total = ncb * K * nch * 2 * nt * 32 * 4;
    for (int e = first; e < total; e += step) {
        const int sidx = e & 3, col = (e >> 2) & 31;
        int r = e >> 7;
        const int t = r % nt; r /= nt;
        const int half = r & 1; r >>= 1;
        const int ch = r % nch; r /= nch;
        const int k = r % K, cb = r / K;
        const int c = ch * 8 + 4 * half + sidx, co = (cb * nt + t) * 32 + col;
        wq[e] = (c < Cin && co < Cout) ? w[((size_t)k * Cin + c) * Cout + co] : 0.0f;
    }
}
__global__ void pack_weights_kernel(const float *w, int K, int Cin, int Cout, int nch, int nt, int ncb, float *wq)
{
    pack_weights_body(w, K, Cin, Cout, nch, nt, ncb, wq, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}
// the (NT, column blocks) the dense-grid kernel uses for C_out output channels; the packing follows it
__host__ __device__ inline void d3_columns(int cout, int *nt, int *ncb) { *nt = cout <= 32 ? 1 : 2; *ncb = (cout + 32 * *nt - 1) / (32 * *nt); }

template <int WV>
__device__ __forceinline__ void d3_tile_origin(int tile, int tiles_y, int tiles_z, int &x0, int &y0, int &z0)
{
    const int tz = tile % tiles_z, ty = (tile / tiles_z) % tiles_y, tx = tile / (tiles_z * tiles_y);
    x0 = tx * WV; y0 = ty * kD3Y; z0 = tz * kD3Z;
}

// steps 1 + 2 of the tile kernels: the row (rank) of every halo cell -> the first pad word of the cell, halo rows -> sX
// (pitch P = cin_pad + 4 floats; no separate rank array: 51,840 bytes at C_in = 32, three workgroups per CU).
// Returns false (block-uniform) when no cell of the tile holds a voxel.
__device__ __forceinline__ int d3_rank(const float *sX, int cell, int P, int cin_pad) { return __float_as_int(sX[cell * P + cin_pad]); }

// step 1: rows (ranks) of the halo cells -> the first pad word of each cell; false (block-uniform) for a tile without a voxel
template <int NCH, int WV, int THREADS = 64 * WV>
__device__ __forceinline__ bool d3_stage_ranks(const ConvParams &p, int x0, int y0, int z0, float *sX, int tid)
{
    constexpr int cin_pad = NCH * 8, P = cin_pad + 4;
    constexpr int kThreads = THREADS, kD3Halo = d3_halo(WV);
    for (int e = tid; e < kD3Halo; e += kThreads) {
        const int hz = e % kD3HZ, hy = (e / kD3HZ) % kD3HY, hx = e / (kD3HZ * kD3HY);
        const int x = x0 - 1 + hx, y = y0 - 1 + hy, z = z0 - 1 + hz;
        const bool in = x >= 0 && x < p.gx && y >= 0 && y < p.gy && z >= 0 && z < p.gz;
        sX[e * P + cin_pad] = __int_as_float(in ? p.vox_rank[((size_t)x * p.gy + y) * p.gz + z] : -1);
    }
    __syncthreads();
    // this thread's output cell (the threads cover the 32 WV cells at least once)
    const int v = tid % (32 * WV);
    const int own = d3_rank(sX, (((v >> 5) + 1) * kD3HY + ((v >> 3) & 3) + 1) * kD3HZ + (v & 7) + 1, P, cin_pad);
    return __syncthreads_or(own >= 0) != 0;
}

// step 2: channels [cbase, cbase + 8 NCH) of the halo rows -> sX (pitch P = 8 NCH + 4 floats), the producer's pending BatchNorm
// (+ReLU) applied on the way in, zeros where there is no voxel or no channel.  Ends with a barrier.
template <int NCH, int WV, int THREADS = 64 * WV>
__device__ __forceinline__ void d3_stage_rows(const ConvParams &p, float *sX, int tid, int dbg, int cbase)
{
    constexpr int cin_pad = NCH * 8, P = cin_pad + 4, C4 = cin_pad / 4;
    constexpr int kThreads = THREADS, kD3Halo = d3_halo(WV);
    constexpr int kItems = kD3Halo * C4;
    constexpr int kIter = (kItems + kThreads - 1) / kThreads;
    float4 hv[kIter];
    int hr[kIter];
    const int last4 = ((p.Cin + 3) & ~3) - 4;
    // the channel group of an item is tid % C4 in every iteration when C4 divides the block size: its scale / shift are loaded once
    constexpr bool kFixedGroup = kThreads % C4 == 0;
    float4 sc0 = make_float4(1.f, 1.f, 1.f, 1.f), sh0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kFixedGroup && p.in_scale) {
        sc0 = *reinterpret_cast<const float4 *>(p.in_scale + min(cbase + (tid % C4) * 4, last4));
        sh0 = *reinterpret_cast<const float4 *>(p.in_shift + min(cbase + (tid % C4) * 4, last4));
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {  // all loads first (clamped addresses), then the fix-ups and LDS stores
        const int e = min(tid + it * kThreads, kItems - 1);
        const int cell = e / C4, c4 = e - cell * C4;
        hr[it] = d3_rank(sX, cell, P, cin_pad);
        if (dbg & 4) hv[it] = make_float4(1.f, 1.f, 1.f, 1.f);
        else hv[it] = *reinterpret_cast<const float4 *>(p.x + (size_t)max(hr[it], 0) * p.ld_x + min(cbase + c4 * 4, last4));
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int e = tid + it * kThreads;
        if (e >= kItems) break;
        const int cell = e / C4, c4 = e - cell * C4;
        const int c = cbase + c4 * 4;
        float4 v4 = hv[it];
        if (p.in_scale) {
            float4 sc = sc0, sh = sh0;
            if (!kFixedGroup) {
                sc = *reinterpret_cast<const float4 *>(p.in_scale + min(c, last4));
                sh = *reinterpret_cast<const float4 *>(p.in_shift + min(c, last4));
            }
            v4.x = fmaf(v4.x, sc.x, sh.x); v4.y = fmaf(v4.y, sc.y, sh.y);
            v4.z = fmaf(v4.z, sc.z, sh.z); v4.w = fmaf(v4.w, sc.w, sh.w);
            if (p.in_relu) {
                v4.x = fmaxf(v4.x, 0.f); v4.y = fmaxf(v4.y, 0.f); v4.z = fmaxf(v4.z, 0.f); v4.w = fmaxf(v4.w, 0.f);
            }
        }
        if (hr[it] < 0 || c >= p.Cin) v4 = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(sX + cell * P + c4 * 4) = v4;
    }
    __syncthreads();
}

template <int NCH, int WV, int THREADS = 64 * WV>
__device__ __forceinline__ bool d3_stage_halo(const ConvParams &p, int x0, int y0, int z0, float *sX, int tid, int dbg)
{
    if (!d3_stage_ranks<NCH, WV, THREADS>(p, x0, y0, z0, sX, tid)) return false;
    d3_stage_rows<NCH, WV, THREADS>(p, sX, tid, dbg, 0);
    return true;
}

// C_out == 1 (the occupancy-logit layer, models/occupancy_initialization.py:171): a 32-column MFMA tile would spend 31/32
// of its work on padding.  Same halo staging; two lanes per cell split the 16-byte channel groups, the weights of the one
// output column come from LDS as broadcasts, plain fma chains, the BatchNorm summary of the tile by Chan merges in
// lane / wave order.
template <int NCH>
__global__ __launch_bounds__(256) void conv3d_tile_narrow_kernel(ConvParams p, int tiles_y, int tiles_z, int ntiles)
{
    constexpr int cin_pad = NCH * 8, P = cin_pad + 4, C4 = cin_pad / 4;
    constexpr int WV = kD3WvNarrow, kD3Halo = d3_halo(WV);
    static_assert(WV == 4, "the cell mapping below covers 128 cells with 256 threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sX = reinterpret_cast<float *>(smem);
    float *sWn = sX + kD3Halo * P;                            // [27][cin_pad] weights of the single column, zero padded
    float *sRed = sWn + 27 * cin_pad;                          // [4][3] wave summaries
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    if (tile >= ntiles) return;
    int x0, y0, z0;
    d3_tile_origin<WV>(tile, tiles_y, tiles_z, x0, y0, z0);
    for (int e = tid; e < 27 * cin_pad; e += 256) {
        const int k = e / cin_pad, c = e - k * cin_pad;
        sWn[e] = c < p.Cin ? p.w[((size_t)k * p.Cin + c) * p.Cout] : 0.0f;
    }
    if (!d3_stage_halo<NCH, WV>(p, x0, y0, z0, sX, tid, p.debug)) {  // (its barriers also publish sWn)
        if (p.bn_partial && tid == 0) bn_partial_store(p, tile, 0, 0.0f, 0.0f, 0.0f);
        return;
    }
    const int v = tid >> 1, part = tid & 1;  // cell (x = v / 32, y = (v / 8) % 4, z = v % 8), half of the channel groups
    const int cell0 = (((v >> 5) + 1) * kD3HY + ((v >> 3) & 3) + 1) * kD3HZ + (v & 7) + 1;
    const int row = d3_rank(sX, cell0, P, cin_pad);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
        const float *xk = sX + (cell0 + (dx * kD3HY + dy) * kD3HZ + dz) * P;
#pragma unroll
        for (int j = 0; j < C4 / 2; ++j) {
            const int c = (2 * j + part) * 4;
            const float4 a = *reinterpret_cast<const float4 *>(xk + c);
            const float4 w = *reinterpret_cast<const float4 *>(sWn + k * cin_pad + c);
            acc = fmaf(a.x, w.x, acc); acc = fmaf(a.y, w.y, acc); acc = fmaf(a.z, w.z, acc); acc = fmaf(a.w, w.w, acc);
        }
    }
    acc += __shfl_xor(acc, 1);
    float n = 0.0f, mean = 0.0f, m2 = 0.0f;
    if (part == 0 && row >= 0) {
        float *o = p.out + (size_t)row * p.ld_out;
        float val = acc + (p.bias ? p.bias[0] : 0.0f);
        if (p.accumulate) val += *o;
        if (p.relu) val = fmaxf(val, 0.0f);
        if (p.res) {
            float rv = p.res[(size_t)row * p.ld_res];
            if (p.res_scale) {
                rv = fmaf(rv, p.res_scale[0], p.res_shift[0]);
                if (p.res_relu) rv = fmaxf(rv, 0.0f);
            }
            val += rv;
        }
        *o = val;
        n = 1.0f; mean = val;
    }
    if (p.bn_partial) {  // (uniform)
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {  // lane-order tree: the lower lane of a pair is the left operand
            const float on = __shfl_xor(n, m), omean = __shfl_xor(mean, m), om2 = __shfl_xor(m2, m);
            const bool lower = (lane & m) == 0;
            float a_n = lower ? n : on, a_mean = lower ? mean : omean, a_m2 = lower ? m2 : om2;
            chan_merge(a_n, a_mean, a_m2, lower ? on : n, lower ? omean : mean, lower ? om2 : m2);
            n = a_n; mean = a_mean; m2 = a_m2;
        }
        if (lane == 0) { sRed[wave * 3] = n; sRed[wave * 3 + 1] = mean; sRed[wave * 3 + 2] = m2; }
        __syncthreads();
        if (tid == 0) {
            float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
            for (int w = 0; w < kWaves; ++w) chan_merge(a_n, a_mean, a_m2, sRed[w * 3], sRed[w * 3 + 1], sRed[w * 3 + 2]);
            bn_partial_store(p, tile, 0, a_n, a_mean, a_m2);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 16-row form of the dense-grid kernel on v_mfma_f32_16x16x4_f32, for C_out <= 32 and C_in a multiple of 16.
// The 32-row tile kernel loses on the 94k-voxel initialisation set because its unit of work is too coarse (DESIGN.md 3b:
// 3.1 jobs of 11.5 us per SIMD = four rounds) and because a 32-column MFMA tile is half empty for the C_out = 16 layers.
// Here a workgroup owns 2 x 4 x 8 cells (halo 4 x 6 x 10 = 240 cells, 35 KB at C_in = 32: four workgroups per CU), a wave
// 16 of them (one x, two y, eight z) in CT accumulator tiles of 16 x 16; a job is a quarter of the 32-row kernel's.
//   A operand (lane l: row l & 15, k index q = l >> 4): x[cell(row)][16 kc + 4 q + s] for step s — one ds_read_b128 per chunk
//   B operand: W[k][16 kc + 4 q + s][16 t + (l & 15)], pre-packed so that a wave fetches (k, kc, t) with one 1 KB buffer load
//   C / D: column l & 15, rows 4 (l >> 4) + reg
// Summation order differs from the 32x32x2 kernels (four channels per MFMA): equal within fp32 round-off, not bit for bit.
// Own epilogue for this accumulator layout (conv_common.hpp: tile16_epilogue, shared with the 2D twin conv2d_tile16_kernel):
// bias, ReLU, residual (with its pending BatchNorm), row-wise LayerNorm, BatchNorm summaries.
// ---------------------------------------------------------------------------------------------
constexpr int kD16X = 2;                                     // tile x extent; y, z as the other tile kernels
constexpr int kD16Halo = (kD16X + 2) * kD3HY * kD3HZ;        // 240

// wq16[((((k * KCH + kc) * CT + t) * 4 + q) * 16 + col) * 4 + s] = W[k][16 kc + 4 q + s][16 t + col]
// Tail section (C_out = 16 (ct - 1) + 1 .. 8 only), behind the tiles: the last <= 8 columns once more in the operand order of
// v_mfma_f32_4x4x1_16B_f32 as the direct gather kernel feeds it (csrc/sparse_conv_direct.hip: tail_to_tile) —
//   tail[((((k * KCH + kc) * 2 + cg) * 4 + q) * 4 + n) * 4 + s] = W[k][16 kc + 4 q + s][16 (ct - 1) + 4 cg + n]
__device__ __forceinline__ void pack_weights16_body(const float *w, int K, int Cin, int Cout, int kch, int ct, float *wq, int first,
                                                    int step)
{
    const int total = K * kch * ct * 256;
    const int rem = Cout - 16 * (ct - 1);
    const int total_tail = (rem >= 1 && rem <= 8) ? K * kch * 128 : 0;
    for (int e = first; e < total_tail; e += step) {
        const int sidx = e & 3, n = (e >> 2) & 3, q = (e >> 4) & 3, cg = (e >> 6) & 1;
        const int r = e >> 7;
        const int kc = r % kch, k = r / kch;
        const bool tail8 = kc == kch - 1 && Cin - 16 * kc <= 8;
        const int c = tail8 ? (sidx < 2 ? 16 * kc + 2 * q + sidx : Cin) : 16 * kc + 4 * q + sidx;
        const int co = 16 * (ct - 1) + 4 * cg + n;
        wq[(size_t)total + e] = (c < Cin && co < Cout) ? w[((size_t)k * Cin + c) * Cout + co] : 0.0f;
    }
    for (int e = first; e < total; e += step) {
        const int sidx = e & 3, col = (e >> 2) & 15, q = (e >> 6) & 3;
        int r = e >> 8;
        const int t = r % ct; r /= ct;
        const int kc = r % kch, k = r / kch;
        // a last chunk of <= 8 channels is laid out for TWO MFMAs (k index q <-> channels 2 q, 2 q + 1) instead of four
        const bool tail8 = kc == kch - 1 && Cin - 16 * kc <= 8;
        const int c = tail8 ? (sidx < 2 ? 16 * kc + 2 * q + sidx : Cin) : 16 * kc + 4 * q + sidx;
        const int co = 16 * t + col;
        wq[e] = (c < Cin && co < Cout) ? w[((size_t)k * Cin + c) * Cout + co] : 0.0f;
    }
}
__global__ void pack_weights16_kernel(const float *w, int K, int Cin, int Cout, int kch, int ct, float *wq)
{
    pack_weights16_body(w, K, Cin, Cout, kch, ct, wq, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// Many packings in ONE launch (eprecon_conv_pack_many_async): block (x, y) works on job y.  An optimisation step changes every
// weight, so every layer's operand-order copies are rebuilt once per step: ~190 launches of 4 us as separate calls.
__global__ void pack_many_kernel(const eprecon_pack_job *jobs)
{
    const eprecon_pack_job j = jobs[blockIdx.y];
    const int first = blockIdx.x * blockDim.x + threadIdx.x, step = gridDim.x * blockDim.x;
    if (j.kind == 0) {
        int nt, ncb;
        d3_columns(j.cout, &nt, &ncb);
        pack_weights_body(j.weight, j.kvol, j.cin, j.cout, (j.cin + 7) / 8, nt, ncb, j.packed, first, step);
    } else {
        pack_weights16_body(j.weight, j.kvol, j.cin, j.cout, (j.cin + 15) / 16, (j.cout + 15) / 16, j.packed, first, step);
    }
}

// EP_TILE16_MIX (compile time): 1 (default) the loads an offset issues — CT weight quads two offsets ahead, the next offset's A
// quad from LDS — are spread among its 4 CT MFMAs (sched_group_barrier: one VMEM read per four MFMAs, then the LDS read) instead
// of issued in front of them behind a scheduling fence (0: the round-3..5 schedule; 2: no fence at all, the compiler's choice —
// measured equal to 0).  32 -> 32 + LayerNorm on the 94k-voxel set: 71.3 -> 64.5 us, 0.44 -> 0.49 of the fp32-MFMA peak; the cfg2
// step 1.595 -> 1.574 ms (tools/probes/t16_ab.sh, two interleaved rounds).  The same products in the same order: bit-identical.
#ifndef EP_TILE16_MIX
#define EP_TILE16_MIX 1
#endif
template <int CT, int KCH>
__global__ __launch_bounds__(256, 7) void conv3d_tile16_kernel(ConvParams p, int tiles_y, int tiles_z, int ntiles)
{
    // The input channels are walked in KCH PASSES of 16: the halo tile in LDS holds 16 channels at a time (240 cells x 80 B =
    // 19.2 KB whatever C_in is), so that seven to eight workgroups fit a CU and ALL tiles of the 94k-voxel set (1,594 non-empty,
    // 6.2 per CU) are resident at once — with the 32-channel halo (35 KB, four per CU) the layer ran in two batches and its
    // MFMA loop took 58 us for 36 us of MFMAs.  Accumulators carry over; one staging + barrier per pass.
    constexpr int cin_pad = 16, NCH = 2;
    constexpr int P = cin_pad + 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sX = reinterpret_cast<float *>(smem);   // [kD16Halo][P]: 16 channels + the cell's row in the first pad word
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    if (tile >= ntiles) return;
    int x0, y0, z0;
    d3_tile_origin<kD16X>(tile, tiles_y, tiles_z, x0, y0, z0);
    float *sStat = sX;  // (after the loop) [4 waves][3][16 CT] summaries

    if (!d3_stage_ranks<NCH, kD16X, 256>(p, x0, y0, z0, sX, tid)) {
        if (p.bn_partial && tid < 16 * CT && tid < p.Cout) bn_partial_store(p, tile, tid, 0.0f, 0.0f, 0.0f);
        return;
    }
    // wave -> (x = wave / 2, y pair = wave % 2); MFMA row r -> cell (y = 2 (wave % 2) + r / 8, z = r % 8)
    const int wx = wave >> 1, wy = 2 * (wave & 1);
    const int cell_a = ((wx + 1) * kD3HY + wy + (l16 >> 3) + 1) * kD3HZ + (l16 & 7) + 1;   // this lane's A row
    int orow[4];   // output rows of this lane's accumulator rows 4 q + j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * q + j;
        orow[j] = d3_rank(sX, ((wx + 1) * kD3HY + wy + (r >> 3) + 1) * kD3HZ + (r & 7) + 1, P, cin_pad);
    }
    const bool work = __ballot(d3_rank(sX, cell_a, P, cin_pad) >= 0) != 0ull && !(p.debug & 1);   // (wave-uniform)

    f32x4 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const float *xa = sX + (cell_a - (kD3HY + 1) * kD3HZ - 1) * P + 4 * q;
    constexpr unsigned kStepBytes = CT * 1024u, kOffBytes = KCH * kStepBytes;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq), 0, (int)(27 * kOffBytes), 0x00020000);
    const unsigned wlane = (unsigned)lane * 16u;
    constexpr int kAheadB = 2;
    for (int pass = 0; pass < KCH; ++pass) {
        if (pass > 0) __syncthreads();  // every wave is done reading the previous pass's channels
        d3_stage_rows<NCH, kD16X, 256>(p, sX, tid, p.debug, 16 * pass);
        if (!work) continue;
        float4 bq[kAheadB + 1][CT];
        float4 aq[2];
        auto load_b = [&](int k, float4(&dst)[CT]) {
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)t * 1024u,
                                                                      (unsigned)((p.debug & 2) ? 0 : k) * kOffBytes + (unsigned)pass * kStepBytes, 0);
                dst[t] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
        };
        auto load_a = [&](int k) {
            const int dx = k % 3, dy = (k / 3) % 3, dz = k / 9;
            return *reinterpret_cast<const float4 *>(xa + ((dx * kD3HY + dy) * kD3HZ + dz) * P);
        };
#pragma unroll
        for (int k = 0; k < kAheadB; ++k) load_b(k, bq[k]);
        aq[0] = load_a(0);
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            if (k + kAheadB < 27) load_b(k + kAheadB, bq[(k + kAheadB) % (kAheadB + 1)]);
            if (k + 1 < 27) aq[(k + 1) & 1] = load_a(k + 1);
#if EP_TILE16_MIX == 0
            __builtin_amdgcn_sched_barrier(0);
#endif
            const float4 av = aq[k & 1];
            const float4(&bk)[CT] = bq[k % (kAheadB + 1)];
            // the CT accumulators alternate: a 16x16x4 MFMA issues every 32 cycles but returns after 40
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bk[t].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bk[t].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bk[t].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bk[t].w, acc[t], 0, 0, 0);
#if EP_TILE16_MIX == 1      // (probe builds: this offset's loads spread among its MFMAs instead of in front of them)
#pragma unroll
            for (int sg = 0; sg < CT; ++sg) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();  // every wave is done with the halo: the summaries' scratch overlays it

    tile16_epilogue<CT>(p, acc, orow, sStat, tile);
}

enum D3Kind { kD3None = 0, kD3Narrow = 1, kD3Tile16 = 2 };

int d3_tiles_kind(const ConvParams &p, int kind, int *ty = nullptr, int *tz = nullptr)
{
    const int wv = kind == kD3Tile16 ? kD16X : kD3WvNarrow;
    const int tx = (p.gx + wv - 1) / wv, tyy = (p.gy + kD3Y - 1) / kD3Y, tzz = (p.gz + kD3Z - 1) / kD3Z;
    if (ty) *ty = tyy;
    if (tz) *tz = tzz;
    return tx * tyy * tzz;
}
size_t conv3d_narrow_lds(int nch)
{
    return ((size_t)d3_halo(kD3WvNarrow) * (nch * 8 + 4) + (size_t)27 * nch * 8 + 16) * sizeof(float);
}

// eligibility of the dense-grid kernels (independent of the data: shapes, alignment, fusions)
// EPRECON_CONV_DENSE3D: 0 off; 1 the single-column kernel only; 2 (default) also the 16-row MFMA kernel.
// Measured on the 94k-voxel initialisation set (rocprofv3 kernel durations, profiles/r03/conv3d_*):
//   32 -> 1   24 us   against 82 us for the gather form            (single-column kernel)
//   16 -> 16  24 us   against 50 us,  32 -> 16  37 us against 76 us,  32 -> 32  71 us against 78 us     (16-row kernel)
// (a 32-row tile kernel on v_mfma_f32_32x32x2_f32 was built in round 3, bit-identical to the gather form and slower on this
// set — 97 us against 78 us: 3,185 wave jobs of 11.5 us on 1,024 SIMDs = four rounds, DESIGN.md 3b — and removed in round 4.)
inline int d3_level()
{
    const char *e = getenv("EPRECON_CONV_DENSE3D");   // (read per launch: tests flip it)
    return e ? atoi(e) : 2;
}

// which dense-grid kernel takes this layer: level 1 the single-column kernel, level 2 also the 16-row MFMA kernel
// (C_out <= 32, C_in a multiple of 16); every other shape runs on the kernel map
int conv3d_kind(const ConvParams &p)
{
    const int level = d3_level();
    if (level <= 0 || !p.vox_rank || p.K != 27 || p.gx <= 0 || p.gy <= 0 || p.gz <= 0) return kD3None;
    if (p.Cin % 4 != 0 || p.Cin > 64 || p.ld_x % 4 != 0 || (reinterpret_cast<uintptr_t>(p.x) & 15) != 0) return kD3None;
    if (p.in_scale && ((reinterpret_cast<uintptr_t>(p.in_scale) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.in_shift) & 15) != 0))
        return kD3None;
    if (p.Cout == 1 && !p.ln) return kD3Narrow;
    if (level < 2 || p.accumulate) return kD3None;
    // (the caller packs the weights for the kernel ITS mirror of this rule picks — eprecon_amd/sparse.py DenseMap.kind —,
    // so a missing packing means "not this kernel", never an error)
    if (p.Cout <= 32 && p.Cin % 16 == 0 && !(p.ln && p.bn_partial) && p.wq16 && (reinterpret_cast<uintptr_t>(p.wq16) & 15) == 0)
        return kD3Tile16;
    return kD3None;
}
bool conv3d_tile_ok(const ConvParams &p, bool *narrow)
{
    const int kind = conv3d_kind(p);
    *narrow = kind == kD3Narrow;
    return kind != kD3None;
}

template <int CT, int KCH>
int launch_conv3d_tile16(const ConvParams &p, hipStream_t st)
{
    int ty, tz;
    const int ntiles = d3_tiles_kind(p, kD3Tile16, &ty, &tz);
    const size_t lds = max((size_t)kD16Halo * (16 + 4) * sizeof(float), (size_t)kWaves * 3 * 16 * CT * sizeof(float));
    if (lds > 64 * 1024) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv3d_tile16_kernel<CT, KCH>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (attr != hipSuccess) return EPRECON_ERR_HIP_BASE - (int)attr;
    }
    ConvParams q = p;
    q.wq = p.wq16;
    hipLaunchKernelGGL((conv3d_tile16_kernel<CT, KCH>), dim3((unsigned)ntiles), dim3(256), lds, st, q, ty, tz, ntiles);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int launch_conv3d_16(const ConvParams &p, hipStream_t st)
{
    const int kch = p.Cin / 16;
    if (p.Cout <= 16) {
        switch (kch) {
            case 1: return launch_conv3d_tile16<1, 1>(p, st);
            case 2: return launch_conv3d_tile16<1, 2>(p, st);
            case 3: return launch_conv3d_tile16<1, 3>(p, st);
            default: return launch_conv3d_tile16<1, 4>(p, st);
        }
    }
    switch (kch) {
        case 1: return launch_conv3d_tile16<2, 1>(p, st);
        case 2: return launch_conv3d_tile16<2, 2>(p, st);
        case 3: return launch_conv3d_tile16<2, 3>(p, st);
        default: return launch_conv3d_tile16<2, 4>(p, st);
    }
}

template <int NCH>
int launch_conv3d_narrow(const ConvParams &p, hipStream_t st)
{
    int ty, tz;
    const int ntiles = d3_tiles_kind(p, kD3Narrow, &ty, &tz);
    const size_t lds = conv3d_narrow_lds(NCH);
    if (lds > 64 * 1024) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv3d_tile_narrow_kernel<NCH>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (attr != hipSuccess) return EPRECON_ERR_HIP_BASE - (int)attr;
    }
    hipLaunchKernelGGL((conv3d_tile_narrow_kernel<NCH>), dim3((unsigned)ntiles), dim3(256), lds, st, p, ty, tz, ntiles);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int launch_conv3d_single_column(const ConvParams &p, hipStream_t st)
{
    switch ((p.Cin + 7) / 8) {
        case 1: return launch_conv3d_narrow<1>(p, st);
        case 2: return launch_conv3d_narrow<2>(p, st);
        case 3: return launch_conv3d_narrow<3>(p, st);
        case 4: return launch_conv3d_narrow<4>(p, st);
        case 5: return launch_conv3d_narrow<5>(p, st);
        case 6: return launch_conv3d_narrow<6>(p, st);
        case 7: return launch_conv3d_narrow<7>(p, st);
        default: return launch_conv3d_narrow<8>(p, st);
    }
}

// ---------------------------------------------------------------------------------------------
// Short lists with wide inputs (a few thousand voxels / the 10,800 pixels of the 1/16 maps, C_in > 64):
// there are too few 128-row tiles to fill the chip, nothing overlaps, and the slab kernel's time is the
// LENGTH of its dependent chain: K * ceil(C_in / 32) staged slabs, each a global round trip + barrier
// (108 for a 27-offset 128-channel layer, ~130 us).  Here a workgroup owns 32 rows x 32 columns and its
// four waves split the (offset, slab) list round-robin, each staging its own slabs into a wave-private LDS
// buffer (no workgroup barrier in the loop); the four partial accumulators are summed in fixed order
// through LDS at the end.  4x the workgroups, 1/4 of the chain.
// ---------------------------------------------------------------------------------------------
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
        const char *e = getenv("EPRECON_CONV_SPLITK_FAST");      // (read per launch: tests flip it)
        if (p.splitk_pipe == 2 && !(e && e[0] == '0')) {
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

// ---------------------------------------------------------------------------------------------
// Medium lists with wide channels (4k .. 40k rows, C_in >= 96, 64 < C_out <= 128: the coarsest level's ConvGRU and SPVCNN's
// up-stage).  The split-K kernel above is operand-bandwidth-bound there (a 64-row x 32-column workgroup
// fetches 384 B per input channel for 4,096 flops = 10.7 flops per byte out of L2).  Here a workgroup owns 128 rows x ALL
// columns: each (offset, 32-channel slab) of the operand-order packed weights (p.wq) is copied ONCE into LDS (double-buffered,
// one barrier per stage) and feeds the four waves' 32 rows x 3..4 column tiles — 27 flops per byte —, the gathers of the next
// stage are in flight meanwhile.  128-row workgroups alone would leave most CUs idle (74 for 9,415 rows), so the 27 offsets are
// split ACROSS workgroups (blockIdx.y): every split writes its accumulators as they sit in registers to the caller's
// workspace, and spconv_wide_reduce_kernel adds the splits in order and runs the shared epilogue.  Deterministic; the
// summation order differs from the other kernels' (equal within round-off).
// ---------------------------------------------------------------------------------------------
constexpr int kWideRows = 128;
constexpr int kWideSlabF4 = 2 * 512;   // float4 per staged slab: 2 column blocks x [4 chunks][2 halves][2 tiles][32 columns]

inline int wide_splits(int n_out)
{
    // workgroups wanted per launch (three fit a CU)
    constexpr int target = 640;   // (320: 165 us on 9,415 rows 192 -> 96 — one workgroup per CU —, 640: 123 us)
    const int blocks = (int)ceil_div(n_out, kWideRows);
    return max(2, min(13, (target + blocks / 2) / blocks));
}

template <int NTT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 3))) void spconv_wide_kernel(ConvParams p, int nsplit, float *partial)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int nch8 = (p.Cin + 7) / 8, nslab = (p.Cin + 31) / 32, cinA = (p.Cin + 3) & ~3;
    const int split = (int)blockIdx.y;
    const int k0 = split * p.K / nsplit, k1 = (split + 1) * p.K / nsplit, nk = k1 - k0;
    const int kmax = (p.K + nsplit - 1) / nsplit + 1;
    float4 *sB = reinterpret_cast<float4 *>(smem);                       // [2][kWideSlabF4]
    int *sNbr = reinterpret_cast<int *>(sB + 2 * kWideSlabF4);           // [kmax][kWideRows]
    float *sAff = reinterpret_cast<float *>(sNbr + kmax * kWideRows);    // [2][cinA]
    const int row0 = (int)blockIdx.x * kWideRows;

    for (int e = tid; e < nk * kWideRows; e += 256) {
        const int kk = e / kWideRows, r = e - kk * kWideRows;
        const int row = row0 + r;
        sNbr[e] = row < p.n_out ? p.nbr[(size_t)(k0 + kk) * p.n_out + row] : -1;
    }
    stage_in_affine<256>(p, sAff, cinA, tid);

    f32x16 acc[NTT];
#pragma unroll
    for (int t = 0; t < NTT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    // packed layout (pack_weights_kernel, NT = 2): float4 index ((cb * K + k) * nch8 + chunk) * 128 + (half * 2 + t) * 32 + col
    const float4 *wq4 = reinterpret_cast<const float4 *>(p.wq);
    // Offsets none of the workgroup's 128 rows has a neighbour at are skipped (no slab staged, no gathers, no MFMAs): ConvGRU's
    // second gate convolution runs on a voxel set without a single adjacent pair (the already scaled coordinates divided by
    // the resolution again, models/modules.py:216-217) — 26 of its 27 offsets are dead for every row.
    __shared__ int sLiveK[32];
    __syncthreads();   // sNbr / sAff are written
    int nlive = 0;
    for (int kk = 0; kk < nk; ++kk) {
        const int any = __syncthreads_or(tid < kWideRows && sNbr[kk * kWideRows + tid] >= 0);
        if (any) {
            if (tid == 0) sLiveK[nlive] = kk;
            ++nlive;
        }
    }
    __syncthreads();
    auto slab_src = [&](int st, int e) -> const float4 * {
        const int kl = st / nslab, sl = st - kl * nslab;
        const int kk = sLiveK[kl];
        const int cb = e >> 9, i = e & 511;
        const int chunk = min(4 * sl + (i >> 7), nch8 - 1);   // (a chunk past C_in multiplies zeros)
        return wq4 + ((size_t)(cb * p.K + k0 + kk) * nch8 + chunk) * 128 + (i & 127);
    };
    struct StageA {
        float4 a[4];
        int j, c0;
    };
    auto fetch_a = [&](int st, StageA &g) {
        const int kl = st / nslab, sl = st - kl * nslab;
        const int kk = sLiveK[kl];
        g.c0 = sl * 32;
        g.j = sNbr[kk * kWideRows + wave * 32 + r32];
        const float *xrow = p.x + (size_t)max(g.j, 0) * p.ld_x;
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) g.a[ch] = *reinterpret_cast<const float4 *>(xrow + min(g.c0 + ch * 8 + 4 * half, cinA - 4));
    };
    const int nst = nlive * nslab;
    static_assert(kWideSlabF4 == 4 * 256, "four float4 of a slab per thread");
    StageA cur, nxt;
    if (nst > 0) {
        const float4 s0 = *slab_src(0, tid), s1 = *slab_src(0, tid + 256), s2 = *slab_src(0, tid + 512), s3 = *slab_src(0, tid + 768);
        sB[tid] = s0; sB[tid + 256] = s1; sB[tid + 512] = s2; sB[tid + 768] = s3;
        fetch_a(0, cur);
    }
    for (int st = 0; st < nst; ++st) {
        const int stn = min(st + 1, nst - 1);
        // (named values, not an array: the array form was kept on the stack — scratch stores behind vmcnt waits in the loop)
        const float4 b0 = *slab_src(stn, tid), b1 = *slab_src(stn, tid + 256), b2 = *slab_src(stn, tid + 512), b3 = *slab_src(stn, tid + 768);
        fetch_a(stn, nxt);
        __syncthreads();   // slab st is in LDS; every wave is done with slab st - 1
        const float4 *buf = sB + (st & 1) * kWideSlabF4;
        const int c0 = cur.c0;
        float a[4][4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            a[ch][0] = cur.a[ch].x; a[ch][1] = cur.a[ch].y; a[ch][2] = cur.a[ch].z; a[ch][3] = cur.a[ch].w;
        }
        if (p.in_scale) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const int cc = min(c0 + ch * 8 + 4 * half, cinA - 4);
                const float4 sc4 = *reinterpret_cast<const float4 *>(sAff + cc);
                const float4 sh4 = *reinterpret_cast<const float4 *>(sAff + cinA + cc);
                const float sc[4] = {sc4.x, sc4.y, sc4.z, sc4.w}, sh[4] = {sh4.x, sh4.y, sh4.z, sh4.w};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float x = fmaf(a[ch][q], sc[q], sh[q]);
                    a[ch][q] = p.in_relu ? fmaxf(x, 0.0f) : x;
                }
            }
        }
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            const int c = c0 + ch * 8 + 4 * half;
#pragma unroll
            for (int q = 0; q < 4; ++q) a[ch][q] = (cur.j >= 0 && c + q < p.Cin) ? a[ch][q] : 0.0f;
        }
        const int nch = min(4, nch8 - c0 / 8);
        if (!(p.debug & 1)) {
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                if (ch < nch) {   // (uniform)
                    float4 b4[NTT];
#pragma unroll
                    for (int t = 0; t < NTT; ++t) b4[t] = buf[(t >> 1) * 512 + ch * 128 + (half * 2 + (t & 1)) * 32 + r32];
#pragma unroll
                    for (int t = 0; t < NTT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch][0], b4[t].x, acc[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < NTT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch][1], b4[t].y, acc[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < NTT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch][2], b4[t].z, acc[t], 0, 0, 0);
#pragma unroll
                    for (int t = 0; t < NTT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch][3], b4[t].w, acc[t], 0, 0, 0);
                }
            }
        }
        float4 *nbuf = sB + ((st + 1) & 1) * kWideSlabF4;   // read last in stage st - 1: every wave is past this stage's barrier
        nbuf[tid] = b0; nbuf[tid + 256] = b1; nbuf[tid + 512] = b2; nbuf[tid + 768] = b3;
        cur = nxt;
    }
    // accumulators as they sit in the registers: [split][row block][wave][tile][16][64 lanes]
    float *dst = partial + ((((size_t)split * gridDim.x + blockIdx.x) * kWaves + wave) * NTT) * 1024 + lane;
#pragma unroll
    for (int t = 0; t < NTT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dst[(t * 16 + r) * 64] = acc[t][r];
}

template <int NTT>
__global__ __launch_bounds__(256) void spconv_wide_reduce_kernel(ConvParams p, int nsplit, const float *partial)
{
    // one 32-column tile per workgroup (blockIdx.y): 3-4 x the workgroups of a one-dimensional grid, which had 74 of them on
    // 256 CUs for the 9,415-row level; the BatchNorm summaries are per column, so nothing couples the tiles
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sStat = reinterpret_cast<float *>(smem);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int t = blockIdx.y;
    f32x16 acc[1];
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[0][r] = 0.0f;
    for (int s = 0; s < nsplit; ++s) {   // fixed order
        const float *src = partial + ((((size_t)s * gridDim.x + blockIdx.x) * kWaves + wave) * NTT) * 1024 + lane;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][r] += src[(t * 16 + r) * 64];
    }
    conv_epilogue<1>(p, acc, LinearRows{(int)blockIdx.x * kWideRows + wave * 32, p.n_out}, 32 * t, r32, half, wave, sStat,
                     (int)blockIdx.x, (int)gridDim.y);
}

size_t wide_workspace_bytes(const ConvParams &p)
{
    const int ntt = (p.Cout + 31) / 32;
    return (size_t)wide_splits(p.n_out) * (size_t)ceil_div(p.n_out, kWideRows) * kWaves * ntt * 1024 * sizeof(float);
}

// shape / alignment rule of the kernel pair, independent of the workspace (EPRECON_CONV_WIDEK=0 switches it off; per launch)
bool wide_shape_ok(const ConvParams &p)
{
    const char *e = getenv("EPRECON_CONV_WIDEK");
    if (e && e[0] == '0') return false;
    if (p.K != 27 || !p.nbr || !p.wq || (reinterpret_cast<uintptr_t>(p.wq) & 15) != 0) return false;
    if (p.Cin < 96 || p.Cin % 4 != 0 || p.Cout <= 64 || p.Cout > 128) return false;
    if (p.ld_x % 4 != 0 || (reinterpret_cast<uintptr_t>(p.x) & 15) != 0) return false;
    if (p.in_scale && ((reinterpret_cast<uintptr_t>(p.in_scale) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.in_shift) & 15) != 0))
        return false;
    if (p.accumulate || p.ln) return false;
    return p.n_out >= 4096 && p.n_out <= 40000;
}
bool wide_ok(const ConvParams &p) { return wide_shape_ok(p) && p.ws && p.ws_bytes >= wide_workspace_bytes(p); }

template <int NTT>
int launch_wide_t(const ConvParams &p, hipStream_t st)
{
    const int nsplit = wide_splits(p.n_out);
    const int blocks = (int)ceil_div(p.n_out, kWideRows);
    const int kmax = (p.K + nsplit - 1) / nsplit + 1;
    const size_t lds = (size_t)2 * kWideSlabF4 * sizeof(float4) + (size_t)kmax * kWideRows * sizeof(int) +
                       (size_t)2 * ((p.Cin + 3) & ~3) * sizeof(float) + 16;
    float *partial = reinterpret_cast<float *>(p.ws);
    hipLaunchKernelGGL((spconv_wide_kernel<NTT>), dim3((unsigned)blocks, (unsigned)nsplit), dim3(256), lds, st, p, nsplit, partial);
    EP_LAUNCH_CHECK();
    const size_t lds2 = (size_t)max(kWaves * 3 * 32 * NTT, 3 * 256) * sizeof(float);
    hipLaunchKernelGGL((spconv_wide_reduce_kernel<NTT>), dim3((unsigned)blocks, (unsigned)NTT), dim3(256), lds2, st, p, nsplit, (const float *)partial);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
int launch_wide(const ConvParams &p, hipStream_t st) { return (p.Cout + 31) / 32 == 3 ? launch_wide_t<3>(p, st) : launch_wide_t<4>(p, st); }

// short list + long (offset, slab) chain + a caller that can take 32-row BatchNorm summary blocks
bool splitk_ok(const ConvParams &p)
{
    const char *e = getenv("EPRECON_CONV_SPLITK");   // (per launch, like the other selection switches)
    if ((e && e[0] == '0') || p.accumulate) return false;
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

// One-shot timing hook for bench.py's `roofline_conv`: the next launch whose (K, Cin, Cout) match and whose list is
// at least min_rows long is bracketed by two events on the launch stream.
struct ConvProf {
    bool armed = false, recorded = false;
    int K = 0, cin = 0, cout = 0;
    int64_t min_rows = 0, rows = 0;
    const char *kernel = "";
    hipEvent_t start = nullptr, stop = nullptr;
    unsigned long long *pairs_dev = nullptr;  // [0] live (output row, offset) pairs of the bracketed launch, [1] the pairs it issues MFMAs for
} g_conv_prof;

// live pairs of a launch = what its algorithmic flop count rests on; counted on the launch stream BEHIND the stop event
__global__ void count_map_pairs_kernel(const int32_t *nbr, size_t total, unsigned long long *out)
{
    unsigned long long c = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) c += nbr[e] >= 0;
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
__global__ void count_grid_pairs_kernel(const int32_t *rank, int gx, int gy, int gz, unsigned long long *out)
{
    unsigned long long c = 0;
    const int total = gx * gy * gz;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        if (rank[e] < 0) continue;
        const int z = e % gz, y = (e / gz) % gy, x = e / (gz * gy);
        for (int k = 0; k < 27; ++k) {
            const int xx = x + k % 3 - 1, yy = y + (k / 3) % 3 - 1, zz = z + k / 9 - 1;
            if (xx >= 0 && xx < gx && yy >= 0 && yy < gy && zz >= 0 && zz < gz) c += rank[(xx * gy + yy) * gz + zz] >= 0;
        }
    }
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
// rows of the (32-row group, offset) pairs with at least one neighbour: what the direct kernel issues MFMAs for
__global__ void count_map_groups_kernel(const int32_t *nbr, int n, int K, unsigned long long *out)
{
    const int groups = (n + 31) / 32;
    unsigned long long c = 0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < K * groups; e += gridDim.x * blockDim.x) {
        const int k = e / groups, g = e - k * groups;
        const int rows = min(32, n - 32 * g);
        bool any = false;
        for (int i = 0; i < rows; ++i) any |= nbr[(size_t)k * n + 32 * g + i] >= 0;
        if (any) c += rows;
    }
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
const char *g_last_conv_kernel = "";

int conv_dispatch_inner(ConvParams &p, int64_t n_in, hipStream_t st);

int conv_dispatch(ConvParams &p, int64_t n_in, hipStream_t st)
{
    ConvProf &g = g_conv_prof;
    const bool hit = g.armed && p.K == g.K && p.Cin == g.cin && p.Cout == g.cout && p.n_out >= g.min_rows;
    // EPRECON_CONV_LOG=<file>: one line per launch (shape and the kernel that took it), in launch order, for joining with a
    // rocprofv3 kernel trace (tools/trace_cfg4_layers.py)
    static FILE *const layer_log = getenv("EPRECON_CONV_LOG") ? fopen(getenv("EPRECON_CONV_LOG"), "a") : nullptr;
    if (layer_log) {
        const int rc = conv_dispatch_inner(p, n_in, st);
        fprintf(layer_log, "%d %d %d %d %s ln=%d stats=%d acc=%d\n", p.n_out, p.K, p.Cin, p.Cout, g_last_conv_kernel, p.ln ? 1 : 0,
                p.bn_partial ? 1 : 0, p.accumulate ? 1 : 0);
        fflush(layer_log);
        return rc;
    }
    if (!hit) return conv_dispatch_inner(p, n_in, st);
    EP_HIP_CHECK(hipEventRecord(g.start, st));
    const int rc = conv_dispatch_inner(p, n_in, st);
    EP_HIP_CHECK(hipEventRecord(g.stop, st));
    g.armed = false;
    g.recorded = rc == EPRECON_OK;
    g.rows = p.n_out;
    g.kernel = g_last_conv_kernel;
    if (g.pairs_dev) {
        EP_HIP_CHECK(hipMemsetAsync(g.pairs_dev, 0, 2 * sizeof(unsigned long long), st));
        bool narrow;
        if (conv3d_tile_ok(p, &narrow))
            hipLaunchKernelGGL(count_grid_pairs_kernel, dim3(256), dim3(256), 0, st, p.vox_rank, p.gx, p.gy, p.gz, g.pairs_dev);
        else if (p.nbr) {
            hipLaunchKernelGGL(count_map_pairs_kernel, dim3(256), dim3(256), 0, st, p.nbr, (size_t)p.K * p.n_out, g.pairs_dev);
            if (!strcmp(g.kernel, "spconv_direct16_kernel"))
                hipLaunchKernelGGL(count_map_groups_kernel, dim3(256), dim3(256), 0, st, p.nbr, p.n_out, p.K, g.pairs_dev + 1);
        } else  // identity map
            EP_HIP_CHECK(hipMemcpyAsync(g.pairs_dev, &g.rows, sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        EP_LAUNCH_CHECK();
    }
    return rc;
}

int conv_dispatch_inner(ConvParams &p, int64_t n_in, hipStream_t st)
{
    {
        const int kind = conv3d_kind(p);
        if (kind != kD3None) {
            g_last_conv_kernel = kind == kD3Narrow ? "conv3d_tile_narrow_kernel" : "conv3d_tile16_kernel";
            return kind == kD3Tile16 ? launch_conv3d_16(p, st) : launch_conv3d_single_column(p, st);
        }
        if (!p.nbr && p.K != 1) return EPRECON_ERR_ARG;  // dense-grid form requested for a shape it does not take, no map given
    }
    // dense 2D 3x3 layers on long pixel lists: the 16-row image-tile kernel (sparse_conv_tile2d.hip; EPRECON_CONV_TILE2D16=0: off)
    if (tile2d16_ok(p)) {
        g_last_conv_kernel = "conv2d_tile16_kernel";
        return launch_tile2d16(p, st);
    }
    // ... and on short pixel lists: one 16-pixel tile per workgroup, the reduction split across its waves (sparse_conv_tile2d_short.hip;
    // EPRECON_CONV_TILE2D_SHORT=0: off)
    if (tile2d_short_ok(p)) {
        g_last_conv_kernel = "conv2d_tile_short_kernel";
        return launch_tile2d_short(p, st);
    }
    // dense 2D 3x3 layers whose caller packed the weights for it: the direct gather kernel on the pixel map (long lists: the wq16
    // packing of a short list is the short-list kernel's, which declined)
    const bool direct2d = p.K == 9 && direct16_ok(p) && !tile2d_short_list(p);
    if (!direct2d) {
        int nt, nch;
        int64_t blocks;
        if (conv2d_tile_ok(p, &nt, &nch, &blocks)) {
            g_last_conv_kernel = "conv2d_tile_kernel";
            switch (nch) {
                case 1: return launch_conv2d_tile<1>(p, st);
                case 2: return launch_conv2d_tile<2>(p, st);
                case 3: return launch_conv2d_tile<3>(p, st);
                case 4: return launch_conv2d_tile<4>(p, st);
                default: return launch_conv2d_tile<5>(p, st);
            }
        }
    }
    // 16-byte gathers need aligned rows; a channel count that is not a multiple of 4 is fine as long as the
    // row pitch covers the rounded-up count (the tail lanes are zeroed after the load)
    const bool vec4 = (p.ld_x % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.x) & 15) == 0) &&
                      (p.Cin % 4 == 0 || p.ld_x >= ((p.Cin + 3) & ~3));
    // Output columns per workgroup: all of them (<= 128) when the row tiles alone fill the chip,
    // 32-column blocks over blockIdx.y for short lists (10,800 pixels of the 1/16 maps are 85 row
    // tiles for 256 CUs; the gathered rows are re-read from L2 by each column block).
    const int nblk = (int)ceil_div(p.n_out, kRowsPerBlock);
    const int nt_full = (p.Cout + 31) / 32;
    if (p.ln && (nt_full > 4 || p.bn_partial || p.accumulate)) return EPRECON_ERR_UNSUPPORTED;
    if (wide_ok(p)) {
        g_last_conv_kernel = "spconv_wide_kernel";
        return launch_wide(p, st);
    }
    if (!direct2d && splitk_ok(p)) {
        g_last_conv_kernel = "spconv_splitk_kernel";
        return vec4 ? launch_splitk_v<true>(p, st) : launch_splitk_v<false>(p, st);
    }
    if (direct16_ok(p) && !tile2d_short_list(p)) {
        g_last_conv_kernel = "spconv_direct16_kernel";
        return launch_direct16(p, st);
    }
    const bool split = nblk < 256 && nt_full > 1 && !p.ln;
    const int cin_pad = (p.Cin + 7) / 8 * 8;
    // narrow layers: the weights of a group of offsets resident in LDS
    if (cin_pad <= 64 && (p.Cout <= 64 || split)) {
        g_last_conv_kernel = "spconv_resident_kernel";
        return (nt_full == 1 || split) ? launch_resident<1>(p, vec4, cin_pad, st) : launch_resident<2>(p, vec4, cin_pad, st);
    }
    // wide inputs (C_in > 64) on the same pipelined kernel, walked in slabs of <= 64 channels.  Columns: 64 per workgroup
    // when the row tiles alone fill the chip, else 32.
    // (3D kernel maps only: the dense 2D layers, K = 1 / 9 on 10,800..43,200 pixel rows, measured faster on the slab kernel)
    if (cin_pad > 64 && vec4 && (p.K == 27 || p.K == 8) && !(p.ln && nt_full > 2)) {
        g_last_conv_kernel = "spconv_resident_kernel(wide)";
        const bool two = nt_full >= 2 && (p.ln || (int64_t)nblk * ((nt_full + 1) / 2) >= 256);
        return two ? launch_resident<2>(p, vec4, cin_pad, st) : launch_resident<1>(p, vec4, cin_pad, st);
    }
    g_last_conv_kernel = "spconv_mfma_kernel";
    if (nt_full == 1 || split) return launch_conv<1>(p, vec4, st);
    if (nt_full == 2) return launch_conv<2>(p, vec4, st);
    if (nt_full == 3) return launch_conv<3>(p, vec4, st);
    return launch_conv<4>(p, vec4, st);  // Cout > 128: 128-column blocks over blockIdx.y
}

}  // namespace

// stage marker for kernel traces: an empty launch whose grid size carries the id
__global__ void profile_mark_kernel() {}
extern "C" int eprecon_profile_mark_async(int id, void *stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(profile_mark_kernel, dim3((unsigned)id + 1), dim3(64), 0, st);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" int eprecon_profile_conv_arm(int kvol, int cin, int cout, int64_t min_rows)
{
    ConvProf &g = g_conv_prof;
    if (!g.start) {
        EP_HIP_CHECK(hipEventCreate(&g.start));
        EP_HIP_CHECK(hipEventCreate(&g.stop));
        EP_HIP_CHECK(hipMalloc(&g.pairs_dev, 2 * sizeof(unsigned long long)));
    }
    g.K = kvol; g.cin = cin; g.cout = cout; g.min_rows = min_rows;
    g.armed = true;
    g.recorded = false;
    return EPRECON_OK;
}

extern "C" float eprecon_profile_conv_ms(int64_t *rows_out, const char **kernel_out)
{
    ConvProf &g = g_conv_prof;
    if (!g.recorded || hipEventSynchronize(g.stop) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, g.start, g.stop) != hipSuccess) return -1.0f;
    if (rows_out) *rows_out = g.rows;
    if (kernel_out) *kernel_out = g.kernel;
    return ms;
}

extern "C" const char *eprecon_profile_last_conv_kernel(void) { return g_last_conv_kernel; }

extern "C" int64_t eprecon_profile_conv_pairs(void)
{
    ConvProf &g = g_conv_prof;
    if (!g.recorded || !g.pairs_dev || hipEventSynchronize(g.stop) != hipSuccess) return -1;
    unsigned long long v = 0;
    if (hipMemcpy(&v, g.pairs_dev, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

extern "C" int64_t eprecon_profile_conv_executed_pairs(void)
{
    ConvProf &g = g_conv_prof;
    if (!g.recorded || !g.pairs_dev || hipEventSynchronize(g.stop) != hipSuccess) return -1;
    unsigned long long v = 0;
    if (hipMemcpy(&v, g.pairs_dev + 1, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;   // 0: the kernel that took the launch walks every offset of every row
}

extern "C" size_t eprecon_conv_pack_weight_floats(int kvol, int cin, int cout)
{
    if (kvol <= 0 || cin <= 0 || cout <= 0) return 0;
    int nt, ncb;
    d3_columns(cout, &nt, &ncb);
    return (size_t)ncb * kvol * ((cin + 7) / 8) * 2 * nt * 32 * 4;
}

extern "C" int eprecon_conv_pack_weight_async(const float *weight, int kvol, int cin, int cout, float *packed, void *stream)
{
    if (!weight || !packed || kvol <= 0 || cin <= 0 || cout <= 0) return EPRECON_ERR_ARG;
    int nt, ncb;
    d3_columns(cout, &nt, &ncb);
    const size_t total = eprecon_conv_pack_weight_floats(kvol, cin, cout);
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)min((size_t)1024, (total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       weight, kvol, cin, cout, (cin + 7) / 8, nt, ncb, packed);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" size_t eprecon_conv_pack_weight16_floats(int kvol, int cin, int cout)
{
    if (kvol <= 0 || cin <= 0 || cout <= 0 || cout > 80) return 0;
    const int rem = cout - 16 * ((cout + 15) / 16 - 1);      // columns of the last tile: <= 8 -> the tail section follows the tiles
    return (size_t)kvol * ((cin + 15) / 16) * ((cout + 15) / 16) * 256 + (rem <= 8 ? (size_t)kvol * ((cin + 15) / 16) * 128 : 0);
}

extern "C" int eprecon_conv_pack_weight16_async(const float *weight, int kvol, int cin, int cout, float *packed, void *stream)
{
    if (!weight || !packed || kvol <= 0 || cin <= 0 || cout <= 0 || cout > 80) return EPRECON_ERR_ARG;
    const size_t total = eprecon_conv_pack_weight16_floats(kvol, cin, cout);
    hipLaunchKernelGGL(pack_weights16_kernel, dim3((unsigned)min((size_t)1024, (total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       weight, kvol, cin, cout, (cin + 15) / 16, (cout + 15) / 16, packed);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" int eprecon_conv_pack_many_async(const eprecon_pack_job *jobs_dev, int njobs, void *stream)
{
    if (njobs < 0 || (njobs > 0 && !jobs_dev) || njobs > 65535) return EPRECON_ERR_ARG;
    if (njobs == 0) return EPRECON_OK;
    hipLaunchKernelGGL(pack_many_kernel, dim3(32, (unsigned)njobs), dim3(256), 0, (hipStream_t)stream, jobs_dev);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" size_t eprecon_conv_bn_partial_bytes(int64_t n_out, int cout)
{
    return (size_t)ep::ceil_div(n_out > 0 ? n_out : 1, (int64_t)128) * 3 * (size_t)(cout > 0 ? cout : 1) * sizeof(float);
}

static int conv_check_and_run(ConvParams &p, int64_t n_in, int64_t n_out, void *stream)
{
    if (!p.x || !p.w || !p.out || n_in < 0 || n_out < 0 || p.K <= 0 || p.K > 64 || p.Cin <= 0 || p.Cout <= 0 ||
        p.ld_x < p.Cin || p.ld_out < p.Cout || (p.res && p.ld_res < p.Cout))
        return EPRECON_ERR_ARG;
    if (!p.nbr && !p.vox_rank && p.K != 1) return EPRECON_ERR_ARG;
    if (!p.nbr && n_in != n_out) return EPRECON_ERR_ARG;
    if ((p.in_scale == nullptr) != (p.in_shift == nullptr) || (p.res_scale == nullptr) != (p.res_shift == nullptr))
        return EPRECON_ERR_ARG;
    if (p.Cout > 4096 || n_out > 0x7fffffff) return EPRECON_ERR_UNSUPPORTED;
    if (n_out == 0) return EPRECON_OK;
    p.n_out = (int)n_out;
    p.x_bytes = n_in > 0 ? ((n_in - 1) * (int64_t)p.ld_x + ((p.Cin + 3) & ~3)) * 4 : 0;
    return conv_dispatch(p, n_in, (hipStream_t)stream);
}

// Descriptor form of the gather-GEMM (include/eprecon_hip.h: eprecon_conv_desc): every fused prologue /
// epilogue of the convolution blocks of the reference in one launch.
static void params_from_desc(ConvParams &p, const eprecon_conv_desc *d)
{
    p.x = d->x; p.nbr = d->nbr; p.w = d->weight; p.bias = d->bias; p.out = d->out;
    p.K = d->kvol; p.Cin = d->cin; p.Cout = d->cout; p.ld_x = d->ld_x; p.ld_out = d->ld_out;
    p.relu = d->relu; p.accumulate = d->accumulate;
    p.res = d->residual; p.ld_res = d->ld_res; p.bn_partial = d->bn_partial; p.bn_ld = d->bn_ld;
    p.in_scale = d->in_scale; p.in_shift = d->in_shift; p.in_relu = d->in_relu;
    p.res_scale = d->res_scale; p.res_shift = d->res_shift; p.res_relu = d->res_relu;
    p.ln = d->ln; p.ln_gamma = d->ln_gamma; p.ln_beta = d->ln_beta; p.ln_eps = d->ln_eps;
    p.ln_post_relu = d->ln_post_relu;
    p.img_h = d->img_h; p.img_w = d->img_w; p.img_maps = d->img_maps;
    p.vox_rank = d->vox_rank; p.gx = d->grid_x; p.gy = d->grid_y; p.gz = d->grid_z; p.wq = d->packed_weight;
    p.wq16 = d->packed_weight16;
    p.ws = d->workspace; p.ws_bytes = d->workspace_bytes;
    p.flex_partial = 1;
    p.bn_acc = d->bn_acc; p.bn_acc_ld = d->bn_acc_ld; p.bn_acc_c0 = d->bn_acc_c0; p.bn_gamma = d->bn_gamma; p.bn_beta = d->bn_beta;
    p.in_acc = d->in_acc; p.in_acc_ld = d->in_acc_ld; p.in_acc_c0 = d->in_acc_c0; p.in_eps = d->in_eps;
}

extern "C" int eprecon_batchnorm_acc_affine_async(const long long *acc, int acc_ld, int acc_c0, int channels, float eps,
                                                  float *scale_out, float *shift_out, void *stream);

// BatchNorm form (c) — which launches take part.  PRODUCER: every kernel whose summaries go through conv_epilogue or
// direct_epilogue (all gather forms and the 2D image-tile kernel); the dense-grid 3D tile kernels keep their own epilogues.
// CONSUMER: the same families finish the accumulators in their prologue; for the others the library queues the stand-alone
// finish (one launch, like the finalize it replaces) into the caller's in_affine_scratch.
static bool bn_acc_family(const ConvParams &p) { return conv3d_kind(p) == 0; }

extern "C" size_t eprecon_bn_acc_words(int ld)
{
    return ld > 0 ? (size_t)epconv::kBnCopies * ld * epconv::kBnWords + (size_t)(2 * ld + 1) / 2 : 0;
}

extern "C" int eprecon_conv_desc_takes_bn_acc(const eprecon_conv_desc *d)
{
    if (!d || d->n_out <= 0) return 0;
    ConvParams p = {};
    params_from_desc(p, d);
    p.n_out = (int)d->n_out;
    return !p.ln && !p.accumulate && bn_acc_family(p) ? 1 : 0;
}

extern "C" int64_t eprecon_conv_desc_partial_rows(const eprecon_conv_desc *d);

extern "C" int eprecon_conv_desc_async(const eprecon_conv_desc *d, void *stream)
{
    if (!d) return EPRECON_ERR_ARG;
    ConvParams p = {};
    params_from_desc(p, d);
    p.n_out = (int)(d->n_out > 0 && d->n_out <= 0x7fffffff ? d->n_out : 0);
    if (p.bn_partial) {     // row stride of the channel-major summaries: at least the rows this launch writes
        const int64_t rows = eprecon_conv_desc_partial_rows(d);
        if (p.bn_ld == 0) p.bn_ld = (int)(rows > 0 ? rows : 1);
        if (p.bn_ld < rows) return EPRECON_ERR_ARG;
    }
    if (p.bn_acc && (p.bn_acc_ld <= 0 || p.bn_acc_c0 < 0 || p.bn_acc_c0 + p.Cout > p.bn_acc_ld || p.ln || p.accumulate || !bn_acc_family(p)))
        return EPRECON_ERR_ARG;        // (ask eprecon_conv_desc_takes_bn_acc first)
    if (p.in_acc) {
        if (p.in_scale || p.in_shift || p.in_acc_ld <= 0 || p.in_acc_c0 < 0 || p.in_acc_c0 + p.Cin > p.in_acc_ld) return EPRECON_ERR_ARG;
        if (bn_acc_family(p)) {
            // (the kernels test in_scale for "there is a pending BatchNorm": any non-null value; stage_in_affine reads in_acc)
            p.in_scale = p.in_shift = reinterpret_cast<const float *>(p.in_acc);
        } else {
            if (!d->in_affine_scratch) return EPRECON_ERR_ARG;
            const int rc = eprecon_batchnorm_acc_affine_async(p.in_acc, p.in_acc_ld, p.in_acc_c0, p.Cin, p.in_eps, d->in_affine_scratch,
                                                              d->in_affine_scratch + p.Cin, stream);
            if (rc != EPRECON_OK) return rc;
            p.in_scale = d->in_affine_scratch;
            p.in_shift = d->in_affine_scratch + p.Cin;
            p.in_acc = nullptr;
        }
    }
    return conv_check_and_run(p, d->n_in, d->n_out, stream);
}

extern "C" size_t eprecon_conv_desc_workspace_bytes(const eprecon_conv_desc *d)
{
    if (!d || d->n_out <= 0 || d->n_out > 0x7fffffff) return 0;
    ConvParams p = {};
    params_from_desc(p, d);
    p.n_out = (int)d->n_out;
    return wide_shape_ok(p) ? wide_workspace_bytes(p) : 0;
}

// rows of bn_partial the launch described by `d` writes (= the nblk to hand to
// eprecon_batchnorm_finalize_affine_async): 128-row blocks for the gather forms, image tiles for the
// dense 2D tile kernels
extern "C" int64_t eprecon_conv_desc_partial_rows(const eprecon_conv_desc *d)
{
    if (!d || d->n_out <= 0) return 0;
    ConvParams p = {};
    params_from_desc(p, d);
    p.n_out = (int)d->n_out;
    int nt, nch;
    int64_t blocks;
    if (const int kind = conv3d_kind(p)) return d3_tiles_kind(p, kind);
    p.x_bytes = d->n_in > 0 ? ((d->n_in - 1) * (int64_t)p.ld_x + ((p.Cin + 3) & ~3)) * 4 : 0;
    if (tile2d16_ok(p)) return tile2d16_partial_rows(p);
    if (tile2d_short_ok(p)) return tile2d_short_partial_rows(p);
    if (p.K == 9 && direct16_ok(p) && !tile2d_short_list(p)) return ep::ceil_div(d->n_out, (int64_t)direct16_partial_block_rows(p));
    if (conv2d_tile_ok(p, &nt, &nch, &blocks)) return blocks;
    if (wide_ok(p)) return ep::ceil_div(d->n_out, (int64_t)kWideRows);
    if (splitk_ok(p)) return ep::ceil_div(d->n_out, (int64_t)32);
    if (direct16_ok(p) && !tile2d_short_list(p)) return ep::ceil_div(d->n_out, (int64_t)direct16_partial_block_rows(p));
    return ep::ceil_div(d->n_out, (int64_t)kRowsPerBlock);
}

// out = [ReLU]( sum_k x[nbr[k]] @ W[k] + bias [+ out] ) [+ residual]; optionally the per-workgroup
// BatchNorm summaries of the stored values (see conv_epilogue) -> bn_partial, to be consumed by
// eprecon_batchnorm_apply_partials_async.
extern "C" int eprecon_sparse_conv_fused_async(const float *x, int64_t n_in, int ld_x, const int32_t *nbr,
                                               int kvol, int64_t n_out, const float *weight, int cin,
                                               int cout, const float *bias, const float *residual,
                                               int ld_res, float *out, int ld_out, int relu,
                                               int accumulate, float *bn_partial, void *stream)
{
    ConvParams p = {};
    p.x = x; p.nbr = nbr; p.w = weight; p.bias = bias; p.out = out;
    p.K = kvol; p.Cin = cin; p.Cout = cout; p.ld_x = ld_x; p.ld_out = ld_out;
    p.relu = relu; p.accumulate = accumulate;
    p.res = residual; p.ld_res = ld_res; p.bn_partial = bn_partial;
    p.bn_ld = (int)ep::ceil_div(n_out > 0 ? n_out : 1, (int64_t)kRowsPerBlock);   // (no flex_partial: 128-row blocks only)
    return conv_check_and_run(p, n_in, n_out, stream);
}

extern "C" int eprecon_sparse_conv_async(const float *x, int64_t n_in, int ld_x, const int32_t *nbr,
                                         int kvol, int64_t n_out, const float *weight, int cin,
                                         int cout, const float *bias, float *out, int ld_out,
                                         int relu, int accumulate, void *stream)
{
    return eprecon_sparse_conv_fused_async(x, n_in, ld_x, nbr, kvol, n_out, weight, cin, cout, bias, nullptr, 0,
                                           out, ld_out, relu, accumulate, nullptr, stream);
}
