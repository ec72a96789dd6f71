// Device code shared by the gather-GEMM kernels on v_mfma_f32_32x32x2_f32 (sparse_conv_slab.hip, sparse_conv_resident_impl.hpp,
// sparse_conv_splitk.hip, sparse_conv_wide.hip): weight staging into LDS, the row gathers, and the shared epilogue (bias, ReLU,
// residual, BatchNorm summaries or row-wise LayerNorm).
#pragma once
#include "common.hpp"
#include "conv_common.hpp"

namespace epconv {

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

}  // namespace epconv
