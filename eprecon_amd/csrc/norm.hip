// Normalisation epilogues of the sparse layers for gfx950: batch-statistic BatchNorm over all active
// voxels (the reference runs in train mode at test time, main.py:357, so the statistics cannot be
// folded into the weights) and row-wise LayerNorm with the ReLU / residual patterns the reference
// wires around its spconv layers.
//
// Replaces  spnn.BatchNorm / nn.BatchNorm1d (train mode)   models/modules.py:22,41,54,60,65,134,139
//                                                          models/occupancy_initialization.py:29,37
//           nn.LayerNorm + ReLU + residual epilogues       models/modules.py:447-452,473-482
//                                                          models/occupancy_initialization.py:141-169
// Bandwidth-bound column / row reductions; deterministic (fixed-order Chan merges, no float atomics).
#include <stdlib.h>

#include <type_traits>

#include "common.hpp"
#include "conv_common.hpp"

namespace {
using namespace ep;
using epconv::chan_merge;  // the producers' summaries and the finalize merge with the same function

constexpr int kBnPerThread = 8;  // rows each thread of the statistics kernel keeps in registers

// One pass over x: block b summarises rows [b*R, (b+1)*R) with R = kBnPerThread * (256 / C); every
// thread owns one column and <= 8 rows held in registers (two-pass mean / M2 on those, no
// cancellation), then the (256/C) row groups are merged through LDS in fixed order.
// Channel-major like the convolution epilogues (conv_common.hpp, bn_partial_store): partial[(q * C + c) * nblk + b], q = 0
// count, 1 mean, 2 M2, nblk = gridDim.x.
__global__ __launch_bounds__(256) void bn_stats_kernel(const float *x, int n, int C, int ld, float *partial)
{
    __shared__ float sN[256], sMean[256], sM2[256];
    const int tid = threadIdx.x;
    const int rpi = 256 / C;
    const int col = tid % C, rsub = tid / C;
    const bool active = rsub < rpi;
    const int r0 = blockIdx.x * (kBnPerThread * rpi);
    float v[kBnPerThread];
    float cnt = 0.0f, sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kBnPerThread; ++k) {
        const int r = r0 + k * rpi + rsub;
        const bool ok = active && r < n;
        v[k] = ok ? x[(size_t)r * ld + col] : 0.0f;
        cnt += ok ? 1.0f : 0.0f;
        sum += v[k];
    }
    const float mean = cnt > 0.0f ? sum / cnt : 0.0f;
    float m2 = 0.0f;
#pragma unroll
    for (int k = 0; k < kBnPerThread; ++k) {
        const int r = r0 + k * rpi + rsub;
        if (active && r < n) {
            const float d = v[k] - mean;
            m2 = fmaf(d, d, m2);
        }
    }
    sN[tid] = cnt; sMean[tid] = mean; sM2[tid] = m2;
    __syncthreads();
    // fixed-order pairwise tree over the rpi row groups (a serial merge by one thread per column cost
    // 44 us on the single-channel BatchNorm of the occupancy logit: 256 dependent merges with divisions)
    for (int s = 1; s < rpi; s <<= 1) {
        if (active && (rsub % (2 * s)) == 0 && rsub + s < rpi) {
            float n = sN[tid], m = sMean[tid], q = sM2[tid];
            const int o = tid + s * C;
            chan_merge(n, m, q, sN[o], sMean[o], sM2[o]);
            sN[tid] = n; sMean[tid] = m; sM2[tid] = q;
        }
        __syncthreads();
    }
    if (tid < C) {
        const size_t plane = (size_t)C * gridDim.x;
        float *p = partial + (size_t)tid * gridDim.x + blockIdx.x;
        p[0] = sN[tid]; p[plane] = sMean[tid]; p[2 * plane] = sM2[tid];
    }
}

// Thread t's part of the merge of channel c's summaries (channel-major, partial[(q * C + c) * ld + b]): rows t, t + 256, ...
// in order.  The rows of one loop trip — NU per thread, NU * 256 in all — are all loaded before the first is merged: the chain
// of load latencies is what these launches cost.  Each workgroup reads three contiguous runs of nblk floats (a row-major
// [nblk][3][C] list cost one 64-byte segment per float: 3 nblk segments through one CU).  Rows past nblk load as
// empty summaries, which the merge skips, so NU changes the cost and not the result; bn_finalize_nu picks it.
template <int NU>
__device__ __forceinline__ void bn_merge_rows(const float *partial, int nblk, int64_t ld, int C, int c, int tid, float &a_n,
                                              float &a_mean, float &a_m2)
{
    const float *pn = partial + (size_t)c * ld, *pm = pn + (size_t)C * ld, *pq = pm + (size_t)C * ld;
    for (int b = tid; b < nblk; b += NU * 256) {
        float vn[NU], vm[NU], vq[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int bb = b + u * 256;
            const bool ok = bb < nblk;
            vn[u] = ok ? pn[bb] : 0.0f;
            vm[u] = ok ? pm[bb] : 0.0f;
            vq[u] = ok ? pq[bb] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) chan_merge(a_n, a_mean, a_m2, vn[u], vm[u], vq[u]);
    }
}

// rows per thread and loop trip: the smallest of 1, 2, 4, 8, 16 that takes the list in one trip (16: registers, then a loop).
// Empty loads and merges are not free: with NU = 16 fixed, a list of 85 rows took 4.9 us against 3.2 us (profiles/r08).
inline int bn_finalize_nu(int64_t nblk)
{
    const int64_t need = (nblk + 255) / 256;
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
}

// ... as a compile-time NU: launch(std::integral_constant<int, NU>) picks the instantiation of a kernel template
template <class Launch>
void with_finalize_nu(int64_t nblk, Launch launch)
{
    switch (bn_finalize_nu(nblk)) {
    case 1: launch(std::integral_constant<int, 1>()); break;
    case 2: launch(std::integral_constant<int, 2>()); break;
    case 4: launch(std::integral_constant<int, 4>()); break;
    case 8: launch(std::integral_constant<int, 8>()); break;
    default: launch(std::integral_constant<int, 16>()); break;
    }
}

// one workgroup per channel: thread t merges partials t, t+256, ... in order, then a fixed LDS tree
template <int NU>
__global__ __launch_bounds__(256) void bn_finalize_kernel(const float *partial, int nblk, int64_t ld, int C, float *mean_out,
                                                          float *var_out)
{
    __shared__ float sN[256], sMean[256], sM2[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
    bn_merge_rows<NU>(partial, nblk, ld, C, c, tid, a_n, a_mean, a_m2);
    sN[tid] = a_n; sMean[tid] = a_mean; sM2[tid] = a_m2;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            float n = sN[tid], m = sMean[tid], q = sM2[tid];
            chan_merge(n, m, q, sN[tid + s], sMean[tid + s], sM2[tid + s]);
            sN[tid] = n; sMean[tid] = m; sM2[tid] = q;
        }
        __syncthreads();
    }
    if (tid == 0) {
        mean_out[c] = sMean[0];
        var_out[c] = sN[0] > 0.0f ? sM2[0] / sN[0] : 0.0f;  // biased variance
    }
}

// the same merge, published in affine form: y = x * scale + shift  ==  (x - mean) / sqrt(var + eps) * gamma + beta
template <int NU>
__global__ __launch_bounds__(256) void bn_finalize_affine_kernel(const float *partial, int nblk, int64_t ld, int C,
                                                                 const float *gamma, const float *beta, float eps,
                                                                 float *scale_out, float *shift_out)
{
    // one workgroup per channel; fixed merge order: thread t takes rows t, t + 256, ...; lanes merge by
    // xor-shuffles (lower lane first), the four wave results in wave order -- one barrier in total
    __shared__ float sN[4], sMean[4], sM2[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    // (gamma / beta travel with the first summaries instead of behind the merge: one memory round trip less on a launch that
    // is nothing but round trips — 37 of these sit between the layers of a cfg2 step)
    const float g_c = gamma ? gamma[c] : 1.0f, b_c = beta ? beta[c] : 0.0f;
    float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
    bn_merge_rows<NU>(partial, nblk, ld, C, c, tid, a_n, a_mean, a_m2);
    const int lane = tid & 63;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float on = __shfl_xor(a_n, m), om = __shfl_xor(a_mean, m), oq = __shfl_xor(a_m2, m);
        // both partners compute the same (lower, upper) merge, so every lane ends with the same value
        float ln = (lane & m) ? on : a_n, lm = (lane & m) ? om : a_mean, lq = (lane & m) ? oq : a_m2;
        chan_merge(ln, lm, lq, (lane & m) ? a_n : on, (lane & m) ? a_mean : om, (lane & m) ? a_m2 : oq);
        a_n = ln; a_mean = lm; a_m2 = lq;
    }
    if (lane == 0) { sN[tid >> 6] = a_n; sMean[tid >> 6] = a_mean; sM2[tid >> 6] = a_m2; }
    __syncthreads();
    if (tid == 0) {
        float n = sN[0], mean = sMean[0], m2 = sM2[0];
        for (int w = 1; w < 4; ++w) chan_merge(n, mean, m2, sN[w], sMean[w], sM2[w]);
        const float var = n > 0.0f ? m2 / n : 0.0f;  // biased variance
        const float sc = g_c / sqrtf(var + eps);
        scale_out[c] = sc;
        shift_out[c] = b_c - mean * sc;
    }
}

// THE apply expression, element (r, c): (x - mean) * inv * gamma + beta [+ res (* res_scale + res_shift)] [relu].  The two-launch
// and the one-launch form (bn_apply_kernel, bn_merge_apply_kernel) give the same bits because both evaluate this.
// res_scale / res_shift (optional): the residual operand carries a pending BatchNorm of its own in affine form (the 1x1 skip
// convolution of a residual block, models/modules.py:57-65), applied on load.  (Plain arguments: with the launch-wide operands
// handed to the kernels as one struct the apply launch of 93,512 x 32 rows took 0.3 us more, profiles/r27.)
__device__ __forceinline__ float bn_apply_value(const float *x, int ld_x, int r, int c, const float *mean, const float *var,
                                                const float *gamma, const float *beta, float eps, const float *res, int ld_res,
                                                const float *res_scale, const float *res_shift, int relu)
{
    const float inv = 1.0f / sqrtf(var[c] + eps);
    float v = (x[(size_t)r * ld_x + c] - mean[c]) * inv;
    v = v * (gamma ? gamma[c] : 1.0f) + (beta ? beta[c] : 0.0f);
    if (res) {
        float rv = res[(size_t)r * ld_res + c];
        if (res_scale) rv = fmaf(rv, res_scale[c], res_shift[c]);
        v += rv;
    }
    if (relu) v = fmaxf(v, 0.0f);
    return v;
}

__global__ __launch_bounds__(256) void bn_apply_kernel(const float *x, int n, int C, int ld_x,
                                                       const float *mean, const float *var,
                                                       const float *gamma, const float *beta, float eps,
                                                       const float *res, int ld_res, const float *res_scale,
                                                       const float *res_shift, int relu, float *out, int ld_out)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * C) return;
    const int r = (int)(e / C), c = (int)(e - (size_t)r * C);
    out[(size_t)r * ld_out + c] = bn_apply_value(x, ld_x, r, c, mean, var, gamma, beta, eps, res, ld_res, res_scale, res_shift, relu);
}

// LayerNorm over the C channels of each row: t = x; [relu]; [+ res]; LN(t) * g + b; [relu]
// 8 lanes per row, lane g owns channels g, g+8, ...
__global__ __launch_bounds__(256) void rowwise_ln_kernel(const float *x, int n, int C, int ld_x,
                                                         const float *res, int ld_res,
                                                         const float *gamma, const float *beta, float eps,
                                                         int pre_relu, int post_relu, float *out,
                                                         int ld_out)
{
    const int g = threadIdx.x & 7;
    const int r = blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool live = r < n;
    const float *xr = x + (size_t)(live ? r : 0) * ld_x;
    const float *rr = res ? res + (size_t)(live ? r : 0) * ld_res : nullptr;
    auto value = [&](int c) -> float {
        float v = xr[c];
        if (pre_relu) v = fmaxf(v, 0.0f);
        if (rr) v += rr[c];
        return v;
    };
    float s = 0.0f;
    if (live)
        for (int c = g; c < C; c += 8) s += value(c);
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    const float mean = s / (float)C;
    float q = 0.0f;
    if (live)
        for (int c = g; c < C; c += 8) {
            const float d = value(c) - mean;
            q = fmaf(d, d, q);
        }
    q += __shfl_xor(q, 1);
    q += __shfl_xor(q, 2);
    q += __shfl_xor(q, 4);
    const float inv = 1.0f / sqrtf(q / (float)C + eps);
    if (live)
        for (int c = g; c < C; c += 8) {
            float v = (value(c) - mean) * inv * (gamma ? gamma[c] : 1.0f) + (beta ? beta[c] : 0.0f);
            if (post_relu) v = fmaxf(v, 0.0f);
            out[(size_t)r * ld_out + c] = v;
        }
}

// out = [relu]( x * scale + shift [+ res] ): a BatchNorm its producer finished.  RES is decided by the host: with a test of the
// pointer in the kernel, the launch without a residual (dense2d.materialize, 172,800 x 24) took 9.3 - 9.4 us against 8.8 - 9.0.
// res / ld_res come last, so that the instantiation without them finds every argument it reads where it would without them
template <bool RES>
__global__ __launch_bounds__(256) void affine_rows_kernel(const float *x, int n, int C, int ld_x, const float *scale,
                                                          const float *shift, int relu, float *out, int ld_out,
                                                          const float *res, int ld_res)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * C) return;
    const int r = (int)(e / C), c = (int)(e - (size_t)r * C);
    float v = fmaf(x[(size_t)r * ld_x + c], scale[c], shift[c]);
    if constexpr (RES) v += res[(size_t)r * ld_res + c];
    if (relu) v = fmaxf(v, 0.0f);
    out[(size_t)r * ld_out + c] = v;
}

// The two joins of the 2D fusion stack (Occupancy_Initialization.feat_fusion_pre): the outer levels reach the 1/8 grid through a
// 2x2 mean (1/4 level) or a bilinear x2 (1/16 level) and land in their channel slice of the concat buffer.  One launch each from
// the level's raw rows and its pending BatchNorm, instead of affine_rows -> a resampling launch -> a strided copy with two
// intermediate tensors: t = [relu](x * scale + shift) is formed on load (affine_rows_kernel's expression), then
//   pool   (((0 + t00) + t01) + t10) + t11) / 4: the sum in (kh, kw) order from zero, then the divide, as the library's
//          average pooling of a channels-last tensor does it; odd heights / widths drop their last row / column
//   up     upsample2x_nhwc_kernel's taps, weights and sum (csrc/grid_ops.hip)
// VEC = 4: four channels per thread where C, the strides and the pointers allow 16-byte accesses; else one.
template <int VEC>
__device__ __forceinline__ void load_affine(const float *x, const float *scale, const float *shift, int relu, float (&t)[VEC])
{
    if constexpr (VEC == 4) {
        const float4 v = *reinterpret_cast<const float4 *>(x);
        t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
    } else {
        t[0] = x[0];
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
        t[k] = fmaf(t[k], scale[k], shift[k]);
        if (relu) t[k] = fmaxf(t[k], 0.0f);
    }
}

template <int VEC>
__device__ __forceinline__ void store_vec(float *dst, const float (&o)[VEC])
{
    if constexpr (VEC == 4) *reinterpret_cast<float4 *>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    else dst[0] = o[0];
}

template <int VEC>
__global__ __launch_bounds__(256) void affine_pool2_rows_kernel(const float *x, int maps, int h, int w, int C, int ld_x,
                                                                const float *scale, const float *shift, int relu, float *out,
                                                                int ld_out)
{
    const int cv = C / VEC, oh = h / 2, ow = w / 2;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)maps * oh * ow * cv) return;
    const int c = (int)(e % cv) * VEC;
    const size_t orow = e / cv;
    const int ox = (int)(orow % ow), oy = (int)((orow / ow) % oh), img = (int)(orow / ow / oh);
    const float *p = x + (((size_t)img * h + 2 * oy) * w + 2 * ox) * ld_x + c;
    float t00[VEC], t01[VEC], t10[VEC], t11[VEC], o[VEC];
    load_affine<VEC>(p, scale + c, shift + c, relu, t00);
    load_affine<VEC>(p + ld_x, scale + c, shift + c, relu, t01);
    load_affine<VEC>(p + (size_t)w * ld_x, scale + c, shift + c, relu, t10);
    load_affine<VEC>(p + (size_t)(w + 1) * ld_x, scale + c, shift + c, relu, t11);
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = ((((0.0f + t00[k]) + t01[k]) + t10[k]) + t11[k]) / 4.0f;
    store_vec<VEC>(out + orow * ld_out + c, o);
}

template <int VEC>
__global__ __launch_bounds__(256) void affine_up2_rows_kernel(const float *x, int maps, int h, int w, int C, int ld_x,
                                                              const float *scale, const float *shift, int relu, float *out,
                                                              int ld_out)
{
    const int cv = C / VEC;
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)maps * 4 * h * w * cv) return;
    const int c = (int)(e % cv) * VEC;
    const size_t orow = e / cv;
    const int ox = (int)(orow % (2 * w)), oy = (int)((orow / (2 * w)) % (2 * h)), img = (int)(orow / (2 * w) / (2 * h));
    const float sx = fmaxf(((float)ox + 0.5f) * 0.5f - 0.5f, 0.0f);
    const float sy = fmaxf(((float)oy + 0.5f) * 0.5f - 0.5f, 0.0f);
    const int x0 = (int)sx, y0 = (int)sy;
    const int x1 = min(x0 + 1, w - 1), y1 = min(y0 + 1, h - 1);
    const float lx = sx - (float)x0, ly = sy - (float)y0;
    const float *base = x + (size_t)img * h * w * ld_x + c;
    float a[VEC], b[VEC], d[VEC], f[VEC], o[VEC];
    load_affine<VEC>(base + ((size_t)y0 * w + x0) * ld_x, scale + c, shift + c, relu, a);
    load_affine<VEC>(base + ((size_t)y0 * w + x1) * ld_x, scale + c, shift + c, relu, b);
    load_affine<VEC>(base + ((size_t)y1 * w + x0) * ld_x, scale + c, shift + c, relu, d);
    load_affine<VEC>(base + ((size_t)y1 * w + x1) * ld_x, scale + c, shift + c, relu, f);
    const float w00 = (1.0f - ly) * (1.0f - lx), w01 = (1.0f - ly) * lx, w10 = ly * (1.0f - lx), w11 = ly * lx;
#pragma unroll
    for (int k = 0; k < VEC; ++k) o[k] = w00 * a[k] + w01 * b[k] + w10 * d[k] + w11 * f[k];
    store_vec<VEC>(out + orow * ld_out + c, o);
}

// BatchNorm form (c) (csrc/conv_common.hpp): the accumulator block of a producer -> (scale, shift) vectors — the stand-alone
// finish for consumers that do not do it in their prologue (dense-grid tile kernels, residual operands)
__global__ __launch_bounds__(256) void bn_acc_affine_kernel(const long long *acc, int ld, int c0, int C, float eps, float *scale,
                                                            float *shift)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float sc, sh;
    epconv::bn_acc_affine(acc, ld, c0 + c, eps, sc, sh);
    scale[c] = sc;
    shift[c] = sh;
}

// ... and the materialising consumer: out = [relu](x * scale + shift), every workgroup finishing the block itself (C <= 512)
constexpr int kAccRowsMaxC = 512;
__global__ __launch_bounds__(256) void affine_rows_acc_kernel(const float *x, int n, int C, int ld_x, const long long *acc, int ld,
                                                              int c0, float eps, int relu, float *out, int ld_out)
{
    __shared__ float sAff[2 * kAccRowsMaxC];
    for (int c = threadIdx.x; c < C; c += 256) epconv::bn_acc_affine(acc, ld, c0 + c, eps, sAff[c], sAff[kAccRowsMaxC + c]);
    __syncthreads();
    // a workgroup applies them to 16 x 256 elements
    for (int k = 0; k < 16; ++k) {
        const size_t e = ((size_t)blockIdx.x * 16 + k) * 256 + threadIdx.x;
        if (e >= (size_t)n * C) return;
        const int r = (int)(e / C), c = (int)(e - (size_t)r * C);
        float v = fmaf(x[(size_t)r * ld_x + c], sAff[c], sAff[kAccRowsMaxC + c]);
        if (relu) v = fmaxf(v, 0.0f);
        out[(size_t)r * ld_out + c] = v;
    }
}

// (One-launch forms for short summary lists — every workgroup finishing the statistics itself before applying them — were
// measured twice and removed: round 3 with one wave per channel (a 10 us serial chain of Chan merges per workgroup), round 4
// with 256 / C row groups merging side by side and the launch limited to ~16 MB of redundant summary reads: SPVCNN still lost
// 0.1-0.18 ms per level against the separate 5 us finalize launch, gpurun r04_c / r04_d.  A third form — workgroups of
// 64 channels x 256 rows, the list merged once per workgroup by four row lanes with eight summary rows in flight — lost as well:
// SPVCNN of the coarsest level 1.42 -> 1.68 ms.  The merge is a chain of dependent divisions; 74 workgroups repeating it in
// front of their rows is slower than one 5 us launch doing it once.)
//
// The exception is a handful of channels (C <= kBnMergeApplyMaxC: the single-channel BatchNorm of the occupancy logit, 864
// summaries x 3 floats = 10 KB): there the merge is 4 row merges per thread and one pass of the tree, and the finalize launch it
// replaces (5.5 us + a dependent boundary) is as long as the apply launch itself.  bn_merge_apply_kernel does bn_finalize_kernel's
// merges in bn_finalize_kernel's order — rows t, t + 256, ... per thread, then the tree (t, t + 128), (t, t + 64), ... (0, 1) with
// the lower index on the left — so mean and variance have the bits of the two-launch form: the levels 128 and 64 out of LDS by
// wave 0, the levels 32 .. 1 as down-shuffles inside it (lane t takes lane t + s; what the lanes >= s compute is never read).
// The rows are then normalised with bn_apply_kernel's expression (bn_apply_value).  EPRECON_INIT_GLUE=0: the two launches.
constexpr int kBnMergeApplyMaxC = 4;
constexpr int kBnMergeApplyBlocks = 256;    // workgroups at most: one per CU, the rows in grid strides

template <int NU>
__global__ __launch_bounds__(256) void bn_merge_apply_kernel(const float *x, int n, int C, int ld_x, const float *partial, int nblk,
                                                             int64_t ld, const float *gamma, const float *beta, float eps,
                                                             const float *res, int ld_res, const float *res_scale,
                                                             const float *res_shift, int relu, float *out, int ld_out,
                                                             float *mean_out, float *var_out)
{
    __shared__ float sN[256], sMean[256], sM2[256];
    __shared__ float sStat[2 * kBnMergeApplyMaxC];
    const int tid = threadIdx.x;
    for (int c = 0; c < C; ++c) {
        float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
        bn_merge_rows<NU>(partial, nblk, ld, C, c, tid, a_n, a_mean, a_m2);
        sN[tid] = a_n; sMean[tid] = a_mean; sM2[tid] = a_m2;
        __syncthreads();
        if (tid < 64) {
            chan_merge(a_n, a_mean, a_m2, sN[tid + 128], sMean[tid + 128], sM2[tid + 128]);
            float b_n = sN[tid + 64], b_mean = sMean[tid + 64], b_m2 = sM2[tid + 64];
            chan_merge(b_n, b_mean, b_m2, sN[tid + 192], sMean[tid + 192], sM2[tid + 192]);
            chan_merge(a_n, a_mean, a_m2, b_n, b_mean, b_m2);
#pragma unroll
            for (int s = 32; s > 0; s >>= 1) {
                const float on = __shfl_down(a_n, s), om = __shfl_down(a_mean, s), oq = __shfl_down(a_m2, s);
                chan_merge(a_n, a_mean, a_m2, on, om, oq);
            }
            if (tid == 0) {
                sStat[c] = a_mean;
                sStat[kBnMergeApplyMaxC + c] = a_n > 0.0f ? a_m2 / a_n : 0.0f;  // biased variance
            }
        }
        __syncthreads();
    }
    if (blockIdx.x == 0 && tid < C) {
        if (mean_out) mean_out[tid] = sStat[tid];
        if (var_out) var_out[tid] = sStat[kBnMergeApplyMaxC + tid];
    }
    const size_t total = (size_t)n * C;
    for (size_t e = (size_t)blockIdx.x * 256 + tid; e < total; e += (size_t)gridDim.x * 256) {
        const int r = (int)(e / C), c = (int)(e - (size_t)r * C);
        out[(size_t)r * ld_out + c] = bn_apply_value(x, ld_x, r, c, sStat, sStat + kBnMergeApplyMaxC, gamma, beta, eps, res, ld_res,
                                                     res_scale, res_shift, relu);
    }
}

// mean / var of a call: the caller's vectors where given, else two 256-byte-aligned runs of `channels` floats of the workspace
struct MeanVar { float *mean, *var; };
MeanVar carve_mean_var(void *workspace, int channels, float *mean_out, float *var_out)
{
    char *ws = reinterpret_cast<char *>(workspace);
    return {mean_out ? mean_out : reinterpret_cast<float *>(ws),
            var_out ? var_out : reinterpret_cast<float *>(ws + align_up((size_t)channels * sizeof(float), 256))};
}

int bn_finalize_apply(const float *x, int64_t n, int channels, int ld_x, const float *partial, int nblk, int64_t ld,
                      const float *gamma, const float *beta, float eps, const float *residual, int ld_res, const float *res_scale,
                      const float *res_shift, int relu, float *out, int ld_out, MeanVar mv, hipStream_t st)
{
    if (channels <= kBnMergeApplyMaxC && !switch_off("EPRECON_INIT_GLUE")) {
        const unsigned blocks = (unsigned)ceil_div(n * channels, (int64_t)256);
        const dim3 grid(blocks < (unsigned)kBnMergeApplyBlocks ? blocks : (unsigned)kBnMergeApplyBlocks);
        with_finalize_nu(nblk, [&](auto nu) {
            hipLaunchKernelGGL(bn_merge_apply_kernel<decltype(nu)::value>, grid, dim3(256), 0, st, x, (int)n, channels, ld_x, partial,
                               nblk, ld, gamma, beta, eps, residual, ld_res, res_scale, res_shift, relu, out, ld_out, mv.mean, mv.var);
        });
        EP_LAUNCH_CHECK();
        return EPRECON_OK;
    }
    with_finalize_nu(nblk, [&](auto nu) {
        hipLaunchKernelGGL(bn_finalize_kernel<decltype(nu)::value>, dim3(channels), dim3(256), 0, st, partial, nblk, ld, channels,
                           mv.mean, mv.var);
    });
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)ceil_div(n * channels, (int64_t)256)), dim3(256), 0, st, x, (int)n, channels,
                       ld_x, (const float *)mv.mean, (const float *)mv.var, gamma, beta, eps, residual, ld_res, res_scale, res_shift, relu,
                       out, ld_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// the joins: the same checks and the same choice between four channels per thread and one
using JoinKernel = void (*)(const float *, int, int, int, int, int, const float *, const float *, int, float *, int);

bool rows_vec4(const float *x, int ld_x, const float *out, int ld_out, int channels)
{
    return channels % 4 == 0 && ld_x % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)x | (uintptr_t)out) % 16 == 0;
}

// min_hw: the smallest height / width the join takes; out_rows: the rows it writes (the longer of the two lists bounds the index)
int affine_join_rows(JoinKernel vec4, JoinKernel vec1, int min_hw, int64_t out_rows, const float *x, int maps, int height,
                     int width, int channels, int ld_x, const float *scale, const float *shift, int relu, float *out, int ld_out,
                     void *stream)
{
    if (!x || !out || !scale || !shift || maps <= 0 || height < min_hw || width < min_hw || channels <= 0 || ld_x < channels ||
        ld_out < channels)
        return EPRECON_ERR_ARG;
    const int64_t in_rows = (int64_t)maps * height * width;
    if ((in_rows > out_rows ? in_rows : out_rows) * channels > 0x7fffffffll) return EPRECON_ERR_ARG;
    const bool v4 = rows_vec4(x, ld_x, out, ld_out, channels);
    const dim3 grid((unsigned)ceil_div(out_rows * (channels / (v4 ? 4 : 1)), (int64_t)256));
    hipLaunchKernelGGL(v4 ? vec4 : vec1, grid, dim3(256), 0, (hipStream_t)stream, x, maps, height, width, channels, ld_x, scale, shift,
                       relu, out, ld_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // namespace

extern "C" {

static inline int bn_rows_per_block(int channels) { return kBnPerThread * (256 / channels); }

size_t eprecon_batchnorm_workspace_bytes(int64_t n, int channels)
{
    if (channels <= 0 || channels > 256) return 0;
    const size_t nblk = (size_t)ceil_div(n > 0 ? n : 1, bn_rows_per_block(channels));
    return align_up(nblk * 3 * channels * sizeof(float), 256) + 2 * align_up((size_t)channels * sizeof(float), 256);
}

// Train-mode BatchNorm over the n rows: one statistics pass (per-block (count, mean, M2) merged
// with Chan's formula in fixed order -> deterministic, no cancellation), affine, optional residual
// add and ReLU.  out may alias x.  mean_out / var_out (optional, device) receive the statistics.
int eprecon_batchnorm_train_async(const float *x, int64_t n, int channels, int ld_x, const float *gamma,
                                  const float *beta, float eps, const float *residual, int ld_res,
                                  int relu, float *out, int ld_out, float *mean_out, float *var_out,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !out || n < 0 || channels <= 0 || channels > 256 || ld_x < channels || ld_out < channels ||
        !workspace)
        return EPRECON_ERR_ARG;
    if (workspace_bytes < eprecon_batchnorm_workspace_bytes(n, channels)) return EPRECON_ERR_WORKSPACE;
    if (n == 0) return EPRECON_OK;
    hipStream_t st = (hipStream_t)stream;
    const int nblk = (int)ceil_div(n, bn_rows_per_block(channels));
    float *partial = reinterpret_cast<float *>(workspace);
    char *rest = reinterpret_cast<char *>(workspace) + align_up((size_t)nblk * 3 * channels * sizeof(float), 256);
    hipLaunchKernelGGL(bn_stats_kernel, dim3(nblk), dim3(256), 0, st, x, (int)n, channels, ld_x, partial);
    EP_LAUNCH_CHECK();
    return bn_finalize_apply(x, n, channels, ld_x, partial, nblk, nblk, gamma, beta, eps, residual, ld_res, nullptr, nullptr, relu, out,
                             ld_out, carve_mean_var(rest, channels, mean_out, var_out), st);
}

size_t eprecon_batchnorm_apply_workspace_bytes(int channels)
{
    return 2 * align_up((size_t)(channels > 0 ? channels : 1) * sizeof(float), 256);
}

// Second half of the train-mode BatchNorm for a tensor whose per-block (count, mean, M2) summaries
// were already produced by its producer (eprecon_sparse_conv_fused_async's bn_partial,
// [3][channels][ld], ld >= nblk): fixed-order merge -> mean / biased variance -> affine [+ residual] [ReLU].
// res_scale / res_shift: both or neither, and only with a residual (its pending BatchNorm, applied on load).
int eprecon_batchnorm_apply_partials_async(const float *x, int64_t n, int channels, int ld_x, const float *partial, int64_t nblk,
                                           int64_t ld, const float *gamma, const float *beta, float eps, const float *residual,
                                           int ld_res, const float *res_scale, const float *res_shift, int relu, float *out,
                                           int ld_out, float *mean_out, float *var_out, void *workspace, size_t workspace_bytes,
                                           void *stream)
{
    if (!x || !out || !partial || n < 0 || nblk <= 0 || nblk > 0x7fffffff || ld < nblk || channels <= 0 || ld_x < channels ||
        ld_out < channels || !workspace || (residual && ld_res < channels) || !res_scale != !res_shift || (res_scale && !residual))
        return EPRECON_ERR_ARG;
    if (workspace_bytes < eprecon_batchnorm_apply_workspace_bytes(channels)) return EPRECON_ERR_WORKSPACE;
    if (n == 0) return EPRECON_OK;
    return bn_finalize_apply(x, n, channels, ld_x, partial, (int)nblk, ld, gamma, beta, eps, residual, ld_res, res_scale, res_shift,
                             relu, out, ld_out, carve_mean_var(workspace, channels, mean_out, var_out), (hipStream_t)stream);
}

int eprecon_batchnorm_finalize_affine_async(const float *partial, int64_t nblk, int64_t ld, int channels, const float *gamma,
                                            const float *beta, float eps, float *scale_out, float *shift_out,
                                            void *stream)
{
    if (!partial || !scale_out || !shift_out || nblk <= 0 || nblk > 0x7fffffff || ld < nblk || channels <= 0) return EPRECON_ERR_ARG;
    with_finalize_nu(nblk, [&](auto nu) {
        hipLaunchKernelGGL(bn_finalize_affine_kernel<decltype(nu)::value>, dim3(channels), dim3(256), 0, (hipStream_t)stream, partial,
                           (int)nblk, ld, channels, gamma, beta, eps, scale_out, shift_out);
    });
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// out = [relu]( x * scale + shift [+ residual] ): the materialising consumer of a pending BatchNorm, and the tail of the residual
// blocks (models/modules.py:46-72); residual may be null; out may alias x
int eprecon_affine_rows_async(const float *x, int64_t n, int channels, int ld_x, const float *scale, const float *shift,
                              const float *residual, int ld_res, int relu, float *out, int ld_out, void *stream)
{
    if (!x || !out || !scale || !shift || n < 0 || channels <= 0 || ld_x < channels || ld_out < channels ||
        (residual && ld_res < channels) || n * channels > 0x7fffffffll * 256)
        return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    hipLaunchKernelGGL(residual ? affine_rows_kernel<true> : affine_rows_kernel<false>,
                       dim3((unsigned)ceil_div(n * channels, (int64_t)256)), dim3(256), 0, (hipStream_t)stream, x, (int)n, channels,
                       ld_x, scale, shift, relu, out, ld_out, residual, ld_res);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_affine_pool2_rows_async(const float *x, int maps, int height, int width, int channels, int ld_x, const float *scale,
                                    const float *shift, int relu, float *out, int ld_out, void *stream)
{
    return affine_join_rows(affine_pool2_rows_kernel<4>, affine_pool2_rows_kernel<1>, 2, (int64_t)maps * (height / 2) * (width / 2),
                            x, maps, height, width, channels, ld_x, scale, shift, relu, out, ld_out, stream);
}

int eprecon_affine_up2_rows_async(const float *x, int maps, int height, int width, int channels, int ld_x, const float *scale,
                                  const float *shift, int relu, float *out, int ld_out, void *stream)
{
    return affine_join_rows(affine_up2_rows_kernel<4>, affine_up2_rows_kernel<1>, 1, (int64_t)maps * 4 * height * width, x, maps,
                            height, width, channels, ld_x, scale, shift, relu, out, ld_out, stream);
}

int eprecon_batchnorm_acc_affine_async(const long long *acc, int acc_ld, int acc_c0, int channels, float eps, float *scale_out,
                                       float *shift_out, void *stream)
{
    if (!acc || !scale_out || !shift_out || channels <= 0 || acc_c0 < 0 || acc_c0 + channels > acc_ld) return EPRECON_ERR_ARG;
    hipLaunchKernelGGL(bn_acc_affine_kernel, dim3((unsigned)ceil_div(channels, 256)), dim3(256), 0, (hipStream_t)stream, acc, acc_ld,
                       acc_c0, channels, eps, scale_out, shift_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_affine_rows_acc_async(const float *x, int64_t n, int channels, int ld_x, const long long *acc, int acc_ld, int acc_c0,
                                  float eps, int relu, float *out, int ld_out, void *stream)
{
    if (!x || !out || !acc || n < 0 || channels <= 0 || channels > kAccRowsMaxC || ld_x < channels || ld_out < channels ||
        acc_c0 < 0 || acc_c0 + channels > acc_ld || n * channels > 0x7fffffffll * 256)
        return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    hipLaunchKernelGGL(affine_rows_acc_kernel, dim3((unsigned)ceil_div(n * channels, (int64_t)4096)), dim3(256), 0,
                       (hipStream_t)stream, x, (int)n, channels, ld_x, acc, acc_ld, acc_c0, eps, relu, out, ld_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_rowwise_layernorm_async(const float *x, int64_t n, int channels, int ld_x,
                                    const float *residual, int ld_res, const float *gamma,
                                    const float *beta, float eps, int pre_relu, int post_relu,
                                    float *out, int ld_out, void *stream)
{
    if (!x || !out || n < 0 || channels <= 0 || ld_x < channels || ld_out < channels) return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    hipLaunchKernelGGL(rowwise_ln_kernel, dim3((unsigned)ceil_div(n, 32)), dim3(256), 0,
                       (hipStream_t)stream, x, (int)n, channels, ld_x, residual, ld_res, gamma, beta, eps,
                       pre_relu, post_relu, out, ld_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
