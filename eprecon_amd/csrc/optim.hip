// The last stage of an optimisation step (main.py:308-310: clip_grad_norm_(1.0), optimizer.step()) over every trainable
// parameter in two or three launches: the gradients' global L2 norm, summed in double in a fixed order, and torch's
// non-amsgrad Adam with the clip coefficient folded into the gradient load.  The work is cut into chunks of one parameter
// each (eprecon_adam_chunk, built on the host), one workgroup per chunk; nothing is accumulated with atomics, so a step is
// bit-identical from run to run.
#include "common.hpp"

namespace {
constexpr int kBlock = 256;

// Sum of one double per thread over the workgroup in a fixed order: lanes by halving shuffles, then the waves in index
// order through LDS.  Every thread returns the total.  One __syncthreads() pair; every thread of the block must call it.
__device__ __forceinline__ double block_sum_ordered(double x, double *wave_sums)
{
#pragma unroll
    for (int off = ep::kWave / 2; off > 0; off >>= 1) x += __shfl_down(x, off, ep::kWave);
    const int lane = threadIdx.x & (ep::kWave - 1), wid = threadIdx.x / ep::kWave;
    if (lane == 0) wave_sums[wid] = x;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / ep::kWave; ++w) total += wave_sums[w];
    __syncthreads();
    return total;
}

// partial[c] = sum of the squares of chunk c's gradient elements.  A float's square is exact in double: only the
// additions round.
__global__ __launch_bounds__(kBlock) void grad_sqsum_kernel(const eprecon_adam_segment *segs, const eprecon_adam_chunk *chunks,
                                                            double *partials)
{
    __shared__ double wave_sums[kBlock / ep::kWave];
    const eprecon_adam_chunk c = chunks[blockIdx.x];
    const float *g = segs[c.segment].grad + c.start;
    double acc = 0.0;
    int done = 0;
    if (c.flags & EPRECON_ADAM_GRAD_ALIGNED) {
        const int n4 = c.count >> 2;
        const float4 *g4 = reinterpret_cast<const float4 *>(g);
        for (int i = threadIdx.x; i < n4; i += kBlock) {
            const float4 q = g4[i];
            acc += (double)q.x * (double)q.x;
            acc += (double)q.y * (double)q.y;
            acc += (double)q.z * (double)q.z;
            acc += (double)q.w * (double)q.w;
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < c.count; i += kBlock) acc += (double)g[i] * (double)g[i];
    const double total = block_sum_ordered(acc, wave_sums);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// The partials in index order (thread t takes t, t + 256, ...; then block_sum_ordered) -> what clip_grad_norm_ forms
// from the norm: float norm, coef = min(1, max_norm / (norm + 1e-6)) with a NaN kept (torch.clamp keeps it).
__device__ __forceinline__ float2 norm_and_coef(const double *partials, int nchunks, float max_norm, double *wave_sums)
{
    double acc = 0.0;
    for (int i = threadIdx.x; i < nchunks; i += kBlock) acc += partials[i];
    const double total = block_sum_ordered(acc, wave_sums);
    const float norm = (float)sqrt(total);
    const float c = max_norm / (norm + 1e-6f);
    return make_float2(norm, c >= 1.0f ? 1.0f : c);
}

__global__ __launch_bounds__(kBlock) void grad_norm_finish_kernel(const double *partials, int nchunks, float max_norm, float *norm_coef)
{
    __shared__ double wave_sums[kBlock / ep::kWave];
    const float2 nc = norm_and_coef(partials, nchunks, max_norm, wave_sums);
    if (threadIdx.x == 0) { norm_coef[0] = nc.x; norm_coef[1] = nc.y; }
}

struct AdamConsts {
    float lerp_w, beta2, one_minus_beta2, eps, wd, coef, step_size, bias2_sqrt;
};

// torch/optim/adam.py (_multi_tensor_adam, amsgrad off, maximize off), operation by operation; each multiply-add that ends an
// operation is one fused operation (one rounding)
__device__ __forceinline__ void adam_one(float &p, float grad, float &m, float &v, const AdamConsts &k)
{
    float g = grad * k.coef;
    if (k.wd != 0.0f) g = fmaf(k.wd, p, g);
    m = fmaf(k.lerp_w, g - m, m);
    v = fmaf(k.one_minus_beta2 * g, g, v * k.beta2);
    const float denom = sqrtf(v) / k.bias2_sqrt + k.eps;
    p = fmaf(-k.step_size, m / denom, p);
}

// RESUM: no finish launch; every workgroup sums the partials itself (the same order, so the same bits) and workgroup 0
// stores the norm.  Otherwise norm_coef holds what the finish launch left, or is NULL: no clipping.
template <bool RESUM>
__global__ __launch_bounds__(kBlock) void adam_update_kernel(const eprecon_adam_segment *segs, const eprecon_adam_chunk *chunks,
                                                             const float *seg_scalars, float lerp_w, float beta2,
                                                             float one_minus_beta2, float eps, float wd, const double *partials,
                                                             int nchunks, float max_norm, float *norm_coef)
{
    __shared__ double wave_sums[kBlock / ep::kWave];
    AdamConsts k;
    k.lerp_w = lerp_w; k.beta2 = beta2; k.one_minus_beta2 = one_minus_beta2; k.eps = eps; k.wd = wd;
    if (RESUM) {
        const float2 nc = norm_and_coef(partials, nchunks, max_norm, wave_sums);
        if (blockIdx.x == 0 && threadIdx.x == 0) { norm_coef[0] = nc.x; norm_coef[1] = nc.y; }
        k.coef = nc.y;
    } else {
        k.coef = norm_coef ? norm_coef[1] : 1.0f;
    }
    const eprecon_adam_chunk c = chunks[blockIdx.x];
    const eprecon_adam_segment s = segs[c.segment];
    k.step_size = seg_scalars[2 * c.segment];
    k.bias2_sqrt = seg_scalars[2 * c.segment + 1];
    float *p = s.param + c.start, *m = s.exp_avg + c.start, *v = s.exp_avg_sq + c.start;
    const float *g = s.grad + c.start;
    int done = 0;
    if (c.flags & EPRECON_ADAM_ALL_ALIGNED) {
        const int n4 = c.count >> 2;
        float4 *p4 = reinterpret_cast<float4 *>(p), *m4 = reinterpret_cast<float4 *>(m), *v4 = reinterpret_cast<float4 *>(v);
        const float4 *g4 = reinterpret_cast<const float4 *>(g);
        for (int i = threadIdx.x; i < n4; i += kBlock) {
            float4 pp = p4[i], mm = m4[i], vv = v4[i];
            const float4 gg = g4[i];
            adam_one(pp.x, gg.x, mm.x, vv.x, k);
            adam_one(pp.y, gg.y, mm.y, vv.y, k);
            adam_one(pp.z, gg.z, mm.z, vv.z, k);
            adam_one(pp.w, gg.w, mm.w, vv.w, k);
            p4[i] = pp; m4[i] = mm; v4[i] = vv;
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < c.count; i += kBlock) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_one(pp, g[i], mm, vv, k);
        p[i] = pp; m[i] = mm; v[i] = vv;
    }
}
}  // namespace

extern "C" int eprecon_grad_sqsum_async(const eprecon_adam_segment *segs_dev, const eprecon_adam_chunk *chunks_dev, int nchunks,
                                        double *partials, void *stream)
{
    if (nchunks < 0 || (nchunks > 0 && (!segs_dev || !chunks_dev || !partials))) return EPRECON_ERR_ARG;
    if (nchunks == 0) return EPRECON_EMPTY;
    hipLaunchKernelGGL(grad_sqsum_kernel, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, segs_dev, chunks_dev,
                       partials);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" int eprecon_grad_norm_finish_async(const double *partials, int nchunks, float max_norm, float *norm_coef, void *stream)
{
    if (nchunks <= 0 || !partials || !norm_coef) return EPRECON_ERR_ARG;
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kBlock), 0, (hipStream_t)stream, partials, nchunks, max_norm,
                       norm_coef);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" int eprecon_adam_update_async(const eprecon_adam_segment *segs_dev, const eprecon_adam_chunk *chunks_dev, int nchunks,
                                         const float *seg_scalars, float lerp_weight, float beta2, float one_minus_beta2, float eps,
                                         float weight_decay, const double *partials, float max_norm, float *norm_coef, void *stream)
{
    if (nchunks < 0 || (nchunks > 0 && (!segs_dev || !chunks_dev || !seg_scalars)) || (partials && !norm_coef))
        return EPRECON_ERR_ARG;
    if (nchunks == 0) return EPRECON_EMPTY;
    if (partials)
        hipLaunchKernelGGL(adam_update_kernel<true>, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, segs_dev,
                           chunks_dev, seg_scalars, lerp_weight, beta2, one_minus_beta2, eps, weight_decay, partials, nchunks,
                           max_norm, norm_coef);
    else
        hipLaunchKernelGGL(adam_update_kernel<false>, dim3((unsigned)nchunks), dim3(kBlock), 0, (hipStream_t)stream, segs_dev,
                           chunks_dev, seg_scalars, lerp_weight, beta2, one_minus_beta2, eps, weight_decay, partials, nchunks,
                           max_norm, norm_coef);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
