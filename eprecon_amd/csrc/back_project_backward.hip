// Backward pass of the multi-view back-projection (back_project.hip) for gfx950: gradient of the gathered rows with respect to
// the channels-last image features, as float atomics or as an order-independent 64-bit fixed-point sum.
#include "back_project_common.hpp"

namespace {
using namespace ep;

// ---------------------------------------------------------------------------------------------
// Backward of the back-projection with respect to the image features (training): the
// transpose of the bilinear gather is a scatter of four weighted taps per (voxel, visible view, channel).
//   MEAN / MEAN_DEPTH   d f_v = d out / cnt                          (the mean-depth channel has no feature gradient)
//   VARIANCE            d f_v = 2 (f_v - mean) / cnt * d var + d mean / cnt
// One thread per (valid voxel, channel): consecutive lanes hit consecutive addresses of one pixel, so the
// hardware float atomics of a wave coalesce.  Same projection and tap arithmetic as bp_gather_kernel.
// ---------------------------------------------------------------------------------------------
struct BpBwdParams {
    const int32_t *coords; int64_t n;      // the VALID voxels (out_coords of the forward)
    const float *origin; int batch; float voxel_size;
    const float *feats_nhwc; const float *krcam;
    int V, C, H, W, mode;
    const float *dout; int ld_dout;
    const float *dmean;                    // VARIANCE only, may be null
    float *dfeats;                         // [V*B][H*W][C], zeroed by the caller
    unsigned long long *dfix;              // the same elements as 64-bit fixed point (deterministic form), or null
};

constexpr double kFixScale = 1099511627776.0;   // 2^40
__device__ __forceinline__ unsigned long long to_fixed(float v)
{
    const double x = fmin(fmax((double)v * kFixScale, -9.0e18), 9.0e18);
    return (unsigned long long)__double2ll_rn(x);           // two's complement: an unsigned add is a signed add
}
// A contribution the fixed-point word cannot hold must stay visible: the clamp above would turn NaN / Inf, and any finite value
// beyond +-8.2e6, into a finite +-8.2e6.  Such a contribution (non-finite, or |v| > kFixMax) is not added; the element of the
// fp32 output (zeroed by the caller) is marked NaN instead — a plain store of one value, so still independent of the order — and
// the conversion below leaves marked elements alone.  (A SUM of in-range contributions beyond 2^23 still wraps: see the header.)
constexpr float kFixMax = 8.0e6f;   // < 9.0e18 / 2^40 = 8.19e6
__device__ __forceinline__ void fixed_add(unsigned long long *acc, float *mark, float v)
{
    if (fabsf(v) <= kFixMax) atomicAdd(acc, to_fixed(v));   // (false for NaN)
    else *mark = __builtin_nanf("");
}
__global__ void fixed_to_float_kernel(const unsigned long long *acc, long long n, float *out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && !__builtin_isnan(out[i])) out[i] = (float)((double)(long long)acc[i] * (1.0 / kFixScale));
}

__global__ __launch_bounds__(256) void bp_backward_kernel(BpBwdParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sP = reinterpret_cast<float *>(smem);
    stage_matrices(sP, p.krcam, p.V * p.batch, threadIdx.x, 256);
    __syncthreads();
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= p.n * p.C) return;
    const int64_t i = e / p.C;
    const int ch = (int)(e - i * p.C);
    const int4 c = reinterpret_cast<const int4 *>(p.coords)[i];
    if (c.x < 0 || c.x >= p.batch) return;
    float X, Y, Z;
    voxel_centre(c, p.origin, p.voxel_size, X, Y, Z);
    const float wm1 = (float)(p.W - 1), hm1 = (float)(p.H - 1);
    const size_t map_elems = (size_t)p.H * p.W * p.C;
    int cnt = 0;
    for (int v = 0; v < p.V; ++v) cnt += project(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1).vis ? 1 : 0;
    if (cnt == 0) return;
    const float inv = 1.0f / (float)cnt;
    const float g = p.dout[i * p.ld_dout + ch];
    float mean = 0.0f;
    if (p.mode == EPRECON_BP_VARIANCE) {
        for (int v = 0; v < p.V; ++v) {
            const Proj pr = project(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1);
            if (!pr.vis) continue;
            const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(pr.gx, 1.0f), 2.0f), wm1);
            const float iy = __fmul_rn(__fdiv_rn(__fadd_rn(pr.gy, 1.0f), 2.0f), hm1);
            mean += Chan<1>::sample(p.feats_nhwc + ((size_t)v * p.batch + c.x) * map_elems + ch, make_taps(ix, iy, p.W, p.H, p.C)).v;
        }
        mean *= inv;
    }
    const float gm = (p.mode == EPRECON_BP_VARIANCE && p.dmean) ? p.dmean[i * p.C + ch] * inv : 0.0f;
    for (int v = 0; v < p.V; ++v) {
        const Proj pr = project(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1);
        if (!pr.vis) continue;
        const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(pr.gx, 1.0f), 2.0f), wm1);
        const float iy = __fmul_rn(__fdiv_rn(__fadd_rn(pr.gy, 1.0f), 2.0f), hm1);
        const Taps t = make_taps(ix, iy, p.W, p.H, p.C);
        const size_t mo = ((size_t)v * p.batch + c.x) * map_elems + ch;
        float gv;
        if (p.mode == EPRECON_BP_VARIANCE) {
            const float f = Chan<1>::sample(p.feats_nhwc + mo, t).v;
            gv = 2.0f * (f - mean) * inv * g + gm;
        } else {
            gv = g * inv;
        }
        if (p.dfix) {
            // order-independent accumulation: 64-bit fixed point (2^-40 resolution, |sum| < 8.4e6), integer atomics
            unsigned long long *d = p.dfix + mo;
            float *m = p.dfeats + mo;
            if (t.w00 != 0.0f) fixed_add(d + t.o00, m + t.o00, t.w00 * gv);
            if (t.w10 != 0.0f) fixed_add(d + t.o10, m + t.o10, t.w10 * gv);
            if (t.w01 != 0.0f) fixed_add(d + t.o01, m + t.o01, t.w01 * gv);
            if (t.w11 != 0.0f) fixed_add(d + t.o11, m + t.o11, t.w11 * gv);
        } else {
            float *d = p.dfeats + mo;
            if (t.w00 != 0.0f) unsafeAtomicAdd(d + t.o00, t.w00 * gv);
            if (t.w10 != 0.0f) unsafeAtomicAdd(d + t.o10, t.w10 * gv);
            if (t.w01 != 0.0f) unsafeAtomicAdd(d + t.o01, t.w01 * gv);
            if (t.w11 != 0.0f) unsafeAtomicAdd(d + t.o11, t.w11 * gv);
        }
    }
}

}  // namespace

extern "C" {

static int bp_backward_impl(const int32_t *coords_valid, int64_t n_valid, const float *origin, int batch, float voxel_size,
                            const float *feats_nhwc, const float *krcam, int n_views, int channels, int height, int width, int mode,
                            const float *dout, int ld_dout, const float *dmean, float *dfeats_nhwc, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    if (n_valid < 0 || batch < 1 || n_views < 1 || channels < 1 || !dfeats_nhwc || !krcam || !origin) return EPRECON_ERR_ARG;
    if (mode == EPRECON_BP_VARIANCE && !feats_nhwc) return EPRECON_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const size_t elems = (size_t)n_views * batch * height * width * channels;
    if (workspace && workspace_bytes < elems * sizeof(unsigned long long)) return EPRECON_ERR_WORKSPACE;
    if (workspace) EP_HIP_CHECK(hipMemsetAsync(workspace, 0, elems * sizeof(unsigned long long), st));
    // (the fp32 output is zeroed in the fixed-point form too: it carries the NaN marks of non-finite contributions, fixed_add)
    EP_HIP_CHECK(hipMemsetAsync(dfeats_nhwc, 0, elems * sizeof(float), st));
    if (n_valid == 0) return EPRECON_OK;
    if (!coords_valid || !dout) return EPRECON_ERR_ARG;
    BpBwdParams p;
    p.coords = coords_valid; p.n = n_valid; p.origin = origin; p.batch = batch; p.voxel_size = voxel_size;
    p.feats_nhwc = feats_nhwc; p.krcam = krcam; p.V = n_views; p.C = channels; p.H = height; p.W = width; p.mode = mode;
    p.dout = dout; p.ld_dout = ld_dout; p.dmean = dmean; p.dfeats = dfeats_nhwc; p.dfix = (unsigned long long *)workspace;
    const size_t lds = (((size_t)n_views * batch * 12 + 3) & ~(size_t)3) * sizeof(float);
    hipLaunchKernelGGL(bp_backward_kernel, dim3((unsigned)ceil_div(n_valid * channels, 256)), dim3(256), lds, st, p);
    EP_LAUNCH_CHECK();
    if (workspace) {
        hipLaunchKernelGGL(fixed_to_float_kernel, dim3((unsigned)ceil_div((int64_t)elems, 256)), dim3(256), 0, st,
                           (const unsigned long long *)workspace, (long long)elems, dfeats_nhwc);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

int eprecon_back_project_backward_async(const int32_t *coords_valid, int64_t n_valid, const float *origin, int batch,
                                        float voxel_size, const float *feats_nhwc, const float *krcam, int n_views,
                                        int channels, int height, int width, int mode, const float *dout, int ld_dout,
                                        const float *dmean, float *dfeats_nhwc, void *stream)
{
    return bp_backward_impl(coords_valid, n_valid, origin, batch, voxel_size, feats_nhwc, krcam, n_views, channels, height, width, mode,
                            dout, ld_dout, dmean, dfeats_nhwc, nullptr, 0, stream);
}

size_t eprecon_back_project_backward_workspace_bytes(int batch, int n_views, int channels, int height, int width)
{
    return (size_t)n_views * batch * height * width * channels * sizeof(unsigned long long);
}

int eprecon_back_project_backward_det_async(const int32_t *coords_valid, int64_t n_valid, const float *origin, int batch,
                                            float voxel_size, const float *feats_nhwc, const float *krcam, int n_views,
                                            int channels, int height, int width, int mode, const float *dout, int ld_dout,
                                            const float *dmean, float *dfeats_nhwc, void *workspace, size_t workspace_bytes,
                                            void *stream)
{
    if (!workspace) return EPRECON_ERR_ARG;
    return bp_backward_impl(coords_valid, n_valid, origin, batch, voxel_size, feats_nhwc, krcam, n_views, channels, height, width, mode,
                            dout, ld_dout, dmean, dfeats_nhwc, workspace, workspace_bytes, stream);
}

}  // extern "C"
