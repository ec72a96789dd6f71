// Fragment ground truth cut out of a scene's full volumes on gfx950 (the data-preparation side).
//
// Replaces the per-sample CPU work of RandomTransformSpace.transform         datasets/transforms.py:263-359,367-424
// that follows the TSDF integration: for every voxel of the fragment volume at its three resolutions, the sample
// coordinate in the scene's full volume under the augmentation transform, then
//   tsdf      grid_sample nearest; the trilinear value instead where |nearest| < 1; 1 where a normalised coordinate
//             leaves (-1, 1)                                                                     (:311-320,348-349)
//   colour / semantic / instance   grid_sample nearest, zeros padding; 0 where a coordinate leaves (-1, 1)  (:322-353)
// The coordinate follows the reference's fp32 operation order with explicit round-to-nearest intrinsics:
//   X = i * vs + origin_partial                   (i in finest cells: i_l * 2^l, :269)
//   w = M[:3,:] @ [X,1]                           (k-ordered fma chain = torch's CPU matmul, as tsdf_fusion.hip variant 0, :271)
//   c = (w - old_origin) / vs, then / 2^l         (:272,300)
//   n = 2 c / (D - 1) - 1                         (D = that level's full-volume dims, :306)
//   u = ((n + 1) D - 1) / 2                       (grid_sample's align_corners=False un-normalisation)
// Grid component 0 indexes the volume's LAST axis (:307 `[[2, 1, 0]]`), which only names the axes: every axis goes
// through the same arithmetic.  Nearest index: rintf (ties to even), as grid_sample's nearbyint.
// One thread per output voxel of ANY level (one launch per sample; z fastest = coalesced stores); each thread reads
// 1 nearest TSDF tap (+ 8 trilinear taps inside the band), one 12-byte colour tap and two label taps.  No atomics,
// no host read, the caller's stream.
#include <math.h>

#include "common.hpp"

namespace {
using namespace ep;

struct GtCropArgs {
    eprecon_gt_crop_desc d;
    int32_t out_dims[3][3];   // level l: ceil(dims / 2^l) (the reference's `::2**l` slices)
    int32_t end[3];           // running sum of the levels' cells
};

__device__ __forceinline__ float crop_tap(const float *vol, int ix, int iy, int iz, int dx, int dy, int dz)
{
    if (ix < 0 || iy < 0 || iz < 0 || ix >= dx || iy >= dy || iz >= dz) return 0.0f;
    return vol[((size_t)ix * dy + iy) * dz + iz];
}

__global__ __launch_bounds__(256) void gt_crop_kernel(GtCropArgs a)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    const int levels = a.d.levels;
    if (idx >= a.end[levels - 1]) return;
    int l = 0;
    while (l < levels - 1 && idx >= a.end[l]) ++l;
    const int local = idx - (l ? a.end[l - 1] : 0);
    const int oy = a.out_dims[l][1], oz = a.out_dims[l][2];
    const int iz = local % oz, iy = (local / oz) % oy, ix = local / (oz * oy);
    const int fi[3] = {ix << l, iy << l, iz << l};
    const float vs = a.d.voxel_size, scale = (float)(1 << l);
    float X[3], u[3];
    bool outside = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) X[k] = __fadd_rn(__fmul_rn((float)fi[k], vs), a.d.origin_partial[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float *m = a.d.transform + 4 * k;
        const float w = __fmaf_rn(1.0f, m[3], __fmaf_rn(X[2], m[2], __fmaf_rn(X[1], m[1], __fmul_rn(m[0], X[0]))));
        const float c = __fdiv_rn(__fdiv_rn(__fsub_rn(w, a.d.old_origin[k]), vs), scale);
        const float D = (float)a.d.full_dims[l][k];
        const float n = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, c), __fsub_rn(D, 1.0f)), 1.0f);
        outside |= !(fabsf(n) < 1.0f);                            // |n| >= 1, and a NaN coordinate
        u[k] = __fdiv_rn(__fsub_rn(__fmul_rn(__fadd_rn(n, 1.0f), D), 1.0f), 2.0f);
    }
    const int dx = a.d.full_dims[l][0], dy = a.d.full_dims[l][1], dz = a.d.full_dims[l][2];
    float tsdf = 1.0f, rgb[3] = {0.0f, 0.0f, 0.0f}, sem = 0.0f, ins = 0.0f;
    if (!outside) {
        // |n| < 1  =>  -0.5 < u < D - 0.5: the nearest cell can still fall outside by rounding, hence the bounds test
        const int nx = (int)rintf(u[0]), ny = (int)rintf(u[1]), nz = (int)rintf(u[2]);
        const bool in = nx >= 0 && ny >= 0 && nz >= 0 && nx < dx && ny < dy && nz < dz;
        const size_t cell = in ? ((size_t)nx * dy + ny) * dz + nz : 0;
        tsdf = in ? a.d.tsdf_full[l][cell] : 0.0f;
        if (fabsf(tsdf) < 1.0f) {
            // grid_sampler_3d's corner order and weights (grid x = our z): x0 = floor(u), weights from the opposite corner
            const float fx = floorf(u[0]), fy = floorf(u[1]), fz = floorf(u[2]);
            const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
            const float wx1 = __fsub_rn(u[0], fx), wx0 = __fsub_rn(__fadd_rn(fx, 1.0f), u[0]);
            const float wy1 = __fsub_rn(u[1], fy), wy0 = __fsub_rn(__fadd_rn(fy, 1.0f), u[1]);
            const float wz1 = __fsub_rn(u[2], fz), wz0 = __fsub_rn(__fadd_rn(fz, 1.0f), u[2]);
            const float *vol = a.d.tsdf_full[l];
            float acc = 0.0f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {     // bit 0: z (grid x), bit 1: y, bit 2: x (grid z) — tnw, tne, tsw, tse, bnw, ...
                const int bz = c & 1, by = (c >> 1) & 1, bx = c >> 2;
                const float w = __fmul_rn(__fmul_rn(bz ? wz1 : wz0, by ? wy1 : wy0), bx ? wx1 : wx0);
                acc = __fadd_rn(acc, __fmul_rn(crop_tap(vol, x0 + bx, y0 + by, z0 + bz, dx, dy, dz), w));
            }
            tsdf = acc;
        }
        if (in && a.d.rgb_full[l]) {
            const float *p = a.d.rgb_full[l] + cell * 3;
            rgb[0] = p[0]; rgb[1] = p[1]; rgb[2] = p[2];
        }
        if (in && a.d.semantic_full[l]) sem = (float)a.d.semantic_full[l][cell];
        if (in && a.d.instance_full[l]) ins = (float)a.d.instance_full[l][cell];
    }
    a.d.tsdf_out[l][local] = tsdf;
    if (a.d.rgb_out[l]) {
        float *p = a.d.rgb_out[l] + (size_t)local * 3;
        p[0] = rgb[0]; p[1] = rgb[1]; p[2] = rgb[2];
    }
    if (a.d.semantic_out[l]) a.d.semantic_out[l][local] = sem;
    if (a.d.instance_out[l]) a.d.instance_out[l][local] = ins;
}

}  // namespace

extern "C" int eprecon_gt_crop_async(const eprecon_gt_crop_desc *desc, void *stream)
{
    if (!desc || desc->levels < 1 || desc->levels > 3 || !(desc->voxel_size > 0.0f)) return EPRECON_ERR_ARG;
    GtCropArgs a;
    a.d = *desc;
    int64_t total = 0;
    for (int l = 0; l < 3; ++l) {
        if (l >= desc->levels) {
            a.end[l] = (int32_t)total;
            for (int k = 0; k < 3; ++k) a.out_dims[l][k] = 0;
            continue;
        }
        // an output needs its source and the other way round; colour / labels are optional as a group per kind
        if (!desc->tsdf_full[l] || !desc->tsdf_out[l] || !desc->rgb_full[l] != !desc->rgb_out[l] ||
            !desc->semantic_full[l] != !desc->semantic_out[l] || !desc->instance_full[l] != !desc->instance_out[l])
            return EPRECON_ERR_ARG;
        int64_t cells = 1, full = 1;
        for (int k = 0; k < 3; ++k) {
            if (desc->dims[k] <= 0 || desc->full_dims[l][k] <= 0) return EPRECON_ERR_ARG;
            if (desc->full_dims[l][k] < 2) return EPRECON_ERR_UNSUPPORTED;      // D - 1 divides the coordinate
            a.out_dims[l][k] = (desc->dims[k] + (1 << l) - 1) >> l;
            cells *= a.out_dims[l][k];
            full *= desc->full_dims[l][k];
        }
        total += cells;
        if (total > 0x7fffffff - 256 || full > 0x7fffffff ||      // (- 256: the last block's thread ids stay positive)
            desc->dims[0] > (1 << 24) || desc->dims[1] > (1 << 24) || desc->dims[2] > (1 << 24))
            return EPRECON_ERR_UNSUPPORTED;                                      // int32 cell ids, indices exact in fp32
        a.end[l] = (int32_t)total;
    }
    hipLaunchKernelGGL(gt_crop_kernel, dim3((unsigned)ceil_div(total, 256)), dim3(256), 0, (hipStream_t)stream, a);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
