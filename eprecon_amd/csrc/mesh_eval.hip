// Scene evaluation on gfx950 — tools/evaluation.py + tools/evaluation_utils.py of the reference (pyrender, open3d and a
// per-point Python KD-tree loop there), driven by eprecon_amd/evaluation.py.
//
//   render_depth     depth of the predicted mesh at every camera pose (pyrender's OpenGL render, culling back faces)
//   depth_metrics    eval_depth's nine numbers, as ten fp64 sums per frame (one reduction over a chunk of frames)
//   point_bounds     bounding box of a cloud (the down-sample's min bound, the NN grid)
//   voxel_down_sample   open3d VoxelDownSample, deterministic and in voxel-key order
//   nn_search        nn_correspondance: exact nearest neighbour through a uniform grid, smallest index on ties
//
// Rasteriser: csrc/mesh_raster.hpp (one thread per (triangle, view), a wave per large pixel box, fp64 edge-plane coverage,
// ray / plane depth).  The z-buffer is the output itself: filled with +inf bits, lowered by
// atomicMin on the (positive) fp32 bit pattern, +inf turned into 0 at the end — a min, so bit-identical run to run.
#include <math.h>

#include <algorithm>

#include "mesh_raster.hpp"
#include "scan.hpp"

namespace {
using namespace ep;
using namespace ep_raster;

// ----------------------------------------------------------------------------------------------- depth rasteriser
// (setup, coverage, depth and the two walks: mesh_raster.hpp, shared with the visibility buffer of mesh_render.hip)

struct DepthSink {
    unsigned *zbuf;
    int height, width;
    __device__ __forceinline__ void operator()(int view, int64_t, int r, int c, unsigned bits) const
    {
        unsigned *dst = zbuf + ((size_t)view * height + r) * width + c;
        if (bits < *dst) atomicMin(dst, bits);
    }
};

__global__ __launch_bounds__(256) void render_tri_kernel(RenderParams P) { raster_tri(P, DepthSink{P.zbuf, P.height, P.width}); }

// one wave per queued (view, triangle): its 64 lanes stride the pixel box
__global__ __launch_bounds__(256) void render_queue_kernel(RenderParams P) { raster_queue(P, DepthSink{P.zbuf, P.height, P.width}); }

__global__ __launch_bounds__(256) void render_finish_kernel(unsigned *zbuf, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && zbuf[i] == kInfBits) zbuf[i] = 0u;
}

// ----------------------------------------------------------------------------------------------- depth metrics

constexpr int kMetricSums = 10;
constexpr int kMetricSegments = 32;    // blocks per frame; their partials are added in segment order

__global__ __launch_bounds__(256) void depth_metrics_partial_kernel(const float *pred, const float *trgt, int64_t n_pix,
                                                                    double *partial)
{
    __shared__ double sh[kMetricSums][256];
    const int view = blockIdx.y, seg = blockIdx.x, tid = threadIdx.x;
    const int64_t per = (n_pix + kMetricSegments - 1) / kMetricSegments;
    const int64_t beg = seg * per, end = min(beg + per, n_pix);
    double acc[kMetricSums];
#pragma unroll
    for (int k = 0; k < kMetricSums; ++k) acc[k] = 0.0;
    const float *pp = pred + (size_t)view * n_pix, *tp = trgt + (size_t)view * n_pix;
    for (int64_t i = beg + tid; i < end; i += 256) {
        const float p = pp[i], t = tp[i];
        if (p > 0.0f) acc[1] += 1.0;
        if (p > 0.0f && t > 0.0f && t < 10.0f) {
            const double dp = p, dt = t;
            const double diff = fabs(dp - dt), sq = diff * diff, ld = log(dp) - log(dt);
            const double th = fmax(dt / dp, dp / dt);
            acc[0] += 1.0;
            acc[2] += diff / dt;
            acc[3] += diff;
            acc[4] += sq / dt;
            acc[5] += sq;
            acc[6] += ld * ld;
            acc[7] += th < 1.25 ? 1.0 : 0.0;
            acc[8] += th < 1.5625 ? 1.0 : 0.0;
            acc[9] += th < 1.953125 ? 1.0 : 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < kMetricSums; ++k) sh[k][tid] = acc[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int k = 0; k < kMetricSums; ++k) sh[k][tid] += sh[k][tid + s];
        }
        __syncthreads();
    }
    if (tid < kMetricSums) partial[((size_t)view * kMetricSegments + seg) * kMetricSums + tid] = sh[tid][0];
}

__global__ __launch_bounds__(256) void depth_metrics_final_kernel(const double *partial, int n_frames, double *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_frames * kMetricSums) return;
    const int view = i / kMetricSums, k = i % kMetricSums;
    double s = 0.0;
    for (int seg = 0; seg < kMetricSegments; ++seg) s += partial[((size_t)view * kMetricSegments + seg) * kMetricSums + k];
    out[i] = s;
}

// ----------------------------------------------------------------------------------------------- point bounds

constexpr int kBoundBlocks = 256;

__global__ __launch_bounds__(256) void bounds_partial_kernel(const float *pts, int64_t n, float *partial)
{
    __shared__ float sh[6][256];
    float m[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float v = pts[3 * (size_t)i + a];
            m[a] = fminf(m[a], v);
            m[3 + a] = fmaxf(m[3 + a], v);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) sh[k][threadIdx.x] = m[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
#pragma unroll
            for (int k = 0; k < 3; ++k) sh[k][threadIdx.x] = fminf(sh[k][threadIdx.x], sh[k][threadIdx.x + s]);
#pragma unroll
            for (int k = 3; k < 6; ++k) sh[k][threadIdx.x] = fmaxf(sh[k][threadIdx.x], sh[k][threadIdx.x + s]);
        }
        __syncthreads();
    }
    if (threadIdx.x < 6) partial[blockIdx.x * 6 + threadIdx.x] = sh[threadIdx.x][0];
}

__global__ void bounds_final_kernel(const float *partial, int nb, float *out)
{
    const int k = threadIdx.x;
    if (k >= 6) return;
    float m = partial[k];
    for (int b = 1; b < nb; ++b) m = k < 3 ? fminf(m, partial[6 * b + k]) : fmaxf(m, partial[6 * b + k]);
    out[k] = m;
}

// ----------------------------------------------------------------------------------------------- voxel down-sample

struct DownParams {
    const float *pts;
    int64_t n;
    double mb[3], voxel;
    int64_t dims[3];
    int64_t x0, x1;          // the x slab of this pass
};

// voxel of point i (open3d: floor((p - min_bound) / voxel)); false when outside this slab
__device__ __forceinline__ bool down_cell(const DownParams &P, int64_t i, int64_t idx[3], int64_t &cell)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double f = floor(((double)P.pts[3 * (size_t)i + a] - P.mb[a]) / P.voxel);
        if (!(f >= -1.0 && f < 9.0e15)) return false;     // (NaN, or far outside the index range)
        idx[a] = (int64_t)f;
    }
    if (idx[0] < P.x0 || idx[0] >= P.x1 || idx[1] < 0 || idx[1] >= P.dims[1] || idx[2] < 0 || idx[2] >= P.dims[2])
        return false;
    cell = ((idx[0] - P.x0) * P.dims[1] + idx[1]) * P.dims[2] + idx[2];
    return true;
}

__global__ __launch_bounds__(256) void down_count_kernel(DownParams P, int32_t *count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    int64_t idx[3], cell;
    if (down_cell(P, i, idx, cell)) atomicAdd(&count[cell], 1);
}

__global__ __launch_bounds__(256) void down_flag_kernel(const int32_t *count, int64_t cells, int32_t *flag)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < cells) flag[c] = count[c] > 0;
}

__global__ __launch_bounds__(256) void down_compact_kernel(const int32_t *count, const int32_t *slot, int64_t cells,
                                                           int32_t *cell_of_slot)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < cells && count[c] > 0) cell_of_slot[slot[c]] = (int32_t)c;
}

// The per-voxel sums are exact integer sums of fixed-point offsets from a reference point of the voxel (its smallest point
// index: independent of arrival order), 2^-36 voxel per step: |offset| < 1 voxel, so up to 2^27 points per voxel fit in
// int64, and a voxel whose points all coincide returns that point exactly.
constexpr double kFix = 68719476736.0;     // 2^36

__global__ __launch_bounds__(256) void down_ref_kernel(DownParams P, const int32_t *slot, int32_t *ref_index)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    int64_t idx[3], cell;
    if (down_cell(P, i, idx, cell)) atomicMin(&ref_index[slot[cell]], (int32_t)i);
}

__global__ __launch_bounds__(256) void down_sum_kernel(DownParams P, const int32_t *slot, const int32_t *ref_index,
                                                       unsigned long long *sums)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P.n) return;
    int64_t idx[3], cell;
    if (!down_cell(P, i, idx, cell)) return;
    const int64_t s = slot[cell], r = ref_index[s];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double off = (double)P.pts[3 * (size_t)i + a] - (double)P.pts[3 * (size_t)r + a];
        const long long q = llrint(off / P.voxel * kFix);
        atomicAdd(&sums[3 * s + a], (unsigned long long)q);    // two's complement: exact, order-free
    }
}

__global__ __launch_bounds__(256) void down_mean_kernel(DownParams P, const int32_t *count, const int32_t *cell_of_slot,
                                                        const int32_t *ref_index, const unsigned long long *sums, int64_t m,
                                                        float *out)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= m) return;
    const long long cnt = count[cell_of_slot[s]];
    const int64_t r = ref_index[s];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const long long sum = (long long)sums[3 * s + a];
        const double q = (double)(sum / cnt) + (double)(sum % cnt) / (double)cnt;
        out[3 * s + a] = (float)((double)P.pts[3 * (size_t)r + a] + q / kFix * P.voxel);
    }
}

// ----------------------------------------------------------------------------------------------- nearest neighbour

struct NnGrid {
    double lo[3], cell;
    int dims[3];
};

__device__ __forceinline__ int grid_coord(const NnGrid &G, double p, int a)
{
    const double f = floor((p - G.lo[a]) / G.cell);
    return (int)fmin(fmax(f, 0.0), (double)(G.dims[a] - 1));
}

__device__ __forceinline__ int64_t grid_cell(const NnGrid &G, const float *p)
{
    return ((int64_t)grid_coord(G, p[0], 0) * G.dims[1] + grid_coord(G, p[1], 1)) * G.dims[2] + grid_coord(G, p[2], 2);
}

__global__ __launch_bounds__(256) void nn_count_kernel(NnGrid G, const float *ref, int64_t n, int32_t *count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) atomicAdd(&count[grid_cell(G, ref + 3 * i)], 1);
}

__global__ __launch_bounds__(256) void nn_scatter_kernel(NnGrid G, const float *ref, int64_t n, int32_t *cursor, float4 *sorted)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int pos = atomicAdd(&cursor[grid_cell(G, ref + 3 * i)], 1);   // (order inside a cell: arbitrary, ties use the index)
    sorted[pos] = make_float4(ref[3 * i], ref[3 * i + 1], ref[3 * i + 2], __int_as_float((int)i));
}

__device__ __forceinline__ void nn_visit(const float4 *sorted, const int32_t *start, const int32_t *count, int64_t c, double qx,
                                         double qy, double qz, double &best, int &bi)
{
    const int b = start[c], e = b + count[c];
    for (int k = b; k < e; ++k) {
        const float4 p = sorted[k];
        const double dx = qx - (double)p.x, dy = qy - (double)p.y, dz = qz - (double)p.z;
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        const int id = __float_as_int(p.w);
        if (d2 < best || (d2 == best && id < bi)) {
            best = d2;
            bi = id;
        }
    }
}

__global__ __launch_bounds__(256) void nn_query_kernel(NnGrid G, const float4 *sorted, const int32_t *start, const int32_t *count,
                                                       const float *query, int64_t n_query, int64_t *idx_out, float *dist_out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_query) return;
    const double qx = query[3 * i], qy = query[3 * i + 1], qz = query[3 * i + 2];
    const int cx = grid_coord(G, qx, 0), cy = grid_coord(G, qy, 1), cz = grid_coord(G, qz, 2);
    const int rmax = max(max(max(cx, G.dims[0] - 1 - cx), max(cy, G.dims[1] - 1 - cy)), max(cz, G.dims[2] - 1 - cz));
    double best = INFINITY;
    int bi = 0x7fffffff;
    for (int r = 0; r <= rmax; ++r) {
        // shell r: the cells at Chebyshev distance r from the query's (clamped) cell, inside the grid
        const int x_lo = max(cx - r, 0), x_hi = min(cx + r, G.dims[0] - 1), y_lo = max(cy - r, 0), y_hi = min(cy + r, G.dims[1] - 1);
        for (int x = x_lo; x <= x_hi; ++x)
            for (int y = y_lo; y <= y_hi; ++y) {
                const int64_t row = ((int64_t)x * G.dims[1] + y) * G.dims[2];
                if (abs(x - cx) == r || abs(y - cy) == r) {
                    const int z_hi = min(cz + r, G.dims[2] - 1);
                    for (int z = max(cz - r, 0); z <= z_hi; ++z) nn_visit(sorted, start, count, row + z, qx, qy, qz, best, bi);
                } else {
                    if (cz - r >= 0) nn_visit(sorted, start, count, row + cz - r, qx, qy, qz, best, bi);
                    if (r > 0 && cz + r < G.dims[2]) nn_visit(sorted, start, count, row + cz + r, qx, qy, qz, best, bi);
                }
            }
        // every cell not yet visited lies outside the visited cube on some axis, i.e. in one of (up to) six slabs of the
        // grid box; no point in them is nearer than the nearest of those slab boxes (>= r * cell, and for a query outside
        // the grid box its whole distance to the box counts too).  No slab left: every cell has been visited.
        const int c[3] = {cx, cy, cz};
        const double q[3] = {qx, qy, qz};
        double lb2 = INFINITY;
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int k0 = side ? c[a] + r + 1 : 0, k1 = side ? G.dims[a] : c[a] - r;   // slab: cells [k0, k1) on axis a
                if (k0 >= k1) continue;
                double d2 = 0.0;
#pragma unroll
                for (int b = 0; b < 3; ++b) {
                    const double lo = G.lo[b] + (b == a ? (double)k0 : 0.0) * G.cell;
                    const double hi = G.lo[b] + (double)(b == a ? k1 : G.dims[b]) * G.cell;
                    const double e = q[b] < lo ? lo - q[b] : (q[b] > hi ? q[b] - hi : 0.0);
                    d2 += e * e;
                }
                lb2 = fmin(lb2, d2);
            }
        if (lb2 == INFINITY) break;
        // (a hair of slack for the rounding of the cell assignment; strict, so that an equal distance is still visited)
        const double lb = fmax(sqrt(lb2) - 1e-9 * G.cell, 0.0);
        if (best < lb * lb) break;
    }
    idx_out[i] = bi;
    dist_out[i] = (float)sqrt(best);
}

}  // namespace

extern "C" {

size_t eprecon_render_depth_workspace_bytes(int64_t queue_capacity) { return raster_workspace_bytes(queue_capacity); }

int eprecon_render_depth_async(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *cams,
                               int n_views, int height, int width, float pixel_center, float znear, float zfar, int cull_back,
                               float *depth_out, int64_t queue_capacity, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!depth_out || !workspace ||
        !raster_args_ok(verts, n_verts, faces, n_faces, cams, n_views, height, width, znear, zfar, queue_capacity))
        return EPRECON_ERR_ARG;
    if (workspace_bytes < eprecon_render_depth_workspace_bytes(queue_capacity)) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    RenderParams P{verts, faces, cams, n_verts, n_faces, n_views, height, width, pixel_center, znear, zfar, cull_back,
                   reinterpret_cast<unsigned *>(depth_out), reinterpret_cast<unsigned *>(ws),
                   reinterpret_cast<unsigned long long *>(ws + 256), queue_capacity};
    const int64_t n_pix = (int64_t)n_views * height * width;
    EP_HIP_CHECK(hipMemsetAsync(P.queue_count, 0, sizeof(unsigned), st));
    EP_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(depth_out), (int)kInfBits, (size_t)n_pix, st));
    if (n_faces > 0) {
        hipLaunchKernelGGL(render_tri_kernel, dim3((unsigned)ceil_div(n_faces, 256), (unsigned)n_views), dim3(256), 0, st, P);
        EP_LAUNCH_CHECK();
        hipLaunchKernelGGL(render_queue_kernel, dim3(2048), dim3(256), 0, st, P);
        EP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(render_finish_kernel, dim3((unsigned)ceil_div(n_pix, 256)), dim3(256), 0, st, P.zbuf, n_pix);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

size_t eprecon_depth_metrics_workspace_bytes(int n_frames)
{
    return align_up((size_t)(n_frames > 0 ? n_frames : 0) * kMetricSegments * kMetricSums * sizeof(double), 256);
}

int eprecon_depth_metrics_async(const float *pred, const float *trgt, int n_frames, int64_t n_pix, double *sums_out,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!pred || !trgt || !sums_out || !workspace || n_frames < 1 || n_frames > 65535 || n_pix < 1) return EPRECON_ERR_ARG;
    if (workspace_bytes < eprecon_depth_metrics_workspace_bytes(n_frames)) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(depth_metrics_partial_kernel, dim3(kMetricSegments, (unsigned)n_frames), dim3(256), 0, st, pred, trgt,
                       n_pix, partial);
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(depth_metrics_final_kernel, dim3((unsigned)ceil_div((int64_t)n_frames * kMetricSums, 256)), dim3(256), 0,
                       st, (const double *)partial, n_frames, sums_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_point_bounds_async(const float *points, int64_t n, float *out, float *workspace, void *stream)
{
    if (!points || n < 1 || !out || !workspace) return EPRECON_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int nb = (int)std::min<int64_t>(ceil_div(n, 256), kBoundBlocks);
    hipLaunchKernelGGL(bounds_partial_kernel, dim3(nb), dim3(256), 0, st, points, n, workspace);
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bounds_final_kernel, dim3(1), dim3(64), 0, st, (const float *)workspace, nb, out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

size_t eprecon_voxel_down_sample_workspace_bytes(int64_t n, int64_t slab_cells)
{
    if (n < 0 || slab_cells < 0) return 0;
    const size_t cseg = align_up((size_t)slab_cells * 4, 256);
    return 3 * cseg + scan_scratch_bytes(slab_cells) + 256 + 2 * align_up((size_t)n * 4, 256) +
           align_up((size_t)n * 24, 256);
}

int eprecon_voxel_down_sample(const float *points, int64_t n, const double *min_bound_host, double voxel,
                              const int64_t *dims_host, float *out, int64_t *n_out_host, int64_t slab_cells, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    if (!points || n < 1 || !min_bound_host || !(voxel > 0.0) || !dims_host || !out || !n_out_host || !workspace)
        return EPRECON_ERR_ARG;
    const int64_t plane = dims_host[1] * dims_host[2];
    if (dims_host[0] < 1 || dims_host[1] < 1 || dims_host[2] < 1 || plane > slab_cells || slab_cells > 0x7fffffffll ||
        n > 0x7fffffffll)
        return EPRECON_ERR_UNSUPPORTED;
    if (workspace_bytes < eprecon_voxel_down_sample_workspace_bytes(n, slab_cells)) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    const size_t cseg = align_up((size_t)slab_cells * 4, 256), sseg = scan_scratch_bytes(slab_cells);
    int32_t *count = reinterpret_cast<int32_t *>(ws), *flag = reinterpret_cast<int32_t *>(ws + cseg),
            *slot = reinterpret_cast<int32_t *>(ws + 2 * cseg), *scratch = reinterpret_cast<int32_t *>(ws + 3 * cseg),
            *total = reinterpret_cast<int32_t *>(ws + 3 * cseg + sseg),
            *cell_of_slot = reinterpret_cast<int32_t *>(ws + 3 * cseg + sseg + 256);
    int32_t *ref_index = reinterpret_cast<int32_t *>(ws + 3 * cseg + sseg + 256 + align_up((size_t)n * 4, 256));
    unsigned long long *sums =
        reinterpret_cast<unsigned long long *>(ws + 3 * cseg + sseg + 256 + 2 * align_up((size_t)n * 4, 256));
    DownParams P;
    P.pts = points;
    P.n = n;
    P.voxel = voxel;
    for (int a = 0; a < 3; ++a) {
        P.mb[a] = min_bound_host[a];
        P.dims[a] = dims_host[a];
    }
    const int64_t slab_x = std::max<int64_t>(1, slab_cells / plane);
    int64_t base = 0;
    for (int64_t x0 = 0; x0 < dims_host[0]; x0 += slab_x) {
        P.x0 = x0;
        P.x1 = std::min(x0 + slab_x, dims_host[0]);
        const int64_t cells = (P.x1 - P.x0) * plane;
        EP_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)cells * 4, st));
        hipLaunchKernelGGL(down_count_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, P, count);
        EP_LAUNCH_CHECK();
        hipLaunchKernelGGL(down_flag_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, st, (const int32_t *)count,
                           cells, flag);
        EP_LAUNCH_CHECK();
        int rc = ep::exclusive_scan_i32(flag, (int)cells, slot, scratch, total, st);
        if (rc != EPRECON_OK) return rc;
        int32_t m = 0;
        EP_HIP_CHECK(hipMemcpyAsync(&m, total, sizeof(m), hipMemcpyDeviceToHost, st));
        EP_HIP_CHECK(hipStreamSynchronize(st));
        if (m <= 0) continue;
        if (base + m > n) return EPRECON_ERR_UNSUPPORTED;    // (cannot happen: every voxel holds a point)
        EP_HIP_CHECK(hipMemsetAsync(sums, 0, (size_t)m * 24, st));
        EP_HIP_CHECK(hipMemsetAsync(ref_index, 0x7f, (size_t)m * 4, st));
        hipLaunchKernelGGL(down_compact_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, st, (const int32_t *)count,
                           (const int32_t *)slot, cells, cell_of_slot);
        EP_LAUNCH_CHECK();
        hipLaunchKernelGGL(down_ref_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, P, (const int32_t *)slot,
                           ref_index);
        EP_LAUNCH_CHECK();
        hipLaunchKernelGGL(down_sum_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, P, (const int32_t *)slot,
                           (const int32_t *)ref_index, sums);
        EP_LAUNCH_CHECK();
        hipLaunchKernelGGL(down_mean_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, P, (const int32_t *)count,
                           (const int32_t *)cell_of_slot, (const int32_t *)ref_index, (const unsigned long long *)sums,
                           (int64_t)m, out + 3 * base);
        EP_LAUNCH_CHECK();
        base += m;
    }
    EP_HIP_CHECK(hipStreamSynchronize(st));
    *n_out_host = base;
    return EPRECON_OK;
}

size_t eprecon_nn_search_workspace_bytes(int64_t n_ref, int64_t n_cells)
{
    if (n_ref < 0 || n_cells < 0) return 0;
    const size_t cseg = align_up((size_t)n_cells * 4, 256);
    return 3 * cseg + scan_scratch_bytes(n_cells) + 256 + align_up((size_t)n_ref * 16, 256);
}

int eprecon_nn_search_async(const float *ref, int64_t n_ref, const float *query, int64_t n_query, const double *lo_host,
                            double cell, const int32_t *dims_host, int64_t *idx_out, float *dist_out, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    if (!ref || n_ref < 1 || !query || n_query < 1 || !lo_host || !(cell > 0.0) || !dims_host || !idx_out || !dist_out ||
        !workspace)
        return EPRECON_ERR_ARG;
    if (dims_host[0] < 1 || dims_host[1] < 1 || dims_host[2] < 1 || n_ref > 0x7fffffffll) return EPRECON_ERR_UNSUPPORTED;
    const int64_t n_cells = (int64_t)dims_host[0] * dims_host[1] * dims_host[2];
    if (n_cells > 0x7fffffffll) return EPRECON_ERR_UNSUPPORTED;
    if (workspace_bytes < eprecon_nn_search_workspace_bytes(n_ref, n_cells)) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    const size_t cseg = align_up((size_t)n_cells * 4, 256), sseg = scan_scratch_bytes(n_cells);
    int32_t *count = reinterpret_cast<int32_t *>(ws), *start = reinterpret_cast<int32_t *>(ws + cseg),
            *cursor = reinterpret_cast<int32_t *>(ws + 2 * cseg), *scratch = reinterpret_cast<int32_t *>(ws + 3 * cseg),
            *total = reinterpret_cast<int32_t *>(ws + 3 * cseg + sseg);
    float4 *sorted = reinterpret_cast<float4 *>(ws + 3 * cseg + sseg + 256);
    NnGrid G;
    G.cell = cell;
    for (int a = 0; a < 3; ++a) {
        G.lo[a] = lo_host[a];
        G.dims[a] = dims_host[a];
    }
    EP_HIP_CHECK(hipMemsetAsync(count, 0, (size_t)n_cells * 4, st));
    hipLaunchKernelGGL(nn_count_kernel, dim3((unsigned)ceil_div(n_ref, 256)), dim3(256), 0, st, G, ref, n_ref, count);
    EP_LAUNCH_CHECK();
    int rc = ep::exclusive_scan_i32(count, (int)n_cells, start, scratch, total, st);
    if (rc != EPRECON_OK) return rc;
    EP_HIP_CHECK(hipMemcpyAsync(cursor, start, (size_t)n_cells * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(nn_scatter_kernel, dim3((unsigned)ceil_div(n_ref, 256)), dim3(256), 0, st, G, ref, n_ref, cursor, sorted);
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(nn_query_kernel, dim3((unsigned)ceil_div(n_query, 256)), dim3(256), 0, st, G, (const float4 *)sorted,
                       (const int32_t *)start, (const int32_t *)count, query, n_query, idx_out, dist_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
