// Ground-truth twin of the global map (models/gru_fusion.py:99-113, :206-213): one channel of TSDF, stored where |tsdf| < 1.
#include "global_map_common.hpp"

namespace {
using namespace ep;

__global__ void fill_f32_kernel(float *p, int n, float v)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}
// map rows inside the FBV -> dense volume; keep flags for the rows outside
__global__ void target_scatter_kernel(const int32_t *coords, const float *feat, int n, int D, int rx, int ry, int rz,
                                      float *vol, int32_t *keep)
{
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const int x = coords[3 * j] - rx, y = coords[3 * j + 1] - ry, z = coords[3 * j + 2] - rz;
    const bool inside = x >= 0 && x < D && y >= 0 && y < D && z >= 0 && z < D;
    keep[j] = inside ? 0 : 1;
    if (inside) vol[(x * D + y) * D + z] = feat[j];
}
// the current fragment's ground truth overwrites the map's; flag = |v| < 1 (what update_map stores)
__global__ void target_merge_kernel(const float *tsdf_gt, const uint8_t *occ_gt, int cells, float *vol, int32_t *flag)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    float v = vol[i];
    if (occ_gt[i]) {
        v = tsdf_gt[i];
        vol[i] = v;
    }
    flag[i] = fabsf(v) < 1.0f ? 1 : 0;
}
__global__ void target_lookup_kernel(const float *vol, const int32_t *updated, int n, int D, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = vol[(updated[3 * i] * D + updated[3 * i + 1]) * D + updated[3 * i + 2]];
}
// the same with the live length on the device: min(n_cap, *n_dev) (the queued GRU stage)
__global__ void target_lookup_dn_kernel(const float *vol, const int32_t *updated, int n_cap, const int32_t *n_dev, int D, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= min(n_cap, *n_dev)) return;
    out[i] = vol[(updated[3 * i] * D + updated[3 * i + 1]) * D + updated[3 * i + 2]];
}

}  // namespace

int ep::target_dense_queue(EpMap *tm, const float *tsdf_gt, const uint8_t *occ_gt, int dim, const int32_t *rel, const int32_t *updated,
                           int64_t n, const int32_t *n_dev, float *tsdf_target_out, int32_t *n_new_dev, int32_t *n_kept_dev,
                           hipStream_t st)
{
    const DenseView v = dense_view(tm, dim);
    const int cells = dim * dim * dim;
    for (int a = 0; a < 3; ++a) tm->rel[a] = rel[a];
    tm->pending_dim = dim;
    const dim3 blk(256), gcells((unsigned)ceil_div(cells, 256));
    if (tm->size > 0) {
        hipLaunchKernelGGL(target_scatter_kernel, dim3((unsigned)ceil_div(tm->size, 256)), blk, 0, st, (const int32_t *)tm->coords[tm->cur],
                           (const float *)tm->feats[tm->cur], (int)tm->size, dim, rel[0], rel[1], rel[2], v.vol, tm->keep);
        EP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(target_merge_kernel, gcells, blk, 0, st, tsdf_gt, occ_gt, cells, v.vol, v.flag);
    EP_LAUNCH_CHECK();
    if (n > 0) {
        const dim3 grows((unsigned)ceil_div(n, 256));
        if (n_dev)
            hipLaunchKernelGGL(target_lookup_dn_kernel, grows, blk, 0, st, (const float *)v.vol, updated, (int)n, n_dev, dim, tsdf_target_out);
        else
            hipLaunchKernelGGL(target_lookup_kernel, grows, blk, 0, st, (const float *)v.vol, updated, (int)n, dim, tsdf_target_out);
        EP_LAUNCH_CHECK();
    }
    int rc = exclusive_scan_i32(v.flag, cells, v.rank, tm->scan_scratch, n_new_dev, st);
    if (rc != EPRECON_OK) return rc;
    return exclusive_scan_i32(tm->keep, (int)tm->size, tm->keep_rank, tm->scan_scratch + tm->scratch_cap, n_kept_dev, st);
}

extern "C" {

int eprecon_map_target_fuse(void *handle, const float *tsdf_gt, const uint8_t *occ_gt, int dim,
                            const int32_t *relative_origin_host, const int32_t *updated, int64_t n, float *tsdf_target_out,
                            void *stream)
{
    EpMap *m = as_map(handle);
    if (!m || m->channels != 1 || !tsdf_gt || !occ_gt || dim <= 0 || dim > 512 || !relative_origin_host || n < 0 ||
        (n > 0 && (!updated || !tsdf_target_out)))
        return EPRECON_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const int cells = dim * dim * dim;
    int rc = ensure_crop(m, dim);
    if (rc != EPRECON_OK) return rc;
    hipLaunchKernelGGL(fill_f32_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, st, dense_view(m, dim).vol, cells, 1.0f);
    EP_LAUNCH_CHECK();
    rc = target_dense_queue(m, tsdf_gt, occ_gt, dim, relative_origin_host, updated, n, nullptr, tsdf_target_out, m->counts_dev,
                            m->counts_dev + 1, st);
    if (rc != EPRECON_OK) return rc;
    EP_HIP_CHECK(hipMemcpyAsync(m->counts_host, m->counts_dev, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EP_HIP_CHECK(hipStreamSynchronize(st));
    // (the stream is idle: the replace step's grow rule is the unconditional ensure_rows this call used to make)
    return map_replace_rows(m, m->size > 0 ? m->counts_host[1] : 0, m->counts_host[0], true, nullptr, nullptr, 0, st);
}

}  // extern "C"
