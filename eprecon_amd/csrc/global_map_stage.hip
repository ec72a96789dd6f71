// One GRU-fusion level queued as ONE call with device-side counts (include/eprecon_hip.h: eprecon_gru_stage_desc).
#include "global_map_common.hpp"
#include "hashgrid.hpp"

namespace {
using namespace ep;

// [h | x] buffers of the two ConvGRUs of a scale in one pass: h = the map's row, x = the fragment's row (zeros where absent),
// channels [0, chv) to the voxel cell, [chv, C) to the image cell.  The union size lives on the device.
__global__ __launch_bounds__(256) void stage_gather_kernel(const float *map_feat, const float *cur_feat, int ld_cur,
                                                           const int32_t *src_glob, const int32_t *src_cur, int n_cap,
                                                           const int32_t *n_dev, int C, int chv, float *hx_v, float *hx_i)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int n = min(n_cap, *n_dev);
    if (e >= (int64_t)n * C) return;
    const int i = (int)(e / C), c = (int)(e - (int64_t)i * C);
    const int jg = src_glob[i], jc = src_cur[i];
    const float h = jg >= 0 ? map_feat[(size_t)jg * C + c] : 0.0f;
    const float x = jc >= 0 ? cur_feat[(size_t)jc * ld_cur + c] : 0.0f;
    const int chi = C - chv;
    if (c < chv) {
        hx_v[(size_t)i * 2 * chv + c] = h;
        hx_v[(size_t)i * 2 * chv + chv + c] = x;
    } else {
        hx_i[(size_t)i * 2 * chi + (c - chv)] = h;
        hx_i[(size_t)i * 2 * chi + chi + (c - chv)] = x;
    }
}
// union cells -> voxel coordinates of the fragment (batch, cell * interval) and their aligned-camera coordinates
// (models/gru_fusion.py:332-337; the arithmetic of aligned_coords_kernel, csrc/voxelize.hip: separate multiply / add, then the
// k-ordered fma chain of the [N,4] x [4,3] product); the batch column of the points is 0 like the reference's
__global__ void stage_points_kernel(const int32_t *updated, int n_cap, const int32_t *n_dev, int interval, int batch_index,
                                    const float *origin, float vs, const float *w2ac, int4 *out_coords, float4 *r_coords)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= min(n_cap, *n_dev)) return;
    const int cx = updated[3 * i] * interval, cy = updated[3 * i + 1] * interval, cz = updated[3 * i + 2] * interval;
    out_coords[i] = make_int4(batch_index, cx, cy, cz);
    const float X = __fadd_rn(__fmul_rn((float)cx, vs), origin[0]);
    const float Y = __fadd_rn(__fmul_rn((float)cy, vs), origin[1]);
    const float Z = __fadd_rn(__fmul_rn((float)cz, vs), origin[2]);
    float r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        r[j] = __fmaf_rn(1.0f, w2ac[4 * j + 3], __fmaf_rn(Z, w2ac[4 * j + 2], __fmaf_rn(Y, w2ac[4 * j + 1], __fmul_rn(X, w2ac[4 * j]))));
    r_coords[i] = make_float4(r[0], r[1], r[2], 0.0f);
}
// ... and, in the same launch, the two voxelisations' coordinate side (point_quantize_kernel twice, csrc/voxelize.hip: IEEE division
// by the resolution, floor; the second one on the ALREADY-SCALED points — ConvGRU's convr, models/modules.py:216-217)
__global__ void stage_points_quantize_kernel(const int32_t *updated, int n_cap, const int32_t *n_dev, int interval, int batch_index,
                                             const float *origin, float vs, const float *w2ac, float res, int4 *out_coords,
                                             float4 *r_coords, float4 *scaled1, int4 *vox1, float4 *scaled2, int4 *vox2)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= min(n_cap, *n_dev)) return;
    const int cx = updated[3 * i] * interval, cy = updated[3 * i + 1] * interval, cz = updated[3 * i + 2] * interval;
    out_coords[i] = make_int4(batch_index, cx, cy, cz);
    const float X = __fadd_rn(__fmul_rn((float)cx, vs), origin[0]);
    const float Y = __fadd_rn(__fmul_rn((float)cy, vs), origin[1]);
    const float Z = __fadd_rn(__fmul_rn((float)cz, vs), origin[2]);
    float r[3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
        r[j] = __fmaf_rn(1.0f, w2ac[4 * j + 3], __fmaf_rn(Z, w2ac[4 * j + 2], __fmaf_rn(Y, w2ac[4 * j + 1], __fmul_rn(X, w2ac[4 * j]))));
    r_coords[i] = make_float4(r[0], r[1], r[2], 0.0f);
    const float x1 = __fdiv_rn(r[0], res), y1 = __fdiv_rn(r[1], res), z1 = __fdiv_rn(r[2], res);
    scaled1[i] = make_float4(x1, y1, z1, 0.0f);
    vox1[i] = make_int4(0, (int)floorf(x1), (int)floorf(y1), (int)floorf(z1));
    const float x2 = __fdiv_rn(x1, res), y2 = __fdiv_rn(y1, res), z2 = __fdiv_rn(z1, res);
    scaled2[i] = make_float4(x2, y2, z2, 0.0f);
    vox2[i] = make_int4(0, (int)floorf(x2), (int)floorf(y2), (int)floorf(z2));
}

// the argument checks of eprecon_gru_stage_begin_async, in front of everything it queues or allocates
int stage_validate(const eprecon_gru_stage_desc *d)
{
    if (!d || !d->map || d->n_cur < 0 || d->dim <= 0 || d->dim > 512 || d->interval <= 0 || d->capacity <= 0 || !d->updated ||
        !d->out_coords || !d->r_coords || !d->hx_voxel || !d->hx_image || !d->counts || !d->origin || !d->w2ac || !d->workspace ||
        !(d->resolution > 0.0f) || !d->scaled1 || !d->vox1 || !d->inverse1 || !d->uniq1 || !d->table1 || !d->scaled2 || !d->vox2 ||
        !d->inverse2 || !d->uniq2 || !d->table2)
        return EPRECON_ERR_ARG;
    const EpMap *m = as_map(d->map), *tm = as_map(d->target_map);
    const int C = m->channels;
    if (d->ch_voxel <= 0 || d->ch_voxel >= C || (d->n_cur > 0 && (!d->cur_coords || !d->cur_feat || d->ld_cur < C))) return EPRECON_ERR_ARG;
    if (d->capacity < eprecon_gru_stage_capacity(d->map, d->n_cur, d->dim)) return EPRECON_ERR_ARG;
    if (d->workspace_bytes < eprecon_gru_stage_workspace_bytes(d->capacity)) return EPRECON_ERR_WORKSPACE;
    if (tm && (tm->channels != 1 || !d->tsdf_gt || !d->occ_gt || !d->tsdf_target)) return EPRECON_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(d->counts) & 15) != 0) return EPRECON_ERR_ARG;
    return EPRECON_OK;
}

}  // namespace

extern "C" {

int64_t eprecon_gru_stage_capacity(const void *map, int64_t n_cur, int dim)
{
    const EpMap *m = reinterpret_cast<const EpMap *>(map);
    if (!m || n_cur < 0 || dim <= 0) return -1;
    const int64_t cells = (int64_t)dim * dim * dim;
    const int64_t cap = n_cur + m->size < cells ? n_cur + m->size : cells;
    return cap > 0 ? cap : 1;
}

size_t eprecon_gru_stage_workspace_bytes(int64_t capacity)
{
    const int64_t cap = capacity > 0 ? capacity : 1;
    return 2 * align_up((size_t)cap * sizeof(int32_t), 256) + eprecon_unique_workspace_bytes(cap);
}

int eprecon_gru_stage_begin_async(const eprecon_gru_stage_desc *d, void *stream)
{
    int rc = stage_validate(d);
    if (rc != EPRECON_OK) return rc;
    EpMap *m = as_map(d->map), *tm = as_map(d->target_map);
    const int C = m->channels;
    hipStream_t st = (hipStream_t)stream;
    const int dim = d->dim, cap = (int)d->capacity;
    rc = ensure_crop(m, dim);
    if (rc != EPRECON_OK) return rc;
    char *ws = reinterpret_cast<char *>(d->workspace);
    const size_t iseg = align_up((size_t)cap * sizeof(int32_t), 256);
    int32_t *src_cur = reinterpret_cast<int32_t *>(ws);
    int32_t *src_glob = reinterpret_cast<int32_t *>(ws + iseg);
    void *uws = ws + 2 * iseg;
    const size_t uws_bytes = d->workspace_bytes - 2 * iseg;
    int32_t *cnt = d->counts;

    // --- everything the call has to reset, in ONE launch: the counters, the two index volumes (-1) and the flag volume (0) of the
    //     crop, the ground-truth twin's dense volume (1.0) and the two hash tables of the shared voxelisations ---
    {
        const DenseView v = dense_view(m, dim);
        ep::FillRegion reg[ep::kMaxFillRegions];
        int nr = 0;
        reg[nr++] = ep::FillRegion{cnt, 8 * sizeof(int32_t), 0u};
        reg[nr++] = ep::FillRegion{v.idx_cur, 2 * v.seg, 0xFFFFFFFFu};
        reg[nr++] = ep::FillRegion{v.flag, v.seg, 0u};
        if (tm) {
            rc = ensure_crop(tm, dim);
            if (rc != EPRECON_OK) return rc;
            reg[nr++] = ep::FillRegion{dense_view(tm, dim).vol, v.seg, 0x3f800000u};   // 1.0f (the whole 256-byte-aligned segment)
        }
        for (void *table : {d->table1, d->table2}) {
            rc = ep::table_clear_regions(table, d->table_capacity, reg + nr);
            if (rc != EPRECON_OK) return rc;
            nr += 3;
        }
        rc = ep::multi_fill(reg, nr, st);
        if (rc != EPRECON_OK) return rc;
    }

    // --- crop + union (the kernels of eprecon_map_crop_union, without its host read) ---
    rc = map_crop_queue(m, d->cur_coords, d->cur_feat, d->n_cur, d->ld_cur, dim, d->interval, d->activity_mode, d->rel, cnt + 0, cnt + 1,
                        d->updated, src_cur, src_glob, st);
    if (rc != EPRECON_OK) return rc;
    m->kept = kCropPending;   // eprecon_gru_stage_commit_async supplies the count the host read
    const int32_t *n_u = cnt + 0;

    // --- [h | x] rows of the two cells ---
    hipLaunchKernelGGL(stage_gather_kernel, dim3((unsigned)ceil_div((int64_t)cap * C, 256)), dim3(256), 0, st,
                       (const float *)m->feats[m->cur], d->cur_feat, d->ld_cur, (const int32_t *)src_glob, (const int32_t *)src_cur, cap,
                       n_u, C, d->ch_voxel, d->hx_voxel, d->hx_image);
    EP_LAUNCH_CHECK();

    // --- ground-truth twin: dense volume (1.0 since the first launch) <- map rows in the FBV <- ground truth; targets at the union ---
    if (tm) {
        rc = target_dense_queue(tm, d->tsdf_gt, d->occ_gt, dim, d->rel, d->updated, cap, n_u, d->tsdf_target, cnt + 4, cnt + 5, st);
        if (rc != EPRECON_OK) return rc;
        tm->kept = kCropPending;
    }

    // --- the fragment's points and the two voxelisations the six SConv3d of the scale share ---
    // (one launch for the points and both quantisations; the tables were reset by the call's first launch; each numbering's
    // last launch leaves its table's status word next to the counts: one host read for everything)
    hipLaunchKernelGGL(stage_points_quantize_kernel, dim3((unsigned)ceil_div(cap, 256)), dim3(256), 0, st, (const int32_t *)d->updated,
                       cap, n_u, d->interval, d->batch_index, d->origin, d->voxel_size, d->w2ac, d->resolution,
                       reinterpret_cast<int4 *>(d->out_coords), reinterpret_cast<float4 *>(d->r_coords), reinterpret_cast<float4 *>(d->scaled1),
                       reinterpret_cast<int4 *>(d->vox1), reinterpret_cast<float4 *>(d->scaled2), reinterpret_cast<int4 *>(d->vox2));
    EP_LAUNCH_CHECK();
    rc = ep::unique_coords_dn(d->vox1, cap, n_u, 1, d->table1, d->table_capacity, d->inverse1, d->uniq1, cnt + 2, uws, uws_bytes,
                              true, cnt + 6, stream);
    if (rc != EPRECON_OK) return rc;
    return ep::unique_coords_dn(d->vox2, cap, n_u, 1, d->table2, d->table_capacity, d->inverse2, d->uniq2, cnt + 3, uws, uws_bytes, true,
                                cnt + 7, stream);
}

int eprecon_gru_stage_commit_async(void *map, void *target_map, const int32_t *counts_host, void *stream)
{
    EpMap *m = as_map(map), *tm = as_map(target_map);
    if (!m || !counts_host || m->kept != kCropPending) return EPRECON_ERR_ARG;
    if (counts_host[1] < 0 || counts_host[1] > m->size) return EPRECON_ERR_ARG;
    m->kept = counts_host[1];
    if (!tm) return EPRECON_OK;
    if (tm->kept != kCropPending) return EPRECON_ERR_ARG;
    const int64_t n_new = counts_host[4], kept = tm->size > 0 ? counts_host[5] : 0;
    if (n_new < 0 || kept < 0 || kept > tm->size) return EPRECON_ERR_ARG;
    return map_replace_rows(tm, kept, n_new, true, nullptr, nullptr, 0, (hipStream_t)stream);
}

}  // extern "C"
