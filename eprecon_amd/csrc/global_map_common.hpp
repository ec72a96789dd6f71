// What the units of the persistent global map share (global_map.hip and its _exchange / _target / _stage siblings).
// A kernel lives in ONE unit; the host steps below are hidden and the inline helpers static, so `nm -D` shows none of this.
#pragma once

#include "scan.hpp"

#define EP_MAP_LOCAL __attribute__((visibility("hidden")))

namespace ep {

// EpMap::kept while no row count of a crop is at hand (a count is >= 0)
constexpr int64_t kNoCrop = -1;       // no crop since the last update / import / merge
constexpr int64_t kCropPending = -2;  // eprecon_gru_stage_begin_async queued one; its count is still on the device

struct EpMap {
    int channels = 0;
    int64_t size = 0, cap = 0;
    int32_t *coords[2] = {nullptr, nullptr};  // [cap,3] scene-grid voxel units of this scale
    float *feats[2] = {nullptr, nullptr};     // [cap,channels]
    int cur = 0;
    int32_t *keep = nullptr, *keep_rank = nullptr;  // [row_cap] 1 = row outside the last crop's FBV; its scan
    int64_t row_cap = 0;
    int32_t *scan_scratch = nullptr;  // [2][scratch_cap]: one half per scan of a crop
    int64_t scratch_cap = 0;
    int32_t *counts_dev = nullptr;  // [4]
    int32_t *counts_host = nullptr;  // pinned [4]
    char *dense = nullptr;  // dense FBV workspace: see dense_view
    size_t dense_bytes = 0;
    int64_t kept = kNoCrop;  // rows outside the FBV of the last crop, or kNoCrop / kCropPending
    int pending_dim = 0;  // grid size of the twin's last dense pass (target_dense_queue -> map_replace_rows)
    int rel[3] = {0, 0, 0};
    // multi-GPU boundary exchange: per row, which fragment produced its features and whether THIS rank
    // fused it: 0 unknown, +(fragment + 1) fused here, -(fragment + 1) received from another rank
    int32_t *stamps[2] = {nullptr, nullptr};  // [cap], allocated with the rows
    int fuse_stamp = 0;                       // what eprecon_map_update_async writes for the rows it appends
    int32_t *sel = nullptr, *sel_rank = nullptr, *sel_aux = nullptr;  // [sel_cap] selection flags of the exchange, their scan, merge scratch
    int64_t sel_cap = 0;
    int32_t *sel_scratch = nullptr;
    int64_t sel_scratch_cap = 0;
    int64_t n_selected = -1;
};

static inline EpMap *as_map(void *h) { return reinterpret_cast<EpMap *>(h); }

// m->dense for a dim^3 volume: five 256-byte-aligned segments of dense_seg(dim) bytes
static inline size_t dense_seg(int dim) { return align_up((size_t)dim * dim * dim * 4, 256); }
struct DenseView {
    int32_t *idx_cur, *idx_glob;  // row of the fragment / of the map in a cell, -1 = none
    int32_t *flag, *rank;         // the cell is in the union (the twin: is stored); the flags' scan
    float *vol;                   // the twin's dense TSDF volume
    size_t seg;
};
static inline DenseView dense_view(const EpMap *m, int dim)   // after ensure_dense(m, dim)
{
    const size_t seg = dense_seg(dim);
    char *d = m->dense;
    return DenseView{reinterpret_cast<int32_t *>(d), reinterpret_cast<int32_t *>(d + seg), reinterpret_cast<int32_t *>(d + 2 * seg),
                     reinterpret_cast<int32_t *>(d + 3 * seg), reinterpret_cast<float *>(d + 4 * seg), seg};
}

// storage (global_map.hip).  Each may reallocate: the stream must not be reading what it frees.
EP_MAP_LOCAL int ensure_rows(EpMap *m, int64_t rows);
EP_MAP_LOCAL int ensure_dense(EpMap *m, int dim);
EP_MAP_LOCAL int ensure_crop(EpMap *m, int dim);   // ensure_dense + the keep flags and scan scratch for a crop of the current rows
EP_MAP_LOCAL int ensure_sel(EpMap *m, int64_t rows);
// crop + union (global_map.hip): scatter, two scans, emit; sets m->rel.  The caller clears the volumes and owns the host read and m->kept.
EP_MAP_LOCAL int map_crop_queue(EpMap *m, const int32_t *cur_coords, const float *cur_feat, int64_t n_cur, int ld_cur, int dim,
                                int interval, int mode, const int32_t *rel, int32_t *n_union_dev, int32_t *n_kept_dev,
                                int32_t *updated, int32_t *src_cur, int32_t *src_glob, hipStream_t st);
// map = map[keep] ++ n_new rows (global_map.hip): grow, compact, append (twin: the flagged cells of its volume, else the values), flip
EP_MAP_LOCAL int map_replace_rows(EpMap *m, int64_t kept, int64_t n_new, bool twin, const int32_t *updated, const float *values,
                                  int ld_values, hipStream_t st);
// the twin's dense pass (global_map_target.hip) on a volume filled with 1.0; n_dev == nullptr: n is the count, else min(n, *n_dev)
EP_MAP_LOCAL int target_dense_queue(EpMap *tm, const float *tsdf_gt, const uint8_t *occ_gt, int dim, const int32_t *rel,
                                    const int32_t *updated, int64_t n, const int32_t *n_dev, float *tsdf_target_out,
                                    int32_t *n_new_dev, int32_t *n_kept_dev, hipStream_t st);

}  // namespace ep
