// Multi-view back-projection for gfx950 (MI355X): image-feature pyramid -> voxel list.  This unit is the host side: one call
// descriptor (eprecon_bp_call, include/eprecon_hip.h) is validated, planned and queued; the device code is
// back_project_count.hpp (BpParams, count, scan, re-layout, prepare, levels) and back_project_gather.hpp (the two gather
// kernels, depth normalisation), which only this unit includes.
//
// Replaces Back_Project.forward (models/occupancy_initialization.py:189-261 of the reference),
// ops/back_project.py:5-80 and the sample + mean/variance block of
// Occupancy_Initialization.forward (models/occupancy_initialization.py:79-128).
//
// Pipeline per call (all on the caller's stream): prepare -> gather on NCHW maps, count -> gather on channels-last maps
//   bp_prepare       one grid, two independent halves behind a block-uniform branch:
//                    re-layout of the V*B feature maps to channels-last, so that the C channels of one bilinear tap are
//                    one contiguous 4*C-byte run (no such blocks when the caller already holds channels-last maps:
//                    then the launch is bp_count alone);
//                    count, one thread per voxel: 9 projections, visible-view count (float, all N), per-tile valid
//                    totals by wave ballot + popcount, per-batch valid counts;
//   bp_gather        prologue: the output row of the tile = sum of the tile totals in front of it (tile_base; the
//                    workgroup of the last tile publishes n_valid).  Lists of more than EPRECON_BP_FOLD tiles get a
//                    bp_scan launch in front instead (exclusive scan of the totals, one workgroup);
//                    phase 1, one thread per voxel: re-project, stable in-block compaction by
//                    ballot/prefix-sum, pixel coordinates of every (voxel, view) staged in LDS;
//                    phase 2, one thread per (valid voxel, 4-channel group): bilinear gather of
//                    the visible views with 16-byte loads, mean (or two-sweep variance) in
//                    registers, fully coalesced 16-byte stores in compacted order.
//   [bp_depth_norm]  ops.back_project's extra normalised-depth channel.
//
// Roofline: HBM/L2 bandwidth (about 2 flop per gathered byte).  Algorithmic bytes per call
//   16 N (coords in) + 4 N (count out) + 4 V C H W (maps, once) + n_valid (4 C + 16) (rows out).
// Arithmetic contract (bit-exact indices): see oracle/c/back_project_oracle.c and DESIGN.md.
#include <stdlib.h>

#include "back_project_gather.hpp"

namespace {

// Tiles up to which the scan is folded into the gather (tile_base).  >= 3,456 (dense 96^3 at 256 voxels); the sweep of list
// lengths behind the figure is profiles/r12/fold_cap.txt.  tests/test_back_project_launches_gpu.py restates the
// figure (DEFAULT_CAP) and reads the tile totals at offset 0 of the workspace: change them together.
constexpr int kFoldCapDefault = 6144;

// dynamic LDS of a gather workgroup: 12 (mlp: two weights and an offset) or 8 (pixel coordinates) bytes per (voxel, view), the
// matrices, 3 or 5 words per voxel, sWave and sFold
size_t gather_lds_bytes(bool mlp, int vox, int V, int B)
{
    const size_t nP = ((size_t)V * B * 12 + 3) & ~(size_t)3;
    return (size_t)vox * V * (mlp ? 12 : 8) + nP * 4 + (size_t)vox * (mlp ? 3 : 5) * 4 + (size_t)(256 / kWave) * 4 * 3;
}

// QT, the channel groups of four per voxel: the model's widths at compile time (C = 24: 1/4-res level, 32: fused initialisation
// maps, 40: 1/8-res, 80: 1/16-res), any other at run time; C % 4 != 0 takes the scalar kernel.  mlp: U = 1 (2 / 3 / 4 views of
// loads in flight per lane: slower, see back_project_gather.hpp).
template <int VOX, int MODE>
int launch_gather(const BpParams &p, bool mlp, hipStream_t st)
{
    const size_t lds = gather_lds_bytes(mlp, VOX, p.V, p.batch);
    const dim3 grid(p.ntile), block(256);
    if (p.C % 4 != 0) {
        hipLaunchKernelGGL((bp_gather_kernel<VOX, MODE, 1, 0>), grid, block, lds, st, p);
    } else {
        pick<6, 8, 10, 20, 0>(p.C / 4, [&](auto qt) {
            constexpr int QT = decltype(qt)::value;
            if (mlp) hipLaunchKernelGGL((bp_gather_mlp_kernel<VOX, MODE, QT, 1>), grid, block, lds, st, p);
            else hipLaunchKernelGGL((bp_gather_kernel<VOX, MODE, 4, QT>), grid, block, lds, st, p);
            return 0;
        });
    }
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// The workspace of a call, as byte offsets: the tile totals (one int32 per 16 voxels) at 0, the count workgroups' per-batch rows
// (one int32 per 256 voxels and batch element) at `rows`, the channels-last copy of NCHW maps at `maps`, `end` behind them.
// bp_plan and the two exported size functions all come here.
struct BpCarve {
    size_t rows, maps, end;
};

BpCarve bp_carve(int64_t n, int batch, size_t map_bytes)
{
    BpCarve c;
    c.rows = ep::align_up((size_t)ep::ceil_div(n, 16) * sizeof(int32_t), 256);
    c.maps = c.rows + ep::align_up((size_t)ep::ceil_div(n, 256) * batch * sizeof(int32_t), 256);
    c.end = c.maps + ep::align_up(map_bytes, 256);
    return c;
}

// What a descriptor is validated as: the whole call or one of its halves (the values of eprecon_bp_call::phase), or a level of
// eprecon_back_project_prepare_levels_async with a list (a count half for maps of either layout) or without one (coords ==
// NULL: its maps are re-laid out into the workspace, where a list of n entries leaves them; neither counters nor matrices).
enum BpRole { kBpWhole = 0, kBpCountHalf = EPRECON_BP_COUNT, kBpGatherHalf = EPRECON_BP_GATHER, kBpLevelList, kBpLevelMaps };

// Order of the checks (the first fault decides): layout, a half on NCHW maps, rank with several batch elements, sizes and
// mode, pointers (all EPRECON_ERR_ARG); the matrix table (UNSUPPORTED); the workspace (WORKSPACE); the maps' size (UNSUPPORTED).
int bp_validate(const eprecon_bp_call &a, BpRole role)
{
    const bool listed = role != kBpLevelMaps;                          // there is a list: coordinates, matrices, counters
    const bool rows = role == kBpWhole || role == kBpGatherHalf;       // output rows are written (and rank, when given)
    const bool nhwc = a.feats_layout == EPRECON_LAYOUT_NHWC;
    if (a.feats_layout != EPRECON_LAYOUT_NCHW && !nhwc) return EPRECON_ERR_ARG;
    if ((role == kBpCountHalf || role == kBpGatherHalf) && !nhwc) return EPRECON_ERR_ARG;   // (NCHW: re-layout and count are one grid)
    if (rows && a.rank && a.batch != 1) return EPRECON_ERR_ARG;        // (the rows of several batch elements interleave: no single raster)
    if (a.n < 0 || a.n > 0x7fffffff / 64 || a.batch <= 0 || a.n_views <= 0 || a.n_views > 32 || a.channels <= 0 ||
        a.height <= 1 || a.width <= 1 || a.mode < 0 || a.mode > 2)
        return EPRECON_ERR_ARG;
    if (!a.workspace || (!a.feats && !(listed && !rows && nhwc))) return EPRECON_ERR_ARG;   // (a count reads no channels-last maps)
    if (listed && (!a.origin || !a.krcam || !a.n_valid_dev)) return EPRECON_ERR_ARG;
    if (listed && a.n > 0 && (!a.coords || !a.count || (rows && (!a.out_feats || !a.out_coords)))) return EPRECON_ERR_ARG;
    // a count mailbox: there has to be a publisher (a list with entries), a sequence number, and room for 1 + B words
    if (a.counts_host && (!listed || a.n == 0 || a.counts_seq == 0 || 1 + a.batch > EPRECON_MAILBOX_WORDS)) return EPRECON_ERR_ARG;
    if ((size_t)a.n_views * a.batch * 12 * sizeof(float) > 32 * 1024) return EPRECON_ERR_UNSUPPORTED;
    if (a.workspace_bytes < eprecon_back_project_workspace_bytes(a.n, a.batch, a.n_views, a.channels, a.height, a.width,
                                                                 a.feats_layout))
        return EPRECON_ERR_WORKSPACE;
    if ((size_t)a.n_views * a.batch * a.channels * a.height * a.width > 0x7fffffffull) return EPRECON_ERR_UNSUPPORTED;
    return EPRECON_OK;
}

// Every decision of a call, taken once: the two switches, the tile, the launch chain, the workspace carve, the kernel arguments.
struct BpPlan {
    bool nchw, chain4, clear_in_relayout, mlp;   // mlp: bp_gather_mlp_kernel (else bp_gather_kernel)
    int vox, ntile, nblk_count;                  // (the scan is folded into the gather where p.fold is set)
    size_t lds_relayout, lds_count;
    int32_t *tile_sums, *blk_batch;              // workspace (bp_carve): tile totals, the per-batch rows (null for one batch
    float *nhwc;                                 // element), the channels-last maps of an NCHW call
    BpParams p;
};

BpPlan bp_plan(const eprecon_bp_call &a)
{
    BpPlan pl;
    const int64_t n = a.n;
    pl.nchw = a.feats_layout == EPRECON_LAYOUT_NCHW;
    // EPRECON_BP_FOLD (read per call): the largest tile count at which the gather workgroups sum the tile totals themselves
    // (tile_base) instead of a scan launch between count and gather.  Unset: kFoldCapDefault; N > 0: N tiles; 0: the chain of
    // four dependent launches as it was -- re-layout (clearing the counters), count, scan, gather.  Same results every way.
    int fold_cap = kFoldCapDefault;
    if (const char *e = getenv("EPRECON_BP_FOLD"); e && e[0]) {
        const long v = strtol(e, nullptr, 10);
        fold_cap = v <= 0 ? 0 : (v > 0x7fffffffL ? 0x7fffffff : (int)v);
    }
    pl.chain4 = fold_cap == 0;
    // The counters: every word of n_valid_dev[0 .. B] is written by the scan launch or by the gather's last workgroup, so only
    // the empty list needs them cleared.  (The four-launch chain clears them as it always did: inside the re-layout launch when
    // there is one -- NCHW features, <= 255 batch elements -- else by a memset.)
    pl.clear_in_relayout = pl.chain4 && n > 0 && pl.nchw && a.batch < 256;

    char *ws = reinterpret_cast<char *>(a.workspace);
    const BpCarve carve = bp_carve(n, a.batch, 0);
    pl.tile_sums = reinterpret_cast<int32_t *>(ws);
    pl.blk_batch = a.batch > 1 ? reinterpret_cast<int32_t *>(ws + carve.rows) : nullptr;
    pl.nhwc = reinterpret_cast<float *>(ws + carve.maps);
    pl.lds_relayout = (size_t)a.channels * (kTrPix + 1) * sizeof(float);
    pl.lds_count = ((size_t)a.n_views * a.batch * 12 + a.batch + 256 / ep::kWave) * 4 + 16;

    BpParams &p = pl.p;
    p.coords = a.coords; p.n = (int)n; p.origin = a.origin; p.batch = a.batch; p.voxel_size = a.voxel_size;
    p.feats_nhwc = pl.nchw ? pl.nhwc : a.feats; p.krcam = a.krcam;
    p.V = a.n_views; p.C = a.channels; p.Cs = a.channels; p.H = a.height; p.W = a.width;
    p.min_view = a.min_view; p.out_feats = a.out_feats; p.out_mean = a.out_mean; p.out_coords = a.out_coords;
    p.count = a.count; p.out_grid = a.out_grid; p.out_mask = a.out_mask; p.n_valid_dev = a.n_valid_dev;
    p.block_offsets = pl.tile_sums;
    p.rank = a.phase == EPRECON_BP_COUNT ? nullptr : a.rank;   // (the count half writes no rows)
    p.counts_host = a.counts_host; p.counts_seq = a.counts_seq;
    // EPRECON_BP_XCD_SLABS=0 (read per call): the gather's tiles in hardware block order — round-robin over the eight XCDs, so
    // every XCD's L2 sees tiles from the whole volume — instead of one contiguous slab of the raster per XCD.  Same results.
    p.xcd_slabs = ep::switch_off("EPRECON_BP_XCD_SLABS") ? 0 : 1;
    pl.mlp = p.C % 4 == 0 && p.Cs % 4 == 0 && p.V <= 32 && (size_t)p.V * p.batch * p.H * p.W * p.Cs * 4 < 0x7fff0000ull &&
             gather_lds_bytes(true, 256, p.V, p.batch) <= dynamic_lds_limit();

    // Tile = voxels handed to one 256-thread workgroup of the gather kernel.  Short lists get
    // small tiles so that the launch still covers the 256 CUs with several waves each
    // (13,824 voxels -> 864 workgroups of 16; 110,592 -> 1,728 of 64).
    pl.vox = n >= 512 * 1024 ? 256 : (n >= 48 * 1024 ? 64 : 16);
    // bp_gather_kernel<256> stages 8 bytes per (voxel, view): more than a workgroup may have from 29 views on (65,952 bytes at
    // V = 29, B = 1).  Such a list takes the 64-voxel tile instead (17,664 bytes at V = 32); decided before any launch, because the
    // count kernel's tile totals must match the gather's tile.
    if (pl.vox == 256 && !pl.mlp && gather_lds_bytes(false, 256, a.n_views, a.batch) > dynamic_lds_limit()) pl.vox = 64;
    pl.ntile = (int)ep::ceil_div(n, pl.vox);
    pl.nblk_count = (int)ep::ceil_div(n, 256);
    p.fold = (!pl.chain4 && pl.ntile <= fold_cap) ? 1 : 0;
    p.ntile = pl.ntile; p.blk_batch = pl.blk_batch; p.nblk_count = pl.nblk_count;
    return pl;
}

// the counters n_valid_dev[0 .. B] by a memset: an empty list (nothing else writes them), or the four-launch chain without a
// re-layout launch to clear them in
int bp_clear_counters(const eprecon_bp_call &a, hipStream_t st)
{
    EP_HIP_CHECK(hipMemsetAsync(a.n_valid_dev, 0, sizeof(int32_t) * (size_t)(1 + a.batch), st));
    return EPRECON_OK;
}

// the scan launch of a list whose gather does not fold it in: exclusive scan of the tile totals, the counters (and the call's
// count mailbox).  write_back = false: the early publish of a count half -- the counters and the mailbox only, the totals stay raw
int bp_launch_scan(const BpPlan &pl, hipStream_t st, bool write_back = true)
{
    hipLaunchKernelGGL(bp_scan_kernel, dim3(1), dim3(1024), 0, st, pl.tile_sums, pl.ntile, pl.p.n_valid_dev,
                       (const int32_t *)pl.blk_batch, pl.nblk_count, pl.p.batch, write_back ? 1 : 0, pl.p.counts_host,
                       pl.p.counts_seq);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// the counters' memset where one is needed, then prepare (re-layout + count in one grid) or [re-layout,] count, then the scan.
// early_publish: a count half with a count mailbox whose gather folds the scan in -- the counts are final once the count has
// run, so one workgroup sums the totals (leaving them raw) and publishes here, on the stream the count half was given, long
// before the gather half writes the same values again
template <int VOX>
int bp_queue_count(const eprecon_bp_call &a, const BpPlan &pl, hipStream_t st, bool early_publish)
{
    const BpParams &p = pl.p;
    if (a.n == 0 || (pl.chain4 && !pl.clear_in_relayout)) {
        const int rc = bp_clear_counters(a, st);
        if (rc != EPRECON_OK) return rc;
    }
    if (a.n == 0) return EPRECON_OK;
    if (pl.nchw && pl.lds_relayout > 64 * 1024) return EPRECON_ERR_UNSUPPORTED;
    const int hw = a.height * a.width, tiles = ep::ceil_div(hw, kTrPix), maps = a.n_views * a.batch;
    if (pl.nchw && !pl.chain4) {
        const int R = tiles * maps;
        const size_t lds = pl.lds_relayout > pl.lds_count ? pl.lds_relayout : pl.lds_count;
        const dim3 grid((unsigned)(R + pl.nblk_count));
        if (relayout_vec4(a.feats, pl.nhwc, hw, p.Cs))
            hipLaunchKernelGGL((bp_prepare_kernel<VOX, true>), grid, dim3(256), lds, st, p, pl.tile_sums, pl.blk_batch, a.feats,
                               pl.nhwc, hw, tiles, R);
        else
            hipLaunchKernelGGL((bp_prepare_kernel<VOX, false>), grid, dim3(256), lds, st, p, pl.tile_sums, pl.blk_batch, a.feats,
                               pl.nhwc, hw, tiles, R);
    } else {
        if (pl.nchw) {   // (only the four-launch chain comes here with NCHW maps; it clears the counters on the way for batch < 256)
            hipLaunchKernelGGL(nchw_to_nhwc_kernel<false>, dim3((unsigned)tiles, (unsigned)maps), dim3(256), pl.lds_relayout, st,
                               a.feats, pl.nhwc, a.channels, hw, p.Cs, pl.clear_in_relayout ? a.n_valid_dev : (int32_t *)nullptr,
                               pl.clear_in_relayout ? 1 + a.batch : 0);
            EP_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL((bp_count_kernel<VOX>), dim3(pl.nblk_count), dim3(256), pl.lds_count, st, p, pl.tile_sums, pl.blk_batch);
    }
    EP_LAUNCH_CHECK();
    if (!p.fold) return bp_launch_scan(pl, st);
    return early_publish && p.counts_host ? bp_launch_scan(pl, st, false) : EPRECON_OK;
}

// the gather inside the profile bracket, then the depth normalisation of MEAN_DEPTH
template <int VOX>
int bp_queue_gather(const eprecon_bp_call &a, const BpPlan &pl, hipStream_t st)
{
    if (a.n == 0) {
        if (a.rank) EP_HIP_CHECK(hipMemsetAsync(a.rank, 0, sizeof(int32_t), st));
        return EPRECON_OK;
    }
    int rc = ep::profile_bracket_begin(st);
    if (rc != EPRECON_OK) return rc;
    rc = pick<EPRECON_BP_MEAN, EPRECON_BP_MEAN_DEPTH, EPRECON_BP_VARIANCE>(
        a.mode, [&](auto mode) { return launch_gather<VOX, decltype(mode)::value>(pl.p, pl.mlp, st); });
    if (rc != EPRECON_OK) return rc;
    rc = ep::profile_bracket_end(st, pl.mlp ? "bp_gather_mlp_kernel" : "bp_gather_kernel");
    if (rc != EPRECON_OK) return rc;
    if (a.mode == EPRECON_BP_MEAN_DEPTH) {
        hipLaunchKernelGGL(bp_depth_norm_kernel, dim3(a.batch), dim3(1024), 0, st, a.out_feats, a.channels + 1, a.n_valid_dev);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

// the launches of a validated and planned descriptor: both halves, or the one `phase` names
int bp_queue(const eprecon_bp_call &a, const BpPlan &pl, hipStream_t st, bool early_publish = false)
{
    return pick<256, 64, 16>(pl.vox, [&](auto vox) {   // the one place where the tile size becomes a template argument
        constexpr int VOX = decltype(vox)::value;
        const int rc = a.phase != EPRECON_BP_GATHER ? bp_queue_count<VOX>(a, pl, st, early_publish) : EPRECON_OK;
        return rc != EPRECON_OK || a.phase == EPRECON_BP_COUNT ? rc : bp_queue_gather<VOX>(a, pl, st);
    });
}

// ---------------------------------------------------------------------------------------------
// eprecon_back_project_prepare_levels_async (host)
// ---------------------------------------------------------------------------------------------
// a level as the count half it is: the fields the levels entry ignores are the count half's
eprecon_bp_call level_call(const eprecon_bp_call &lv)
{
    eprecon_bp_call a = lv;
    a.phase = EPRECON_BP_COUNT;
    a.out_feats = a.out_mean = a.out_grid = nullptr;
    a.out_coords = a.rank = nullptr;
    a.out_mask = nullptr;
    return a;
}

int bp_prepare_levels_impl(const eprecon_bp_call *levels, int n_levels, hipStream_t st)
{
    if (!levels || n_levels <= 0 || n_levels > kMaxLevels) return EPRECON_ERR_ARG;
    eprecon_bp_call calls[kMaxLevels];
    BpPlan plans[kMaxLevels];
    bool listed[kMaxLevels];
    for (int l = 0; l < n_levels; ++l) {
        calls[l] = level_call(levels[l]);
        listed[l] = levels[l].coords != nullptr;
        const int rc = bp_validate(calls[l], listed[l] ? kBpLevelList : kBpLevelMaps);
        if (rc != EPRECON_OK) return rc;
        plans[l] = bp_plan(calls[l]);
        if (plans[l].nchw && plans[l].lds_relayout > 64 * 1024) return EPRECON_ERR_UNSUPPORTED;
    }
    // EPRECON_BP_LEVELS=0 (read per call), and the four-launch chain of EPRECON_BP_FOLD=0: every level's own launches, as the
    // one-level call queues them
    if (!eprecon_bp_levels() || plans[0].chain4) {
        for (int l = 0; l < n_levels; ++l) {
            const eprecon_bp_call &a = calls[l];
            int rc = EPRECON_OK;
            if (listed[l]) rc = bp_queue(a, plans[l], st);
            else if (plans[l].nchw)
                rc = eprecon_nchw_to_nhwc_async(a.feats, plans[l].nhwc, a.n_views * a.batch, a.channels, a.height * a.width, st);
            if (rc != EPRECON_OK) return rc;
        }
        return EPRECON_OK;
    }
    BpLevelTable t;
    size_t lds = 0;
    int cursor = 0;
    for (int l = 0; l < kMaxLevels; ++l) {
        BpLevelDev &d = t.lv[l];
        d = BpLevelDev{};
        if (l < n_levels) {
            const eprecon_bp_call &a = calls[l];
            const BpPlan &pl = plans[l];
            const bool count = listed[l] && a.n > 0;     // (an empty list: the counters are cleared, nothing else runs)
            if (listed[l] && a.n == 0) {
                const int rc = bp_clear_counters(a, st);
                if (rc != EPRECON_OK) return rc;
            }
            d.hw = a.height * a.width;
            d.tiles = ep::ceil_div(d.hw, kTrPix);
            d.vox = pl.vox;
            d.vec4 = relayout_vec4(a.feats, pl.nhwc, d.hw, pl.p.Cs) ? 1 : 0;
            d.in = a.feats; d.out = pl.nhwc; d.tile_sums = pl.tile_sums; d.blk_batch = pl.blk_batch;
            d.p = pl.p;
            const bool relayout = pl.nchw && (count || !listed[l]);
            if (relayout) {
                cursor += d.tiles * a.n_views * a.batch;
                lds = pl.lds_relayout > lds ? pl.lds_relayout : lds;
            }
            d.end_relayout = cursor;
            if (count) {
                cursor += pl.nblk_count;
                lds = pl.lds_count > lds ? pl.lds_count : lds;
            }
        } else {
            d.end_relayout = cursor;
        }
        d.end = cursor;
    }
    if (cursor > 0) {
        hipLaunchKernelGGL(bp_prepare_levels_kernel, dim3((unsigned)cursor), dim3(256), lds, st, t);
        EP_LAUNCH_CHECK();
    }
    for (int l = 0; l < n_levels; ++l) {   // lists of more tiles than EPRECON_BP_FOLD: the scan launch of the one-level call
        if (listed[l] && calls[l].n > 0 && !plans[l].p.fold) {
            const int rc = bp_launch_scan(plans[l], st);
            if (rc != EPRECON_OK) return rc;
        }
    }
    return EPRECON_OK;
}

}  // namespace

extern "C" {

size_t eprecon_back_project_workspace_bytes(int64_t n, int batch, int n_views, int channels,
                                            int height, int width, int feats_layout)
{
    const size_t map_bytes =
        feats_layout == EPRECON_LAYOUT_NCHW ? (size_t)n_views * batch * channels * height * width * sizeof(float) : 0;
    return bp_carve(n > 0 ? n : 1, batch > 0 ? batch : 1, map_bytes).end + 256;
}

size_t eprecon_back_project_workspace_maps_offset(int64_t n, int batch) { return bp_carve(n, batch, 0).maps; }

int eprecon_nchw_to_nhwc_async(const float *in, float *out, int maps, int channels, int hw,
                               void *stream)
{
    if (!in || !out || maps <= 0 || channels <= 0 || hw <= 0) return EPRECON_ERR_ARG;
    const size_t lds = (size_t)channels * (kTrPix + 1) * sizeof(float);
    if (lds > 64 * 1024) return EPRECON_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)ep::ceil_div(hw, kTrPix), (unsigned)maps);
    if (relayout_vec4(in, out, hw, channels))
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<true>, grid, dim3(256), lds, (hipStream_t)stream, in, out, channels, hw, channels,
                           (int32_t *)nullptr, 0);
    else
        hipLaunchKernelGGL(nchw_to_nhwc_kernel<false>, grid, dim3(256), lds, (hipStream_t)stream, in, out, channels, hw, channels,
                           (int32_t *)nullptr, 0);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_init_glue(void) { return ep::switch_off("EPRECON_INIT_GLUE") ? 0 : 1; }

int eprecon_back_project_call_async(const eprecon_bp_call *call, void *stream)
{
    if (!call || (call->phase != 0 && call->phase != EPRECON_BP_COUNT && call->phase != EPRECON_BP_GATHER)) return EPRECON_ERR_ARG;
    const int rc = bp_validate(*call, (BpRole)call->phase);
    return rc != EPRECON_OK ? rc : bp_queue(*call, bp_plan(*call), (hipStream_t)stream, call->phase == EPRECON_BP_COUNT);
}

int eprecon_back_project_call(const eprecon_bp_call *call, int min_valid_per_batch, int32_t *n_valid_host, void *stream)
{
    if (!call || !n_valid_host || call->phase == EPRECON_BP_COUNT) return EPRECON_ERR_ARG;   // (the count half publishes no counts)
    const int rc = eprecon_back_project_call_async(call, stream);
    if (rc != EPRECON_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    EP_HIP_CHECK(hipMemcpyAsync(n_valid_host, call->n_valid_dev, sizeof(int32_t) * (size_t)(1 + call->batch), hipMemcpyDeviceToHost, st));
    EP_HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < call->batch; ++b)
        if (n_valid_host[1 + b] < min_valid_per_batch) return EPRECON_EMPTY;
    return EPRECON_OK;
}

int eprecon_back_project_async(const int32_t *coords, int64_t n, const float *origin, int batch, float voxel_size, const float *feats,
                               int feats_layout, const float *krcam, int n_views, int channels, int height, int width,
                               int min_view, int mode, float *out_feats, float *out_mean, int32_t *out_coords, float *count,
                               float *out_grid, uint8_t *out_mask, int32_t *n_valid_dev, void *workspace, size_t workspace_bytes,
                               void *stream)
{
    eprecon_bp_call c = {};
    c.coords = coords; c.n = n; c.origin = origin; c.batch = batch; c.voxel_size = voxel_size;
    c.feats = feats; c.feats_layout = feats_layout; c.krcam = krcam;
    c.n_views = n_views; c.channels = channels; c.height = height; c.width = width; c.min_view = min_view; c.mode = mode;
    c.count = count; c.n_valid_dev = n_valid_dev; c.workspace = workspace; c.workspace_bytes = workspace_bytes;
    c.out_feats = out_feats; c.out_mean = out_mean; c.out_coords = out_coords; c.out_grid = out_grid; c.out_mask = out_mask;
    return eprecon_back_project_call_async(&c, stream);
}

int eprecon_bp_levels(void) { return ep::switch_off("EPRECON_BP_LEVELS") ? 0 : 1; }

int eprecon_back_project_prepare_levels_async(const eprecon_bp_call *levels, int n_levels, void *stream)
{
    return bp_prepare_levels_impl(levels, n_levels, (hipStream_t)stream);
}

}  // extern "C"
