/*
 * eprecon_hip.h — C ABI of libeprecon_hip.so, the MI355X (gfx950) implementation of EPRecon's
 * per-fragment 3D hot path.
 *
 * The reference (zhen6618/EPRecon, paths below are relative to its root) has no FFI of its own:
 * its seam is the Python module API, and the arithmetic of the sparse layers lives in the
 * torchsparse / spconv CUDA extensions.  Each entry point here replaces one of those Python-level
 * operators (cited per function); the modules under eprecon_amd/ keep the reference's names and argument
 * meaning on top of this ABI, INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name ends in _host; the library borrows it for
 *     the duration of the call (stream-ordered) and never frees or retains it, except for the
 *     opaque handles created by *_create and released by *_destroy;
 *   - `stream` is a hipStream_t passed as void*; NULL is the legacy default stream.  All work is
 *     enqueued on it; only functions documented as blocking synchronise it;
 *   - one caller thread per device (same as the reference: single Python thread, main.py:72);
 *   - return value: 0 = ok, 1 = "nothing to do" (the reference returns None and the caller bails
 *     out with a zero loss: ops/back_project.py:42-43, models/occupancy_initialization.py:107-108,
 *     :233-234), < 0 = error (EPRECON_ERR_* or -(1000 + hipError_t)).
 *   - coords are int32 rows (batch, x, y, z) in finest-voxel units, grouped by ascending batch
 *     index, exactly as the reference builds them (models/neucon_network.py:246-251).
 */
#ifndef EPRECON_HIP_H
#define EPRECON_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPRECON_OK 0
#define EPRECON_EMPTY 1
#define EPRECON_ERR_ARG (-1)
#define EPRECON_ERR_WORKSPACE (-2)
#define EPRECON_ERR_UNSUPPORTED (-3)
#define EPRECON_ERR_TIMEOUT (-4)      /* eprecon_mailbox_wait: the count was not published within the cap */
#define EPRECON_ERR_HIP_BASE (-1000)

/* goes up when an exported function keeps its name with another argument list: the loader refuses a library of another version */
#define EPRECON_ABI_VERSION 2
int eprecon_abi_version(void);
/* name of the gfx target the kernels were compiled for, e.g. "gfx950" */
const char *eprecon_build_arch(void);

/* ------------------------------------------------------------------------------------------
 * Count mailbox: a kernel's final counts reach the host through host-coherent pinned memory instead of a device-to-host copy
 * queued behind the kernel (no copy launch, no event, nothing on the stream).  One ring of 64 slots per process, allocated at
 * the first acquire; a slot carries at most EPRECON_MAILBOX_WORDS int32.  Thread-safe.
 *
 *   eprecon_mailbox_acquire  fills `out`: EPRECON_OK; EPRECON_EMPTY when no slot is to be had (the ring is full, words >
 *                            EPRECON_MAILBOX_WORDS, or EPRECON_COUNT_MAILBOX=0) -- the caller then copies the counts as before.
 *   a launch that takes a mailbox (eprecon_bp_call::counts_host / counts_seq, eprecon_init_select*_mb_async) is handed
 *                            payload_dev and seq; the thread that writes the final count to device memory stores the same
 *                            words at payload_dev[0 ..] and then seq into the slot's sequence word.  Set `armed` once such
 *                            a launch has been queued.  Nothing on the device waits for or reads the mailbox.
 *   eprecon_mailbox_wait     host spin (pause, then yield) until the slot's sequence word equals `seq`, at most timeout_us;
 *                            EPRECON_OK: out[0 .. words) holds the counts; EPRECON_ERR_TIMEOUT otherwise (callers use a cap
 *                            of 2 s -- far above any step -- and then synchronise the stream and read the device words).
 *   eprecon_mailbox_release  returns the slot, read or not.  A slot that is armed and not published yet is handed out again
 *                            only after its publisher has stored.
 *   eprecon_count_mailbox    1, or 0 under EPRECON_COUNT_MAILBOX=0 (read once, when the library is loaded).
 *   eprecon_mailbox_free_slots  slots that an acquire could hand out right now (diagnostics, tests).
 * ------------------------------------------------------------------------------------------ */
#define EPRECON_MAILBOX_WORDS 15
typedef struct eprecon_mailbox_slot {
    int32_t *payload_dev;         /* what the publishing launch is handed (the sequence word is the int32 in front of it) */
    const int32_t *payload_host;  /* the same words as the host sees them */
    uint32_t seq;                 /* never 0; rises per slot */
    int32_t index;                /* slot in the ring */
    int32_t words;                /* as asked for */
    int32_t armed;                /* set by the caller once a publishing launch is queued */
} eprecon_mailbox_slot;
int eprecon_count_mailbox(void);
int eprecon_mailbox_acquire(int words, eprecon_mailbox_slot *out);
int eprecon_mailbox_wait(const eprecon_mailbox_slot *slot, int64_t timeout_us, int32_t *out);
int eprecon_mailbox_release(const eprecon_mailbox_slot *slot);
int eprecon_mailbox_free_slots(void);

/* ------------------------------------------------------------------------------------------
 * Multi-view back-projection  (K1 project+mask+count, K2 stable compaction, K3 bilinear
 * gather-mean, K3' depth channel, K4 view variance)
 *
 * Replaces  Back_Project.forward            models/occupancy_initialization.py:189-261
 *           back_project                    ops/back_project.py:5-80          (mode MEAN_DEPTH)
 *           the sampling + mean/variance block of Occupancy_Initialization.forward
 *                                           models/occupancy_initialization.py:79-128 (VARIANCE)
 * ------------------------------------------------------------------------------------------ */
#define EPRECON_BP_MEAN 0       /* out_feats[n_valid, C]   = mean over visible views            */
#define EPRECON_BP_MEAN_DEPTH 1 /* out_feats[n_valid, C+1] = mean, normalised mean depth        */
#define EPRECON_BP_VARIANCE 2   /* out_feats[n_valid, C]   = population variance over views,
                                   out_mean[n_valid, C] (optional) = the view mean             */

#define EPRECON_LAYOUT_NCHW 0 /* feats f32[V, B, C, H, W]  (what the reference's backbone emits) */
#define EPRECON_LAYOUT_NHWC 1 /* feats f32[V, B, H, W, C]  (channels-last: skips the re-layout)   */

/* bytes of scratch the call needs (device memory, 256-byte aligned) */
size_t eprecon_back_project_workspace_bytes(int64_t n, int batch, int n_views, int channels,
                                            int height, int width, int feats_layout);

/*
 * One back-projection call, as a descriptor.  Every entry point below takes it; every pointer is device memory.
 *   coords      int32[n,4]            origin   f32[batch,3]       krcam f32[V,batch,4,4]
 *   out_feats   f32[n, C or C+1]      (first n_valid rows are written, input order preserved)
 *   out_mean    f32[n, C] or NULL     out_coords int32[n,4]       count f32[n] (visible views)
 *   out_grid    f32[V, n_valid, 2] or NULL   normalised image coords of the valid voxels
 *   out_mask    u8 [V, n_valid]    or NULL   per-view visibility of the valid voxels
 *               (both packed with row stride n_valid, like the reference's im_grid / mask)
 *   n_valid_dev int32[1 + batch]      [0] = n_valid, [1 + b] = valid voxels of batch b
 * phase: 0, the whole call, or one of its halves, for channels-last maps (EPRECON_LAYOUT_NHWC) only.  EPRECON_BP_COUNT queues
 * what depends on the coordinates and matrices alone (count[], the tile totals in `workspace`; feats may be NULL, the row
 * outputs and rank are ignored); EPRECON_BP_GATHER queues the rest.  Both take the same descriptor and the same workspace,
 * whose contents must survive in between; the count half may run on another stream as long as it has finished when the
 * gather half starts.  Count then gather on one stream is the whole call, launch for launch.
 */
#define EPRECON_BP_COUNT 1
#define EPRECON_BP_GATHER 2
typedef struct eprecon_bp_call {
    const int32_t *coords;     /* int32[n,4] (a level of eprecon_back_project_prepare_levels_async: or NULL, re-layout only) */
    int64_t n;
    const float *origin;       /* f32[batch,3] */
    int32_t batch;
    float voxel_size;
    const float *feats;        /* f32[V,batch,C,H,W] or [V,batch,H,W,C] (feats_layout) */
    int32_t feats_layout;
    const float *krcam;        /* f32[V,batch,4,4] */
    int32_t n_views, channels, height, width, min_view, mode;
    float *count;              /* f32[n] */
    int32_t *n_valid_dev;      /* int32[1 + batch], written by the gather half */
    void *workspace;           /* eprecon_back_project_workspace_bytes(...); of the call's own while a gather half is outstanding */
    size_t workspace_bytes;
    int32_t phase;             /* 0, EPRECON_BP_COUNT or EPRECON_BP_GATHER */
    float *out_feats, *out_mean;
    int32_t *out_coords;
    float *out_grid;
    uint8_t *out_mask;
    /* int32[n + 1] or NULL.  For a list that IS the x-major raster of a dense grid (entry e = cell e, one batch element): the
     * gather also writes rank[e] = output row of entry e or -1, rank[n] = 0 — which is the rank volume eprecon_grid_rank_async
     * would build from the call's out_coords (its trailing word counts voxels off the grid: none here).  An output of this call
     * like the others: the count half ignores it, batch != 1 is EPRECON_ERR_ARG before any launch, n == 0 clears rank[0]. */
    int32_t *rank;
    /* The count mailbox (above): eprecon_mailbox_slot::payload_dev and ::seq of a slot of 1 + batch words, or NULL and 0.  The
     * thread that writes n_valid_dev[0 .. batch] -- in the scan launch of a long list, else in the gather's last workgroup --
     * publishes the same words there.  A count half (phase EPRECON_BP_COUNT) that carries one publishes EARLY: it also queues
     * the one-workgroup scan of its tile totals behind the count on its stream, which leaves the totals as they are and writes
     * and publishes n_valid_dev[0 .. batch]; the gather half (which writes the same values again) is then handed no mailbox.
     * Needs n > 0 (an empty list has no publisher) and 1 + batch <= EPRECON_MAILBOX_WORDS, else EPRECON_ERR_ARG.  The levels of
     * eprecon_back_project_prepare_levels_async carry the fields for their gather halves (and for their scan launches). */
    int32_t *counts_host;
    uint32_t counts_seq;
} eprecon_bp_call;

/* Stream-ordered; does not synchronise.  The whole call or the half `phase` names. */
int eprecon_back_project_call_async(const eprecon_bp_call *call, void *stream);

/*
 * Blocking convenience (phase 0 or EPRECON_BP_GATHER): the call above, then copies n_valid_dev to n_valid_host[1 + batch] and
 * synchronises the stream (the reference synchronises at the same point: `torch.sum(valid_voxel)`
 * models/occupancy_initialization.py:231-233).  Returns EPRECON_EMPTY when some batch element
 * has fewer than `min_valid_per_batch` valid voxels (1 for Back_Project / back_project,
 * 1000 for the occupancy initialiser).
 */
int eprecon_back_project_call(const eprecon_bp_call *call, int min_valid_per_batch, int32_t *n_valid_host, void *stream);

/* The whole call with plain arguments, for callers without the struct: fills a descriptor (phase 0, no rank) and queues it. */
int eprecon_back_project_async(const int32_t *coords, int64_t n, const float *origin, int batch,
                               float voxel_size, const float *feats, int feats_layout,
                               const float *krcam, int n_views, int channels, int height,
                               int width, int min_view, int mode, float *out_feats,
                               float *out_mean, int32_t *out_coords, float *count,
                               float *out_grid, uint8_t *out_mask, int32_t *n_valid_dev,
                               void *workspace, size_t workspace_bytes, void *stream);

/*
 * The first halves of up to four back-projections ("levels": the image pyramid's) as ONE launch: every level's re-layout of NCHW
 * maps into its workspace and its count, for maps, lists and matrices that are all on the device already.  A level is a call
 * descriptor with a workspace of its own; `phase`, the row outputs and `rank` are ignored here.  The same descriptor with
 * phase = EPRECON_BP_GATHER and the outputs filled in queues the level's second half, on this stream or on one that waits for
 * it: a level of NCHW maps hands it the channels-last copy this launch made — `workspace` +
 * eprecon_back_project_workspace_maps_offset(n, batch) bytes — as EPRECON_LAYOUT_NHWC maps.  coords == NULL: the level's maps
 * are re-laid out only (no count; count / n_valid_dev / origin / krcam unused), to where a list of `n` entries puts them.  A
 * channels-last level is counted only.  Every level's workspace holds exactly what its own eprecon_back_project_async call
 * leaves there: the tile totals at offset 0, the per-batch rows, then the maps.  EPRECON_BP_LEVELS=0 (read at every call;
 * eprecon_bp_levels() == 0): the same work as one launch per level, as eprecon_back_project_async queues it.
 */
int eprecon_back_project_prepare_levels_async(const eprecon_bp_call *levels, int n_levels, void *stream);
size_t eprecon_back_project_workspace_maps_offset(int64_t n, int batch);
int eprecon_bp_levels(void);

/*
 * EPRECON_INIT_GLUE (read at every call): 1 unless the variable is set to 0.  0 keeps the occupancy-initialisation branch on
 * its separate glue launches: rank volume by eprecon_grid_rank_async, finalize + apply for BatchNorms of <= 4 channels, the
 * list form of the stage-0 selection ("Switches").  The host wrappers ask here, so that one reading decides.
 */
int eprecon_init_glue(void);

/*
 * Per-kernel timing hook (what bench.py's roofline line is measured with).  While enabled, every
 * eprecon_back_project*_ call brackets its gather kernel with two hipEvents recorded on the
 * caller's stream.  eprecon_profile_gather_ms() synchronises on the last stop event and returns
 * the elapsed milliseconds of that kernel alone (blocking; < 0 when nothing was recorded).
 * on == 2 arms a one-shot: only the next call's gather kernel is bracketed, later calls leave the
 * recorded pair alone (how bench.py singles out the dense 96^3 level inside a queued step).
 */
int eprecon_profile_enable(int on);
float eprecon_profile_gather_ms(void);
/* family of the gather kernel the recorded pair brackets ("bp_gather_mlp_kernel" / "bp_gather_kernel") */
const char *eprecon_profile_gather_kernel(void);

/*
 * The same for the gather-GEMM convolution (bench.py's `roofline_conv`): arm a one-shot — the next
 * sparse-convolution launch with this (kvol, cin, cout) on a list of at least min_rows rows is
 * bracketed by two events on its stream.  eprecon_profile_conv_ms blocks on the stop event and returns
 * the milliseconds (< 0: nothing recorded), the list length and the name of the kernel family chosen.
 */
int eprecon_profile_conv_arm(int kvol, int cin, int cout, int64_t min_rows);
float eprecon_profile_conv_ms(int64_t *rows_out, const char **kernel_out);
/* live (output row, kernel offset) pairs of the bracketed launch (2 * pairs * cin * cout = its algorithmic flops),
 * counted on the launch stream behind the stop event; blocks; -1 when nothing was recorded */
int64_t eprecon_profile_conv_pairs(void);
/* the (row, offset) pairs that launch issued MFMAs for: the direct kernel skips an offset for the 32 rows of a wave when none
 * of them has a neighbour there, so this is 32 x the live (32-row group, offset) pairs; 0 for the kernels that walk every offset
 * of every row (executed = kvol * rows) */
int64_t eprecon_profile_conv_executed_pairs(void);
/* name of the kernel family the most recent convolution launch of this process went to ("spconv_direct16_kernel",
 * "spconv_splitk_kernel", "spconv_wide_kernel", "conv3d_tile16_kernel", ...): lets callers and tests assert the selection */
const char *eprecon_profile_last_conv_kernel(void);
/* stage marker for rocprofv3 kernel traces: an empty launch of (id + 1) workgroups on `stream` (tools/trace_cfg4_layers.py) */
int eprecon_profile_mark_async(int id, void *stream);

/* NCHW -> NHWC re-layout of a stack of feature maps: in f32[maps, C, H*W] -> out f32[maps, H*W, C] */
int eprecon_nchw_to_nhwc_async(const float *in, float *out, int maps, int channels, int hw,
                               void *stream);
/* The same for the per-view maps of up to three pyramid levels in ONE launch: src[l][v] f32[C_l, hw_l] (one contiguous map per
 * view, as models/occupancy_initialization.py:79-90 receives them: features_all[view][level][batch]) -> dst[l] f32[n_views * hw_l,
 * C_l] (pixel rows, views stacked).  Replaces torch.stack per level + the channels-last copy in front of the 2D fusion stack. */
typedef struct eprecon_views_desc {
    const float *src[3][16];
    float *dst[3];
    int32_t channels[3]; int32_t hw[3];
    int32_t levels; int32_t n_views;
} eprecon_views_desc;
int eprecon_views_to_rows_async(const eprecon_views_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------
 * Hash grid over voxel coordinates  (K6 / K7)
 *
 * Replaces  torchsparse F.sphash + F.sphashquery   ops/torchsparse_utils.py:19-21,44-50,73-79
 *           torch.unique(hash) voxel numbering     ops/torchsparse_utils.py:20-22
 * (torchsparse is an un-vendored dependency of the reference, README.md:19; semantics restated
 * in DESIGN.md.)  A table is caller-owned device memory of eprecon_hash_table_bytes(capacity)
 * bytes, capacity = eprecon_hash_capacity(n) (a power of two >= 2n).  Keys are exact 64-bit
 * packings of (b, x, y, z): |coordinate| < 2^19 - 1, 0 <= b <= 14.  `quantum` q >= 1 maps every
 * spatial coordinate to floor(c / q) * q before hashing (q = 2 * tensor_stride builds the strided
 * coordinate set of a k2s2 convolution).
 * ------------------------------------------------------------------------------------------ */
uint32_t eprecon_hash_capacity(int64_t n);
size_t eprecon_hash_table_bytes(uint32_t capacity);
/* value of a key = smallest input row that carries it */
int eprecon_hash_build_async(const int32_t *coords, int64_t n, int quantum, void *table,
                             uint32_t capacity, void *stream);
/* ... with the row count on the device: only the first min(n_cap, *n_dev) rows are inserted (the table is sized by n_cap) */
int eprecon_hash_build_dn_async(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, int quantum, void *table,
                                uint32_t capacity, void *stream);
/* out_index[i] = value stored for queries[i] (int32[m,4] bxyz), or -1 */
int eprecon_hash_query_async(const void *table, uint32_t capacity, const int32_t *queries, int64_t m,
                             int quantum, int32_t *out_index, void *stream);
/* blocking: EPRECON_OK, EPRECON_ERR_UNSUPPORTED (a key was out of range) or
 * EPRECON_ERR_WORKSPACE (table full) */
int eprecon_hash_status(const void *table, void *stream);

/* Unique (quantised) coordinates in FIRST-OCCURRENCE order:
 *   inverse[i]           id of row i's voxel                        int32[n]
 *   unique_coords[id]    its quantised (b,x,y,z)                     int32[n,4] (first n_unique rows)
 *   n_unique_dev         int32[1]
 * afterwards the table maps key -> voxel id (so eprecon_hash_query_async returns ids). */
size_t eprecon_unique_workspace_bytes(int64_t n);
/* exclusive prefix sum of int32 (the device scan behind every compaction / unique numbering of the path: torch.nonzero,
 * boolean-mask indexing and torch.unique at models/neucon_network.py:298-318,454-507, ops/torchsparse_utils.py:20-22):
 * out[i] = in[0] + ... + in[i - 1]; *total (optional, device) = the sum of all n; scratch
 * int32[eprecon_exclusive_scan_scratch_ints(n)]: the tile sums one launch of the call leaves for the next.  The call cannot
 * see the size of what it is given: the query is the contract.  A call touches no memory but what it is handed. */
size_t eprecon_exclusive_scan_scratch_ints(int64_t n);
int eprecon_exclusive_scan_async(const int32_t *in, int64_t n, int32_t *out, int32_t *total, int32_t *scratch, void *stream);
int eprecon_unique_coords_async(const int32_t *coords, int64_t n, int quantum, void *table,
                                uint32_t capacity, int32_t *inverse, int32_t *unique_coords,
                                int32_t *n_unique_dev, void *workspace, size_t workspace_bytes,
                                void *stream);

/* The same with the row count ON THE DEVICE ("outputs written into caller-allocated buffers sized by the static
 * caps, with the actual count returned through a device counter"): the live count is min(n_cap, *n_dev), buffers, the
 * table and the workspace are sized for n_cap, launches cover n_cap rows.  Lets a chain of data-dependent steps (quantise ->
 * unique -> unique of the coarser stride ...) be queued without a host round trip between them; the caller reads all
 * counts back once. */
int eprecon_unique_coords_dn_async(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, int quantum, void *table,
                                   uint32_t capacity, int32_t *inverse, int32_t *unique_coords, int32_t *n_unique_dev,
                                   void *workspace, size_t workspace_bytes, void *stream);
/*
 * The voxel sets of a point cloud at tensor strides 1, 2, 4 (levels <= 3) numbered back to back with every count on the device
 * (SPVCNN: models/modules.py:148-175 voxelises at stride 1, its two k2s2 stages build strides 2 and 4): level l numbers the
 * unique rows of level l - 1 (level 0: the first min(n_cap, *n_dev) rows of `coords`; n_dev NULL: all n_cap) at quantum 2^l into
 * tables[l] (capacities[l] slots, eprecon_hash_capacity(n_cap)), inverse[l] int32[n_cap], unique_coords[l] int32[n_cap,4]; the
 * count of level l is written next to its table's status word (int32 tables[l][1]).  The tables are reset by ONE launch.
 * summary (optional, device int32[2 levels]): receives (status, count) of every level side by side — what the host reads.
 */
int eprecon_unique_hierarchy_dn_async(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, int levels, void *const *tables,
                                      const uint32_t *capacities, int32_t *const *inverse, int32_t *const *unique_coords,
                                      int32_t *summary, void *workspace, size_t workspace_bytes, void *stream);

/*
 * eprecon_kernel_map_async(ksize 3) for a voxel set queried against ITS OWN table — coords int32[n,4] are pairwise distinct and
 * row i is the table's value for its key (what eprecon_unique_coords*_async / eprecon_unique_hierarchy_dn_async leave behind) —
 * with half the hash probes: the map of a submanifold 3x3x3 convolution (models/modules.py:19-23,181, spnn.Conv3d stride 1) is
 * symmetric (offset -o from j reaches i exactly when +o from i reaches j).  Same int32[27][n] table, bit for bit.
 */
int eprecon_kernel_map_self_async(const void *table, uint32_t capacity, const int32_t *coords, int64_t n, int stride, int32_t *nbr,
                                  void *stream);

/*
 * Connected components of a sparse voxel set (csrc/components.hip; no counterpart in the reference, whose users cluster the
 * finished mesh in open3d: the rule is DESIGN.md §5b, the caller eprecon_amd/clean_scene.py).
 *   nbr           int32[27][n], the self map of n pairwise distinct rows (eprecon_kernel_map_self_async, stride 1)
 *   keys          int32[n] or NULL (every key 0)
 *   connectivity  6, 18 or 26: rows are adjacent when their coordinate difference d has d != 0, max |d_i| <= 1 and
 *                 sum |d_i| <= 1, 2 or 3
 * Rows i and j are linked iff they are adjacent, keys[i] == keys[j] and that key is >= 0; a row with a negative key links
 * nothing and bridges nothing.  label[i] = the smallest row index of row i's component (label[i] <= i,
 * label[label[i]] == label[i]), -1 for a row with a negative key: the same values on every run.
 * Three launches (init, hook, flatten) whatever n and the components look like, no host read, no workgroup waits on another.
 * status int32[1] (device): written by every call; 0 afterwards, or bit 0 / bit 1 when a bounded loop (a chain of more than n
 * steps / a link retried more than n times) gave up — the labels mean nothing then, and the caller that reads it raises.
 * workspace: eprecon_components_workspace_bytes(n) bytes, 4-byte aligned (the parent array).  n == 0 only clears status.
 */
size_t eprecon_components_workspace_bytes(int64_t n);
int eprecon_components_async(const int32_t *nbr, int64_t n, const int32_t *keys, int connectivity, int32_t *label, int32_t *status,
                             void *workspace, size_t workspace_bytes, void *stream);

/*
 * Ray casting of a sparse TSDF scene from its voxel rows (csrc/tsdf_raycast.hip; the reference meshes a scene to show it:
 * the rule is DESIGN.md §5b "ray-cast surface", the caller eprecon_amd/raycast.py).
 *   coords  int32[m,3] voxel rows (no batch column; c - 1 .. c + 1 must be keys of the hash grid), tsdf f32[m]
 *   grid    eprecon_raycast_workspace_bytes(m) bytes, 256-byte aligned, owned by the caller: an int32 header (word 0 the build's
 *           status: bit 0 a coordinate out of range, bit 1 a table full; words 1..3 / 4..6 the smallest / largest active cell,
 *           INT_MAX / INT_MIN when no row has tsdf <= 0), the row table (key -> first row) and the brick table (4x4x4-cell
 *           bricks, brick = cell >> 2, a 64-bit word with bit x + 4 y + 16 z per active cell).  Nothing is allocated inside.
 * eprecon_raycast_build_async: two launches (clear, build); m == 0 only clears.
 * eprecon_raycast_async (m >= 1, the grid of a build over the same m rows):
 *   cams    fp64: K[9], K^-1[9], world -> camera [3x4] per view (eprecon_render_visibility_async's block), then origin[3] and
 *           1 / voxel_size
 *   depth f32[V,H,W] camera-z metres (0: nothing hit), normal f32[V,H,W,3] unit, world frame, towards positive TSDF (0),
 *   row int32[V,H,W] index of the hit cell's row corner nearest the hit point (-1)
 *   status int32[1] (device): cleared and written by every call; bit 0 / bit 1 when a bounded walk (cells of a brick / bricks
 *           of the box) gave up: the pixel is empty then, and the caller that reads it raises.
 * One launch, no atomics: the images are bit-identical from run to run and however the views are split into calls.
 */
size_t eprecon_raycast_workspace_bytes(int64_t m);
int eprecon_raycast_build_async(const int32_t *coords, const float *tsdf, int64_t m, void *grid, size_t grid_bytes, void *stream);
int eprecon_raycast_async(const void *grid, int64_t m, const float *tsdf, const double *cams, int n_views, int height, int width,
                          float pixel_center, float znear, float zfar, int refine, float *depth, float *normal, int32_t *row,
                          int32_t *status, void *stream);

/*
 * Distance field of a sparse TSDF scene (csrc/distance_field.hip; the rule is DESIGN.md §5b "distance field", the caller
 * eprecon_amd/distance_field.py): for every cell of the box [lo, hi) the exact squared distance, in cells, to the nearest site
 * inside the box, and that site's row.
 *   coords  int32[m,3] voxel rows (no batch column; c - 1 .. c + 1 must be keys of the hash grid), tsdf f32[m].  A row is
 *           inside when tsdf <= 0, a coordinate that is no row is outside, of rows that repeat a coordinate the first counts;
 *           a site is a row with a 6-neighbour coordinate whose inside-state differs from its own.  Rows outside the box are
 *           looked up as neighbours and are no sites of this call.
 *   lo, hi  host int32[3]; extents X, Y, Z = hi - lo, each 1 .. 1024
 *   radius  R >= 0 in cells
 *   dist2   int32[X,Y,Z] (z fastest): min over the sites s of |x - s|^2, exact where it is <= R^2, 0x7fffffff beyond
 *   site    int32[X,Y,Z]: the smallest row among the sites that attain dist2, -1 beyond R^2
 *   state   uint8[X,Y,Z]: 0 no row, 1 an outside row, 2 an inside row
 *   status  int32[1] (device): cleared and written by every call; bit 0 a coordinate outside the key range (the row is left
 *           out), bit 1 the row table full.  The caller that reads it raises.
 *   workspace  eprecon_distance_field_workspace_bytes(m, lo, hi) bytes (0 for a box the call would refuse), 256-byte aligned:
 *           the row table and two volumes of 64-bit keys (d2 << 32) | row.  Nothing is allocated inside.
 * Six launches whatever the rows look like (clear, insert, seed, and a band-minimum pass along z, y and x); m == 0 fills far
 * and state 0 in the first and launches nothing else.  No atomics outside the table build, no workgroup waits on another,
 * integers only: the outputs are bit-identical from run to run.
 * EPRECON_ERR_ARG: an empty or inverted box, an extent above 1024, radius < 0, a null pointer, a short workspace.
 */
size_t eprecon_distance_field_workspace_bytes(int64_t m, const int32_t lo[3], const int32_t hi[3]);
int eprecon_distance_field_async(const int32_t *coords, const float *tsdf, int64_t m, const int32_t lo[3], const int32_t hi[3],
                                 int radius, int32_t *dist2, int32_t *site, uint8_t *state, int32_t *status, void *workspace,
                                 size_t workspace_bytes, void *stream);
/* ------------------------------------------------------------------------------------------
 * Kernel maps and sparse convolution  (K5, K10, K11, K13)
 *
 * Replaces  spnn.Conv3d (k3 s1 / k2 s2 / transposed / k1)   models/modules.py:19-64,90-122,181
 *           spconv SubMConv3d (k1 / k3, bias)               models/modules.py:252,444
 * nbr is int32[K][n]: nbr[k][i] = row of the voxel at coords[i] + offset_k * stride in the set the
 * table was built on, or -1.  ksize 3: K = 27, offsets in {-1,0,1}^3 with x fastest;
 * ksize 2: K = 8, offsets in {0,1}^3 with z fastest (k = 4 bx + 2 by + bz).
 *   stride-1 k3 conv on a set S:   table(S), coords = S, stride = tensor stride of S
 *   k2s2 down-conv S -> T:         table(S), coords = T (= unique of S at quantum 2 ts), stride = ts
 *   its transpose T -> S:          eprecon_transpose_map_async(S, parent = inverse from the unique call)
 * ------------------------------------------------------------------------------------------ */
int eprecon_kernel_map_async(const void *table, uint32_t capacity, const int32_t *coords, int64_t n,
                             int ksize, int stride, int32_t *nbr, void *stream);
int eprecon_transpose_map_async(const int32_t *fine_coords, int64_t n, const int32_t *parent,
                                int fine_stride, int32_t *up_map, void *stream);
/*
 * out[i, 0:cout] (op)= bias + sum_k x[nbr[k][i], 0:cin] @ weight[k]      weight f32[kvol][cin][cout]
 * x / out are row-major with leading dimensions ld_x / ld_out (so a layer can read from / write
 * into a channel slice of a wider buffer = torchsparse.cat for free).  nbr == NULL means the
 * identity map (kvol must be 1: a per-voxel linear layer).  relu != 0 fuses ReLU; accumulate != 0
 * adds to the existing contents of out.  fp32 MFMA, deterministic.
 */
int eprecon_sparse_conv_async(const float *x, int64_t n_in, int ld_x, const int32_t *nbr, int kvol,
                              int64_t n_out, const float *weight, int cin, int cout, const float *bias,
                              float *out, int ld_out, int relu, int accumulate, void *stream);
/*
 * The same contraction with the epilogues the reference wires around its convolutions:
 *   v = conv + bias [+ out]; [v = relu(v)]; [v += residual];  out = v
 * (residual: BN(x + ReLU(conv(x))) blocks, models/modules.py:385-399), and optionally the first
 * half of the train-mode BatchNorm that follows (models/modules.py:372-383 and every
 * spnn.BatchNorm): bn_partial f32[3][cout][nblk], nblk = ceil(n_out/128), receives per-workgroup
 * (count, mean, M2) summaries of the stored values, channel-major (eprecon_conv_bn_partial_bytes bytes),
 * to be finished by eprecon_batchnorm_apply_partials_async (ld = nblk) without re-reading the tensor
 * for statistics.
 */
size_t eprecon_conv_bn_partial_bytes(int64_t n_out, int cout);
int eprecon_sparse_conv_fused_async(const float *x, int64_t n_in, int ld_x, const int32_t *nbr, int kvol,
                                    int64_t n_out, const float *weight, int cin, int cout,
                                    const float *bias, const float *residual, int ld_res, float *out,
                                    int ld_out, int relu, int accumulate, float *bn_partial, void *stream);
/*
 * Descriptor form with the remaining fusions of a conv -> BatchNorm(train) -> [ReLU] chain, so that
 * one launch per layer is left (the 2D fusion stack of models/occupancy_initialization.py:22-58 is
 * ~32 such layers and launch-bound otherwise):
 *   in_scale / in_shift [cin]   BatchNorm of the producer layer applied while gathering:
 *                               a = [relu]( x * in_scale[c] + in_shift[c] ), zero padding stays 0
 *   res_scale / res_shift [cout] the same for the residual operand
 *   bn_partial                  per-workgroup (count, mean, M2) summaries of THIS layer's stored output:
 *                               eprecon_batchnorm_finalize_affine_async turns them into (scale, shift)
 * The stored tensor is the un-normalised conv output; consumers apply (scale, shift) on load, or
 * eprecon_affine_rows_async materialises it.  (Round 3 also finished the statistics INSIDE the launch — write-through
 * summaries + arrival counters; parity-green and slower than the 7 us finalize launch, removed in round 4: DESIGN.md 7c.)
 */
typedef struct eprecon_conv_desc {
    const float *x; int64_t n_in; int ld_x;
    const int32_t *nbr; int kvol; int64_t n_out;
    const float *weight; int cin; int cout;
    const float *bias;
    const float *residual; int ld_res;
    float *out; int ld_out;
    int relu; int accumulate;
    const float *in_scale; const float *in_shift; int in_relu;
    const float *res_scale; const float *res_shift; int res_relu;
    /* ... channel-major: (count, mean, M2) of column c from summary row r at bn_partial[(q * cout + c) * bn_ld + r], q = 0, 1, 2;
     * bn_ld >= eprecon_conv_desc_partial_rows(desc), 0 = exactly that many */
    float *bn_partial; int bn_ld;
    /* row-wise LayerNorm over the cout channels after bias / ReLU / residual (the spconv + LayerNorm
     * blocks of models/modules.py:447-452,473-482, models/occupancy_initialization.py:141-169):
     * out = [relu]( LN(v) * ln_gamma + ln_beta ); cout <= 128, excludes bn_partial / accumulate */
    int ln; const float *ln_gamma; const float *ln_beta; float ln_eps; int ln_post_relu;
    /* dense 2D 3x3 'same' convolution over img_maps images of img_h x img_w pixel rows (kvol == 9,
     * n_out == img_maps * img_h * img_w): narrow layers then run as an implicit GEMM on image tiles
     * (halo tile + all nine weight matrices in LDS, no kernel map); nbr is still required as the
     * fallback for shapes the tile kernel does not take */
    int img_h; int img_w; int img_maps;
    /* dense-grid form of a 3x3x3 stride-1 convolution (kvol == 27) for voxel sets that fill most of their bounding
     * grid (the submanifold stack of models/occupancy_initialization.py:131-174 on the dense 48^3 grid): vox_rank
     * int32[grid_x*grid_y*grid_z] from eprecon_grid_rank_async maps a grid cell to its voxel's row (-1: none).
     * Layers the tile kernels take (cin % 4 == 0, cin <= 64: cout == 1, or cout <= 32 with cin % 16 == 0 and
     * packed_weight16) run as an implicit GEMM on cell tiles with the halo rows staged once in LDS: no kernel map, nbr
     * may be NULL.  Other shapes fall back to nbr (EPRECON_ERR_ARG when it is NULL). */
    const int32_t *vox_rank; int grid_x; int grid_y; int grid_z;
    /* `weight` in the operand order of v_mfma_f32_32x32x2_f32 (eprecon_conv_pack_weight_async): lets the short-list
     * (split-K) and cross-workgroup (medium lists, wide channels) kernels read their B operands without LDS staging */
    const float *packed_weight;
    /* the same weights in the operand order of the 16x16x4 MFMA kernels (eprecon_conv_pack_weight16_async, cout <= 64):
     *  - with vox_rank: the 16-row tile kernel, which takes cout <= 32 with cin a multiple of 16 (EPRECON_CONV_DENSE3D >= 2);
     *  - with nbr (kvol 27, or 9 for a pixel map): the direct gather kernel for lists the short-list rule does not take
     *    (operands straight from L2 into the MFMAs, no LDS staging; EPRECON_CONV_DIRECT=0 switches it off).  NULL keeps the
     *    launch on the 32x32x2 kernels.
     * Results equal those kernels' within fp32 round-off (four input channels per MFMA instead of two: another summation
     * order); the torchsparse / spconv layers this replaces (models/modules.py:15-72, 178-222) make no ordering promise. */
    const float *packed_weight16;
    /* scratch for kernels that reduce partial sums across workgroups (medium lists with wide channels, 3x3x3, with
     * packed_weight): eprecon_conv_desc_workspace_bytes(desc) bytes (0: none needed); without it those shapes stay on the
     * short-list kernel.  With EPRECON_CONV_PERSIST=1 the query also answers the job counters of the persistent kernel (512
     * bytes, zeroed by the launch): a launch that kernel would take WITHOUT them returns EPRECON_ERR_WORKSPACE — its
     * summaries are per 32-row job, no other kernel can stand in */
    void *workspace; size_t workspace_bytes;
    /* BatchNorm of the OUTPUT without a finalize launch (round 6; replaces bn_partial + eprecon_batchnorm_finalize_affine_async
     * between two layers, models/modules.py:15-29,313-399): the launch adds per-channel sums of the stored values to an
     * accumulator block with order-independent 64-bit integer atomics (exact fixed-point limbs: deterministic), and the
     * consumer of this layer's output names the block as in_acc and finishes it in its prologue.  A block of `ld` channels is
     * int64[eprecon_bn_acc_words(ld)]: int64[8][ld][7] sums, ZEROED by the caller before the producer runs, followed by
     * float[2][ld] (gamma, beta: the producer copies bn_gamma / bn_beta there; NULL = 1 / 0); bn_acc_c0 = first channel of
     * this layer inside the block (layers writing channel slices of one concatenated activation share a block).  Only for
     * launches eprecon_conv_desc_takes_bn_acc() accepts (no ln / accumulate, not the dense-grid 3D tile kernels). */
    long long *bn_acc; int bn_acc_ld; int bn_acc_c0; const float *bn_gamma; const float *bn_beta;
    /* ... and of the INPUT: the block the producer(s) of x filled, instead of in_scale / in_shift (in_relu still applies);
     * in_affine_scratch float[2 * cin]: where the library finishes the block with a launch of its own for the kernels that do
     * not do it in their prologue */
    const long long *in_acc; int in_acc_ld; int in_acc_c0; float in_eps; float *in_affine_scratch;
} eprecon_conv_desc;
/* int64 words of an accumulator block of `ld` channels (sums + the two parameter vectors) */
size_t eprecon_bn_acc_words(int ld);
/* 1 when the launch described by desc can produce into bn_acc (ask before setting it) */
int eprecon_conv_desc_takes_bn_acc(const eprecon_conv_desc *desc);
/* a block -> (scale, shift) vectors of `channels` channels from acc_c0 on: the stand-alone finish */
int eprecon_batchnorm_acc_affine_async(const long long *acc, int acc_ld, int acc_c0, int channels, float eps, float *scale_out,
                                       float *shift_out, void *stream);
/* out[i, c] = [relu]( x[i, c] * scale[c] + shift[c] ) with (scale, shift) finished from a block by every workgroup (channels <= 512) */
int eprecon_affine_rows_acc_async(const float *x, int64_t n, int channels, int ld_x, const long long *acc, int acc_ld, int acc_c0,
                                  float eps, int relu, float *out, int ld_out, void *stream);
int eprecon_conv_desc_async(const eprecon_conv_desc *desc, void *stream);
size_t eprecon_conv_desc_workspace_bytes(const eprecon_conv_desc *desc);
/* number of bn_partial rows the launch described by desc writes (nblk of the finalize call) */
int64_t eprecon_conv_desc_partial_rows(const eprecon_conv_desc *desc);
/* which dense-grid kernel the shape described by desc (vox_rank, grid_*, x, ld_x, cin, cout, in_scale / in_shift, ln,
 * accumulate, bn_partial) is for: 0 none (the launch needs nbr), 1 the single-column kernel, 2 the 16-row tile kernel, which
 * takes the launch when packed_weight16 is given.  Ask before packing weights or dropping the kernel map; host arithmetic,
 * nothing is dereferenced.  EPRECON_CONV_DENSE3D is read per call. */
int eprecon_conv_dense3d_kind(const eprecon_conv_desc *desc);
/* producer-side summaries partial f32[3][channels][ld] (row r of channel c: partial[(q * channels + c) * ld + r], r < nblk <= ld)
 * -> the BatchNorm in affine form */
int eprecon_batchnorm_finalize_affine_async(const float *partial, int64_t nblk, int64_t ld, int channels, const float *gamma,
                                            const float *beta, float eps, float *scale_out, float *shift_out,
                                            void *stream);
/* out[i, c] = [relu]( x[i, c] * scale[c] + shift[c] [+ residual[i, c]] ): a producer-finished BatchNorm materialised, and the
 * tail of the residual blocks (models/modules.py:46-72); residual may be NULL (else ld_res >= channels); out may alias x */
int eprecon_affine_rows_async(const float *x, int64_t n, int channels, int ld_x, const float *scale,
                              const float *shift, const float *residual, int ld_res, int relu, float *out,
                              int ld_out, void *stream);
/*
 * The joins of the 2D fusion stack in one launch each.  x: the pixel rows f32[maps*height*width, channels] (row stride ld_x)
 * of a level with its pending BatchNorm (scale, shift, relu), applied on load as eprecon_affine_rows_async does.
 *   pool2  out row (m, y, x) of the (height/2) x (width/2) grid = mean of the 2x2 block at (2y, 2x): sum in (kh, kw) order,
 *          then the divide (the arithmetic of a channels-last average pooling, kernel 2, stride 2)
 *   up2    out row (m, y, x) of the 2 height x 2 width grid = the bilinear x2 sample of eprecon_upsample2x_nhwc_async
 * out has row stride ld_out >= channels (a channel slice of a concat buffer).  No allocation: capture-safe.
 */
int eprecon_affine_pool2_rows_async(const float *x, int maps, int height, int width, int channels, int ld_x, const float *scale,
                                    const float *shift, int relu, float *out, int ld_out, void *stream);
int eprecon_affine_up2_rows_async(const float *x, int maps, int height, int width, int channels, int ld_x, const float *scale,
                                  const float *shift, int relu, float *out, int ld_out, void *stream);
/*
 * Kernel map of a dense 2D 'same' convolution (odd ksize) over `maps` images of height x width
 * pixels stored as rows [maps][height][width] of a channels-last tensor:
 * nbr int32[ksize*ksize][maps*height*width], offset index ky * ksize + kx, -1 = zero padding.
 * With it nn.Conv2d(padding="same") of models/modules.py:313-399 / models/occupancy_initialization.py:22-31
 * runs on eprecon_sparse_conv_fused_async (weight re-laid out to [ky*ks+kx][cin][cout]).
 */
int eprecon_pixel_map_async(int maps, int height, int width, int ksize, int32_t *nbr, void *stream);
/*
 * Rank volume of a voxel set that lives on a dense grid (coords int32[n,4] (b,x,y,z), multiples of `stride`,
 * 0 <= x / stride < grid_x ...): rank int32[grid_x*grid_y*grid_z + 1], z fastest; rank[cell] = row of the voxel or -1,
 * the last element counts voxels off the grid (0 for a valid set).  Replaces the hash grid + 27-offset kernel map
 * for the dense-grid convolution form of eprecon_conv_desc (the role spconv's indice pairs play at
 * models/modules.py:260-271 for the reference).
 */
int eprecon_grid_rank_async(const int32_t *coords, int64_t n, int stride, int grid_x, int grid_y, int grid_z, int32_t *rank,
                            void *stream);
/* weight f32[kvol][cin][cout] -> the operand order of the dense-grid kernel (eprecon_conv_pack_weight_floats floats) */
size_t eprecon_conv_pack_weight_floats(int kvol, int cin, int cout);
int eprecon_conv_pack_weight_async(const float *weight, int kvol, int cin, int cout, float *packed, void *stream);
/* ... -> the operand order of the 16x16x4 MFMA kernels, cout <= 64 (0 floats / EPRECON_ERR_ARG beyond) */
size_t eprecon_conv_pack_weight16_floats(int kvol, int cin, int cout);
int eprecon_conv_pack_weight16_async(const float *weight, int kvol, int cin, int cout, float *packed, void *stream);
/* Many packings in one launch: `jobs` is an array of njobs (<= 65,535) descriptors in DEVICE memory; kind 0 = the order of
 * eprecon_conv_pack_weight_async, 1 = of eprecon_conv_pack_weight16_async (cout <= 64); `packed` sized by the matching
 * *_floats call.  An optimisation step (main.py:297-313: optimizer.step()) changes every weight, so the operand-order copies
 * of every spnn.Conv3d (models/modules.py:15-72, 178-222) are rebuilt once per step: one launch instead of one per layer. */
typedef struct eprecon_pack_job {
    const float *weight; float *packed;
    int32_t kvol; int32_t cin; int32_t cout; int32_t kind;
} eprecon_pack_job;
int eprecon_conv_pack_many_async(const eprecon_pack_job *jobs, int njobs, void *stream);

/* ------------------------------------------------------------------------------------------
 * Normalisation epilogues  (K12)
 *
 * Replaces  spnn.BatchNorm / nn.BatchNorm1d in TRAIN mode (batch statistics over all active
 *           voxels; the reference tests in train mode, main.py:357)   models/modules.py:22,41,54,60,65
 *           nn.LayerNorm with the ReLU / residual wiring of           models/modules.py:447-452,473-482
 *                                                                     models/occupancy_initialization.py:141-169
 * ------------------------------------------------------------------------------------------ */
size_t eprecon_batchnorm_workspace_bytes(int64_t n, int channels);
/* out = [relu]( (x - mean) / sqrt(var + eps) * gamma + beta [+ residual] ), biased variance;
 * out may alias x; mean_out / var_out optional f32[channels] */
int eprecon_batchnorm_train_async(const float *x, int64_t n, int channels, int ld_x, const float *gamma,
                                  const float *beta, float eps, const float *residual, int ld_res,
                                  int relu, float *out, int ld_out, float *mean_out, float *var_out,
                                  void *workspace, size_t workspace_bytes, void *stream);
/* second half of the same BatchNorm from producer-side summaries partial f32[3][channels][ld], ld >= nblk
 * (count, mean, M2 per block, channel-major as eprecon_batchnorm_finalize_affine_async reads them, merged in block order).
 * res_scale / res_shift (both or neither, and only with a residual, else EPRECON_ERR_ARG): the residual carries a pending
 * BatchNorm of its own in affine form (the 1x1 skip convolution + BatchNorm of a residual block, models/modules.py:57-65,71):
 * residual' = residual * res_scale + res_shift on load.  mean_out / var_out optional f32[channels]. */
size_t eprecon_batchnorm_apply_workspace_bytes(int channels);
int eprecon_batchnorm_apply_partials_async(const float *x, int64_t n, int channels, int ld_x, const float *partial,
                                           int64_t nblk, int64_t ld, const float *gamma, const float *beta, float eps,
                                           const float *residual, int ld_res, const float *res_scale,
                                           const float *res_shift, int relu, float *out, int ld_out, float *mean_out,
                                           float *var_out, void *workspace, size_t workspace_bytes, void *stream);
/* per row: t = x; if pre_relu t = relu(t); if residual t += residual; y = LN(t) * gamma + beta;
 * if post_relu y = relu(y).  out may alias x. */
int eprecon_rowwise_layernorm_async(const float *x, int64_t n, int channels, int ld_x,
                                    const float *residual, int ld_res, const float *gamma,
                                    const float *beta, float eps, int pre_relu, int post_relu,
                                    float *out, int ld_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Dense-grid helpers of the coarse-to-fine loop  (K14, K16)
 * ------------------------------------------------------------------------------------------ */
/*
 * Initialisation -> coarse selection (models/neucon_network.py:264,298-318): per batch element,
 * mark the (dim^3) coarse cells that contain a voxel with sigmoid(logit) > threshold (the 2^3
 * max-pool of the 48^3 volume when cell = 4 and the voxels sit on the interval-2 grid), erode with
 * a zero-padded 3^3 box, dilate twice, and emit the surviving cells in raster order as
 * (b, cell*x, cell*y, cell*z).  coords int32[n,4] are the valid voxels the logits belong to.
 * out_coords int32[batch*dim^3, 4]; n_out_dev int32[1 + batch] ([0] total, [1+b] per batch).
 */
size_t eprecon_init_select_workspace_bytes(int batch, int dim);
int eprecon_init_select_async(const float *logit, const int32_t *coords, int64_t n, float threshold,
                              int batch, int dim, int cell, int32_t *out_coords, int32_t *n_out_dev,
                              void *workspace, size_t workspace_bytes, void *stream);
/*
 * The same for ONE batch element whose voxels are rows of a dense grid_x x grid_y x grid_z grid of `stride` voxels
 * (cell % stride == 0) whose rank volume the caller holds (rank int32[grid_x*grid_y*grid_z]: cell -> row or -1,
 * eprecon_grid_rank_async): the marks are written in full by one launch over the coarse cells, without a clear and
 * without a pass over the list.  Same coordinates, counts and order.  EPRECON_INIT_GLUE=0 runs the list form.
 */
int eprecon_init_select_dense_async(const float *logit, const int32_t *coords, int64_t n, const int32_t *rank, int grid_x,
                                    int grid_y, int grid_z, int stride, float threshold, int dim, int cell,
                                    int32_t *out_coords, int32_t *n_out_dev, void *workspace, size_t workspace_bytes,
                                    void *stream);
/*
 * The two selections with a count mailbox: the thread that writes the last word of n_out_dev[0 .. batch] also publishes them
 * into `slot` (eprecon_mailbox_acquire(1 + batch, ...); 1 + batch words).  slot == NULL: the calls above, which forward here.
 */
int eprecon_init_select_mb_async(const float *logit, const int32_t *coords, int64_t n, float threshold, int batch, int dim,
                                 int cell, int32_t *out_coords, int32_t *n_out_dev, void *workspace, size_t workspace_bytes,
                                 const eprecon_mailbox_slot *slot, void *stream);
int eprecon_init_select_dense_mb_async(const float *logit, const int32_t *coords, int64_t n, const int32_t *rank, int grid_x,
                                       int grid_y, int grid_z, int stride, float threshold, int dim, int cell,
                                       int32_t *out_coords, int32_t *n_out_dev, void *workspace, size_t workspace_bytes,
                                       const eprecon_mailbox_slot *slot, void *stream);
/*
 * Sparsify for the next stage (models/neucon_network.py:454-507) in one call: occupancy = occ > threshold; the kept rows of
 * coords / tsdf / occ / feat_all compacted in row order (torch.nonzero + index_select + cat of the reference) and the counts
 * its guards read: counts int32[1 + 2 * batch] = [kept rows, occupied per batch element ..., occupied with an occupied
 * target per batch element ...] (target uint8[n] or NULL = all ones).  Outputs are sized for n rows:
 * out_coords int32[n,4], out_tsdf / out_occ f32[n], out_all f32[n, c_all], out_feat f32[n, c_feat + 2] = [feat_all[:, :c_feat],
 * tsdf, occ] (the next stage's input).  The random sub-sampling branch (:477-484) is not part of it.
 */
size_t eprecon_sparsify_workspace_bytes(int64_t n);
int eprecon_sparsify_async(const float *occ, int ld_occ, float threshold, const unsigned char *target,
                           const int32_t *coords, const float *tsdf, int ld_tsdf, const float *feat_all, int ld_feat,
                           int c_all, int c_feat, int64_t n, int batch, int32_t *out_coords, float *out_tsdf,
                           float *out_occ, float *out_all, float *out_feat, int32_t *counts, void *workspace,
                           size_t workspace_bytes, void *stream);
/*
 * NeuConNet.upsample (models/neucon_network.py:193-214): up_coords int32[8n,4], up_feat f32[8n,C];
 * children of a voxel are consecutive, in the order 0, +x, +y, +z, +xy, +xz, +yz, +xyz (x `interval`).
 * channels == 0 expands the coordinates only; up_coords NULL (channels > 0) expands the features only.
 */
int eprecon_upsample_async(const float *feat, int ld_feat, const int32_t *coords, int64_t n, int channels,
                           int interval, float *up_feat, int32_t *up_coords, void *stream);

/* ------------------------------------------------------------------------------------------
 * Point <-> voxel transfers  (K8, K9) and aligned-camera coordinates (a7)
 *
 * Replaces  r_coords = W2AC[:3] . [c * vs + origin, 1]   models/neucon_network.py:387-398,
 *                                                         models/gru_fusion.py:332-337
 *           initial_voxelize / point_to_voxel / voxel_to_point   ops/torchsparse_utils.py:15-105
 *           (torchsparse F.spcount, F.spvoxelize, F.calc_ti_weights, F.spdevoxelize)
 * Points are f32[n,4] rows (x, y, z, batch) like torchsparse's PointTensor.C.
 * ------------------------------------------------------------------------------------------ */
int eprecon_aligned_coords_async(const int32_t *coords, int64_t n, const float *origin, int batch,
                                 float voxel_size, const float *world_to_aligned_camera, float *out_xyzb,
                                 void *stream);
/* scaled = (x/res, y/res, z/res, b) (IEEE division); voxel = (b, floor x', floor y', floor z') */
int eprecon_point_quantize_async(const float *points_xyzb, int64_t n, float resolution, float *scaled_xyzb,
                                 int32_t *voxel_bxyz, void *stream);
/*
 * The coordinate side of the NEXT SPVCNN pass, queued BEFORE the host has read how many rows a compaction kept
 * (models/neucon_network.py:454-507 keeps the occupied rows, :193-214 expands them to 8 children, :387-398 maps them to the
 * aligned camera frame, ops/torchsparse_utils.py:15-19 scales and floors them): src_coords int32[cap_src,4] with the live row
 * count in *n_src_dev; children != 0: every row -> its 8 children (interval of the new level) in up_coords int32[8 cap_src,4];
 * r_coords / scaled_xyzb f32[cap_pts,4], voxel_bxyz int32[cap_pts,4], *n_points_dev = live points.  One launch sized by the
 * capacity; the unique-voxel numbering (eprecon_unique_coords_dn_async) then runs on *n_points_dev, and the level's size read
 * rides on the read of the compaction's own counts (one blocking read instead of two).  Same arithmetic as
 * eprecon_upsample_async + eprecon_aligned_coords_async + eprecon_point_quantize_async.
 */
int eprecon_spvcnn_points_dn_async(const int32_t *src_coords, int64_t cap_src, const int32_t *n_src_dev, int children,
                                   int interval, const float *origin, int batch, float voxel_size,
                                   const float *world_to_aligned_camera, float resolution, int32_t *up_coords, float *r_coords,
                                   float *scaled_xyzb, int32_t *voxel_bxyz, int32_t *n_points_dev, void *stream);
/* ... with the point count on the device (see eprecon_unique_coords_dn_async) */
int eprecon_point_quantize_dn_async(const float *points_xyzb, int64_t n_cap, const int32_t *n_dev, float resolution,
                                    float *scaled_xyzb, int32_t *voxel_bxyz, void *stream);
/* CSR lists of the points of each voxel: idx int32[n] in [-1, m) -> offsets int32[m+1],
 * order int32[n] (points of voxel v = order[offsets[v] : offsets[v+1]], ascending point index) */
size_t eprecon_segment_workspace_bytes(int64_t n, int64_t m);
int eprecon_segment_lists_async(const int32_t *idx, int64_t n, int64_t m, int32_t *offsets, int32_t *order,
                                void *workspace, size_t workspace_bytes, void *stream);
/* out[v] = mean of feat[p] over the points p of voxel v (0 for empty voxels) — scatter-mean
 * without float atomics */
int eprecon_segment_mean_async(const float *feat, int ld_feat, const int32_t *offsets, const int32_t *order,
                               int64_t m, int channels, float *out, int ld_out, void *stream);
/*
 * Voxel ORDER of the reference.  torchsparse numbers the voxels of initial_voxelize by ascending
 * F.sphash (`torch.unique(pc_hash)`, ops/torchsparse_utils.py:19-21); nothing depends on that order
 * except ConvGRU's second gate convolution (models/modules.py:216-217), which devoxelises with the
 * corner indices cached by the first voxelisation of the same PointTensor into the second voxel
 * set (ops/torchsparse_utils.py:70-71,97-99).  eprecon_sphash_async returns torchsparse's 60-bit
 * FNV-1a hash of every (b,x,y,z) row (hashed in x,y,z,b order); the caller sorts it.
 * eprecon_remap_index_async rewrites cached indices:  out = perm_new[rank_old[idx]]  (-1 stays -1;
 * a rank >= m_new, an out-of-bounds read in the reference, becomes -1).
 */
int eprecon_sphash_async(const int32_t *coords, int64_t n, int64_t *out_hash, void *stream);
/* the whole order in one call (csrc/hash_order.hip): perm_out[k] = row of the voxel with the k-th smallest hash (hashes of
 * distinct voxels are distinct in practice; equal hashes keep their row order), rank_out = the inverse permutation.
 * workspace: eprecon_sphash_order_workspace_bytes(n). */
size_t eprecon_sphash_order_workspace_bytes(int64_t n);
int eprecon_sphash_order_async(const int32_t *coords, int64_t n, int32_t *perm_out, int32_t *rank_out, void *workspace,
                               size_t workspace_bytes, void *stream);
int eprecon_remap_index_async(const int32_t *idx, int64_t n, const int32_t *rank_old, const int32_t *perm_new,
                              int64_t m_new, int32_t *out, void *stream);
/* 8-corner indices int32[n,8] and renormalised trilinear weights f32[n,8] of points (in voxel
 * units) against the voxel set the table was built on, at tensor stride `stride` */
int eprecon_trilinear_map_async(const void *table, uint32_t capacity, const float *points_xyzb, int64_t n,
                                int stride, int32_t *idx8, float *weight8, void *stream);
/* out[i] (+)= sum_k weight8[i,k] * voxel_feat[idx8[i,k]] */
int eprecon_devoxelize_async(const float *voxel_feat, int ld_feat, const int32_t *idx8, const float *weight8,
                             int64_t n, int channels, float *out, int ld_out, int accumulate, void *stream);

/*
 * The tail of SConv3d inside ConvGRU (models/modules.py:193-196,214-221) in one launch:
 * v = devoxelise(voxel_feat) + skip  (skip = the point-wise Linear of SConv3d), then
 *   mode 1: out = sigmoid(v)                    mode 2: out = sigmoid(v) * h
 *   mode 3: out = (1 - zgate) * h + zgate * tanh(v)
 * out may be a column slice of the [r*h, x] concat buffer.
 */
#define EPRECON_GATE_SIGMOID 1
#define EPRECON_GATE_SIGMOID_MUL 2
#define EPRECON_GATE_GRU_MIX 3
int eprecon_devoxelize_gate_async(const float *voxel_feat, int ld_feat, const int32_t *idx8, const float *weight8,
                                  int64_t n, int channels, const float *skip, int ld_skip, int mode, const float *h,
                                  int ld_h, const float *zgate, int ld_z, float *out, int ld_out, void *stream);

/* ... and, in the same launch, tail_dst[i, 0:tail_channels] = tail_src[i, 0:tail_channels]: with mode 2 writing r * h into the
 * first half of the [r*h, x] buffer (models/modules.py:218) the x half is copied alongside, so the buffer needs no clone of [h, x] */
int eprecon_devoxelize_gate_tail_async(const float *voxel_feat, int ld_feat, const int32_t *idx8, const float *weight8,
                                       int64_t n, int channels, const float *skip, int ld_skip, int mode, const float *h,
                                       int ld_h, const float *zgate, int ld_z, float *out, int ld_out, const float *tail_src,
                                       int ld_tail_src, float *tail_dst, int ld_tail_dst, int tail_channels, void *stream);

/* ------------------------------------------------------------------------------------------
 * GRU-fusion union  (K15)
 *
 * Replaces  GRUFusion.convert2dense + the dense gathers    models/gru_fusion.py:67-114,321-326
 *           sparse_to_dense_channel                         utils.py:176-180
 * Union, in raster order of the local dim^3 grid, of (a) the current fragment's voxels
 * (cur_coords int32[n_cur,4] (b,x,y,z) finest units of ONE batch element, divided by `interval`)
 * and (b) the global-map voxels (glob_coords int32[n_glob,3], scene grid units of this scale)
 * shifted by -relative_origin that land inside [0,dim)^3.  A voxel is active when its current or
 * its global feature row has a non-zero channel (activity_mode 0, the reference's
 * `(volume != 0).any(-1)`) or a channel with |v| < 1 (activity_mode 1, TSDF direct substitution).
 *   updated  int32[n_out,3]   src_cur / src_glob int32[n_out] (row or -1)   glob_valid u8[n_glob]
 * ------------------------------------------------------------------------------------------ */
size_t eprecon_fbv_union_workspace_bytes(int dim);
int eprecon_fbv_union_async(const int32_t *cur_coords, const float *cur_feat, int64_t n_cur, int ld_cur,
                            const int32_t *glob_coords, const float *glob_feat, int64_t n_glob, int ld_glob,
                            int channels, int dim, int interval, int activity_mode,
                            const int32_t *relative_origin_host, int32_t *updated, int32_t *src_cur, int32_t *src_glob, uint8_t *glob_valid,
                            int32_t *n_out_dev, void *workspace, size_t workspace_bytes, void *stream);
/* out[i] = src[i] >= 0 ? feat[src[i]] : fill   (rows of `channels` floats) */
int eprecon_gather_rows_async(const float *feat, int ld_feat, const int32_t *src, int64_t n, int channels,
                              float fill, float *out, int ld_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Persistent global map of GRU fusion behind an opaque handle  (K15, SURVEY.md 8b "Ownership")
 *
 * Replaces  GRUFusion.global_volume / target_tsdf_volume state       models/gru_fusion.py:31-38,59-65
 *           convert2dense (crop to the FBV, union, gathers)          models/gru_fusion.py:67-114,321-326
 *           update_map  (map = map[outside FBV] ++ fused rows)       models/gru_fusion.py:195-215
 * A handle owns its device memory (rows int32[M,3] scene-grid coordinates of one scale + f32[M,C]
 * features, ping-pong buffers with geometric growth) and is the ONE stateful object of the ABI:
 * create once per scale, reset on scene change (models/gru_fusion.py:283-286), destroy at the end.
 * One fragment = crop_union -> gather(s) -> [caller fuses] -> update.  Row order after update is the
 * reference's: rows outside the FBV in their old order, then the union voxels in raster order.
 * Calls on one handle must be issued from one thread; crop_union / target_fuse synchronise `stream`
 * (the reference's torch.nonzero synchronises at the same point), the others are stream-ordered.
 * ------------------------------------------------------------------------------------------ */
int eprecon_map_create(int channels, void **out_handle);
int eprecon_map_destroy(void *handle);
int eprecon_map_reset(void *handle);                 /* size := 0, memory kept */
int64_t eprecon_map_size(const void *handle);        /* rows (host-side count) */
int eprecon_map_channels(const void *handle);
/* copy the rows out (coords int32[size,3], feats f32[size,C], both dense) / replace the contents */
int eprecon_map_export_async(const void *handle, int32_t *coords_out, float *feats_out, void *stream);
int eprecon_map_import_async(void *handle, const int32_t *coords, const float *feats, int64_t n, void *stream);
/*
 * Union, in raster order of the local dim^3 grid, of the current fragment's voxels (as in
 * eprecon_fbv_union_async) and the map rows that fall inside the FBV at relative_origin_host.
 * Outputs have capacity min(dim^3, n_cur + size) rows; counts_host[0] = n_out, [1] = map rows inside.
 * The rows inside are remembered by the handle for the next eprecon_map_update_async.  Blocking.
 */
int eprecon_map_crop_union(void *handle, const int32_t *cur_coords, const float *cur_feat, int64_t n_cur, int ld_cur,
                           int dim, int interval, int activity_mode, const int32_t *relative_origin_host,
                           int32_t *updated, int32_t *src_cur, int32_t *src_glob, int64_t *counts_host, void *stream);
/* out[i, 0:channels] = src_glob[i] >= 0 ? map.feats[src_glob[i], col0 : col0 + channels] : fill */
int eprecon_map_gather_async(const void *handle, const int32_t *src_glob, int64_t n, int col0, int channels, float fill,
                             float *out, int ld_out, void *stream);
/* update_map: drop the rows inside the last crop's FBV, append (updated + relative origin, values) */
int eprecon_map_update_async(void *handle, const int32_t *updated, int64_t n, const float *values, int ld_values,
                             void *stream);
/*
 * Ground-truth twin (a 1-channel map; the reference's test path reads the targets,
 * models/neucon_network.py:488): dense volume default 1 <- map rows inside the FBV <- the fragment's
 * ground truth where occ_gt (tsdf_gt f32[dim^3], occ_gt u8[dim^3]); tsdf_target_out[i] = volume at
 * updated[i]; then map = map[outside] ++ raster-ordered cells with |v| < 1.  Blocking.
 */
int eprecon_map_target_fuse(void *handle, const float *tsdf_gt, const uint8_t *occ_gt, int dim,
                            const int32_t *relative_origin_host, const int32_t *updated, int64_t n, float *tsdf_target_out,
                            void *stream);
/*
 * One GRU-fusion level as ONE stream-ordered call with device-side counts  (models/gru_fusion.py:259-345 up to the ConvGRUs:
 * convert2dense + the gathers :321-326, the ground-truth twin :99-113, the fragment's points and their aligned-camera
 * coordinates :328-337, and the coordinate side of the two voxelisations the six SConv3d of the two ConvGRUs share,
 * ops/torchsparse_utils.py:15-35).  Replaces eprecon_map_crop_union (blocking) + 4 gathers + eprecon_map_target_fuse (blocking) +
 * eprecon_aligned_coords_async + 2 x (eprecon_point_quantize_async, eprecon_unique_coords_async + a host read each): nothing
 * here waits for the device.  Every output has `capacity` rows (eprecon_gru_stage_capacity: min(dim^3, n_cur + map rows));
 * counts int32[8] (device) = [0] union voxels n_u, [1] map rows outside the FBV, [2] / [3] unique voxels of the first / second
 * voxelisation, [4] ground-truth cells appended, [5] ground-truth rows kept, [6] / [7] status words of table1 / table2.
 * The caller reads counts back ONCE, hands them to eprecon_gru_stage_commit_async (which finishes the ground-truth twin's
 * update and arms eprecon_map_update_async) and slices its buffers; kernel maps / point lists / corner tables are then built
 * on the exact sizes.  The second voxelisation is that of the ALREADY SCALED points (models/modules.py:216-217 with the
 * in-place z.C of ops/torchsparse_utils.py:33).
 */
typedef struct eprecon_gru_stage_desc {
    void *map;                    /* feature map of this scale (C channels) */
    void *target_map;             /* ground-truth twin (1 channel) or NULL */
    const int32_t *cur_coords;    /* int32[n_cur,4] (b,x,y,z), finest units, ONE batch element */
    const float *cur_feat;        /* f32[n_cur, ld_cur] */
    int64_t n_cur; int ld_cur;
    int dim; int interval; int activity_mode;
    int32_t rel[3];               /* relative origin of the fragment volume in the scene grid of this scale */
    const float *tsdf_gt; const uint8_t *occ_gt;   /* [dim^3] ground truth of the fragment, with target_map */
    const float *origin;          /* f32[3] (device): vol_origin_partial of this batch element */
    const float *w2ac;            /* f32[16] (device): world_to_aligned_camera of this batch element */
    float voxel_size;             /* finest voxel size */
    float resolution;             /* what the SConv3d divide the point coordinates by (vres / pres) */
    int ch_voxel;                 /* channels [0, ch_voxel) feed the voxel ConvGRU, [ch_voxel, C) the image ConvGRU */
    int batch_index;              /* batch column of out_coords */
    int64_t capacity;
    int32_t *updated;             /* int32[cap,3] union cells, raster order */
    int32_t *out_coords;          /* int32[cap,4] (batch_index, cell * interval) */
    float *r_coords;              /* f32[cap,4] aligned-camera (x,y,z,0) */
    float *hx_voxel;              /* f32[cap, 2 ch_voxel]      [h | x]: the map's row, the fragment's row (zeros where absent) */
    float *hx_image;              /* f32[cap, 2 (C - ch_voxel)] */
    float *tsdf_target;           /* f32[cap] ground-truth TSDF at the union cells, with target_map */
    float *scaled1; int32_t *vox1; int32_t *inverse1; int32_t *uniq1; void *table1;   /* f32[cap,4], int32[cap,4], [cap], [cap,4] */
    float *scaled2; int32_t *vox2; int32_t *inverse2; int32_t *uniq2; void *table2;
    uint32_t table_capacity;      /* eprecon_hash_capacity(capacity) */
    int32_t *counts;              /* int32[8] (device) */
    void *workspace; size_t workspace_bytes;   /* eprecon_gru_stage_workspace_bytes(capacity) */
} eprecon_gru_stage_desc;
int64_t eprecon_gru_stage_capacity(const void *map, int64_t n_cur, int dim);
size_t eprecon_gru_stage_workspace_bytes(int64_t capacity);
int eprecon_gru_stage_begin_async(const eprecon_gru_stage_desc *desc, void *stream);
/* counts_host int32[8]: the host copy of desc->counts */
int eprecon_gru_stage_commit_async(void *map, void *target_map, const int32_t *counts_host, void *stream);
/*
 * Multi-GPU boundary exchange on the handle (the schedule of eprecon_amd/distributed.py, which emulates the
 * sequential map updates of models/gru_fusion.py:195-215,275 across ranks).  Every row carries a stamp: 0 unknown,
 * +(fragment + 1) fused by THIS rank, -(fragment + 1) received.  eprecon_map_set_fragment: the global fragment index
 * eprecon_map_update_async stamps its appended rows with (-1: none).  eprecon_map_stamps_async: import / fill / export the
 * int32[size] stamps (in that order; NULL / 0 skips a step).
 *   select  flags the rows fused here that lie inside any box boxes_lo[b] + [0, dim)^3 with b != own_box (device int32[n_boxes,3],
 *           scene-grid units of this scale) and writes their number to count_out (device int32); asynchronous
 *   pack    writes the selected rows in map order as payload f32[n_rows][4 + channels]: (x, y, z, fragment) as int32 bit
 *           patterns, then the features; n_rows = the count select produced (read back by the caller with the other scales')
 *   merge   applies received payload rows that fall inside the local box: per cell the newest copy wins (atomicMax + one
 *           claim), it overwrites the local row when newer than it or is appended in payload order; received rows are
 *           stamped negative so they are not re-broadcast.  Blocking (one host read: the number of appended rows).
 */
int eprecon_map_set_fragment(void *handle, int fragment_index);
int eprecon_map_stamps_async(void *handle, int32_t *export_to, const int32_t *import_from, int fill_all, int32_t fill_value,
                             void *stream);
int eprecon_map_select_boundary_async(void *handle, const int32_t *boxes_lo, int n_boxes, int own_box, int dim,
                                      int32_t *count_out, void *stream);
int eprecon_map_pack_boundary_async(void *handle, float *payload, int64_t n_rows, void *stream);
int eprecon_map_merge_boundary(void *handle, const float *payload, int64_t n_rows, const int32_t *box_lo_host, int dim,
                               int64_t *n_added_host, void *stream);

/* ------------------------------------------------------------------------------------------
 * TSDF integration of depth frames  (the data-preparation side of the path)
 *
 * Replaces  TSDFVolumeTorch.integrate / integrate()     tools/tsdf_fusion/fusion.py:440-485,551-575
 *           (run on the CPU for every sample: datasets/transforms.py:286-297,375-387)
 *           and the in-tree PyCUDA kernel `integrate`   tools/tsdf_fusion/fusion.py:67-142
 * tsdf / weight f32[dims[0], dims[1], dims[2]] (x-major, like the reference's volumes; a fresh volume is
 * tsdf = 1, weight = 0) are updated in place with ALL n_views frames in one launch (per voxel the views
 * are applied in order, as n successive integrate() calls would).  depth f32[n_views, height, width]
 * (metres along the camera z axis, 0 = invalid); intr_host f32[n_views,3,3]; cam_host f32[n_views,4,4]:
 * variant 0 (TSDFVolumeTorch arithmetic) world->camera matrices (the reference's torch.inverse(cam_pose)),
 * variant 1 (the PyCUDA kernel's arithmetic) the camera poses themselves.  trunc = margin * voxel_size.
 * occ_out u8[cells] or NULL: |tsdf| < 0.999 and weight > 1 after the last view (datasets/transforms.py:295-297).
 * dims_host / origin_host / intr_host / cam_host are HOST pointers.
 * ------------------------------------------------------------------------------------------ */
#define EPRECON_TSDF_TORCH 0
#define EPRECON_TSDF_CUDA 1
int eprecon_tsdf_integrate_async(float *tsdf, float *weight, const int32_t *dims_host, const float *origin_host,
                                 float voxel_size, const float *depth, int n_views, int height, int width,
                                 const float *intr_host, const float *cam_host, float trunc, float obs_weight,
                                 int variant, uint8_t *occ_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Fragment ground truth cut out of a scene's full volumes  (the data-preparation side)
 *
 * Replaces  the grid_sample part of RandomTransformSpace.transform     datasets/transforms.py:263-359,367-424
 * One launch per sample fills the targets of all `levels` (<= 3) resolutions.  Level l has
 * ceil(dims / 2^l) output voxels per axis (the reference's `::2**l` slices of the finest coordinates) and
 * samples the scene volume of that level, full_dims[l] cells (x-major; the levels' dims are independent).
 * Per output voxel i (finest cells i * 2^l), in fp32 and the reference's operation order:
 *   X = i * voxel_size + origin_partial;  w = transform[:3,:] @ [X,1];  c = (w - old_origin) / voxel_size / 2^l;
 *   n = 2 c / (D - 1) - 1;  u = ((n + 1) D - 1) / 2   (grid_sample, align_corners = False);  nearest = rint(u)
 *   tsdf_out      the nearest value; the trilinear value (outside corners count 0) where |nearest| < 1;
 *                 1 where some |n| >= 1
 *   rgb_out [.,3] / semantic_out / instance_out   the nearest value as f32, 0 out of range or where some |n| >= 1
 * transform f32[3][4]: rows 0..2 of the inverse augmentation (HOST values, like origin_partial / old_origin:
 * the struct is read during the call).  rgb_full f32[X,Y,Z,3]; semantic_full / instance_full int32.  The colour,
 * semantic and instance pointers of a level may be NULL (source and output together): the TSDF-only form.
 * EPRECON_ERR_ARG: NULL tsdf pointers, a source without its output, levels outside 1..3, dims <= 0;
 * EPRECON_ERR_UNSUPPORTED: a scene axis of one cell, more than 2^31 - 1 cells.  No workspace, no host read.
 * ------------------------------------------------------------------------------------------ */
typedef struct eprecon_gt_crop_desc {
    const float *tsdf_full[3];
    const float *rgb_full[3];
    const int32_t *semantic_full[3];
    const int32_t *instance_full[3];
    int32_t full_dims[3][3];
    int32_t levels;
    int32_t dims[3];          /* the fragment volume at the finest level */
    float voxel_size;         /* of the finest level */
    float origin_partial[3];
    float old_origin[3];      /* world position of cell (0,0,0) of the scene volumes */
    float transform[12];
    float *tsdf_out[3];
    float *rgb_out[3];
    float *semantic_out[3];
    float *instance_out[3];
} eprecon_gt_crop_desc;
int eprecon_gt_crop_async(const eprecon_gt_crop_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scene ground truth from a labelled point cloud  (csrc/label_volume.hip: the offline step that writes the
 * files the fragment ground truth above is cut from)
 *
 * Replaces  integrate_semantic + the coordinate step     tools/tsdf_fusion/generate_gt.py:77-114,199-202
 *           the NearestNDInterpolator fill               datasets/scannet/label_interpolate.py:25-48
 *
 * eprecon_label_volumes (BLOCKING: one int32 read at the end, the label range check):
 *   xyz / rgb f64[n,3], semantic / instance int64[n] on the device; vol_min_host f64[3], dims_host int32[3] HOST.
 *   cell = clip(rint((xyz - vol_min) / voxel_size), 0, dim - 1) in float64, ties to even.
 *   rgb_out f64[X,Y,Z,3]   per-cell sum in ascending point index / max(count, 1)   (bit-reproducible: no atomics)
 *   semantic_out / instance_out int64[X,Y,Z]   the cell's most frequent label, the smallest on a tie; 0 when empty
 *   EPRECON_ERR_ARG: a label outside [0, 32767] (the outputs are then undefined), dims <= 0, voxel_size <= 0;
 *   EPRECON_ERR_UNSUPPORTED: more than 2^31 - 257 cells or points.
 *
 * eprecon_label_fill_async: vol int32[X,Y,Z] -> out int32[X,Y,Z] (out != vol), every cell the label of a nearest
 *   non-zero cell by exact integer squared distance; all zero when vol is.  Among equidistant sites: the smallest
 *   |dx|, then the lower x, then the smallest |dy|, the lower y, the smallest |dz|, the lower z.
 *   EPRECON_ERR_UNSUPPORTED: an axis above 4,096 (checked before any pointer is looked at).
 * ------------------------------------------------------------------------------------------ */
size_t eprecon_label_volumes_workspace_bytes(int64_t n, int64_t cells);
int eprecon_label_volumes(const double *xyz, const double *rgb, const int64_t *semantic, const int64_t *instance,
                          int64_t n, const double *vol_min_host, double voxel_size, const int32_t *dims_host,
                          double *rgb_out, int64_t *semantic_out, int64_t *instance_out, void *workspace,
                          size_t workspace_bytes, void *stream);
size_t eprecon_label_fill_workspace_bytes(int dx, int dy, int dz);
int eprecon_label_fill_async(const int32_t *vol, const int32_t *dims_host, int32_t *out, void *workspace,
                             size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scene mesh extraction: marching cubes on the dense scene TSDF  (scene output path)
 *
 * Replaces  skimage.measure.marching_cubes(tsdf_vol, level=0) + the vertex label lookups of
 *           SaveScene.tsdf2mesh / tsdf_panoptic2mesh                       utils.py:225-241
 * so the dense volumes of GRUFusion.save_mesh (models/gru_fusion.py:217-257) become a mesh on the device.
 * volume f32[dx,dy,dz] (x-major).  Two phases: _count (blocking: one host read of the sizes, the scanned
 * offsets stay in `workspace`), then _emit_async into caller buffers: verts f32[nv,3] in voxel
 * coordinates (the caller applies voxel_size / origin like utils.py:228), normals f32[nv,3] (unit field
 * gradient) or NULL, faces int32[nt,3] wound along the gradient; vert_label_a/b int32[nv]: labels of the
 * voxel nearest to each vertex from two optional int32 volumes (semantic / instance).
 * Vertices are the sign-change points any marching-cubes variant yields; the triangulation table is
 * generated from one rule (csrc/marching_cubes.hip) — skimage's Lewiner tables are not reproduced.
 * ------------------------------------------------------------------------------------------ */
int eprecon_marching_cubes_table(int8_t *out_host /* [256][16] */);
size_t eprecon_marching_cubes_workspace_bytes(int dx, int dy, int dz);
int eprecon_marching_cubes_count(const float *volume, int dx, int dy, int dz, float level, int64_t *counts_host,
                                 void *workspace, size_t workspace_bytes, void *stream);
int eprecon_marching_cubes_emit_async(const float *volume, int dx, int dy, int dz, float level, float *verts, float *normals,
                                      int32_t *faces, const int32_t *label_a, const int32_t *label_b, int32_t *vert_label_a,
                                      int32_t *vert_label_b, const void *workspace, void *stream);
/* Trimmed form (scene evaluation, eprecon_amd/evaluation.py): the same two phases restricted to the cells whose eight
 * corners all have weight > 0 in weight f32[dx,dy,dz] (open3d's ExtractTriangleMesh rule: a re-fused volume keeps its
 * initial TSDF 1 where no view reached, which would otherwise mesh into a spurious copy of every surface at -sdf_trunc).
 * A cut edge carries a vertex only when one of its (up to four) cells takes part.  Workspace: as above. */
int eprecon_marching_cubes_count_masked(const float *volume, const float *weight, int dx, int dy, int dz, float level,
                                        int64_t *counts_host, void *workspace, size_t workspace_bytes, void *stream);
int eprecon_marching_cubes_emit_masked_async(const float *volume, const float *weight, int dx, int dy, int dz, float level,
                                             float *verts, float *normals, int32_t *faces, const int32_t *label_a,
                                             const int32_t *label_b, int32_t *vert_label_a, int32_t *vert_label_b,
                                             const void *workspace, void *stream);

/* ------------------------------------------------------------------------------------------
 * Scene evaluation  (csrc/mesh_eval.hip; tools/evaluation.py + tools/evaluation_utils.py of the reference)
 *
 * Depth rasteriser  (replaces pyrender's OpenGL render of the predicted mesh at every camera pose)
 *   verts f32[nv,3] (world), faces int32[nf,3]; cams f64[9 + 9 + 12 n_views] on the device: K (row-major 3x3),
 *   K^-1, then per view the world->camera 3x4 (camera x right, y down, z forward).  depth_out f32[n_views,h,w]:
 *   camera-frame z of the nearest surface with znear <= z <= zfar, 0 where nothing is hit.  Pixel (r, c) samples
 *   the ray through image point (c + pixel_center, r + pixel_center).  Coverage: signs of the triple products of the
 *   ray with the three edge planes through the camera centre (inclusive); cull_back: a face is drawn only if
 *   ((v1-v0) x (v2-v0)) . v0_cam < 0.  Z-buffer by atomicMin on the fp32 bits: run-to-run bit-identical.
 *   Five fixed launches for all views; workspace: eprecon_render_depth_workspace_bytes(queue_capacity).
 * ------------------------------------------------------------------------------------------ */
size_t eprecon_render_depth_workspace_bytes(int64_t queue_capacity);
int eprecon_render_depth_async(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *cams,
                               int n_views, int height, int width, float pixel_center, float znear, float zfar, int cull_back,
                               float *depth_out, int64_t queue_capacity, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * View rendering  (csrc/mesh_render.hip; tools/render.py and VIS_INCREMENTAL of the reference open a pyrender window)
 *
 * Visibility buffer  (the depth rasteriser's walk, setup, coverage and depth: csrc/mesh_raster.hpp)
 *   verts, faces, cams, pixel_center, znear, zfar, cull_back, queue_capacity: as eprecon_render_depth_async.
 *   vis_out u64[n_views,h,w]: (fp32 depth bits << 32) | face index of the nearest drawn face, lowered by a 64-bit
 *   atomicMin from all-ones; "no hit" is an upper word at or above the +inf bits 0x7F800000.  Run-to-run
 *   bit-identical; the upper word equals the depth render's z-buffer bit for bit; at equal depth bits the smallest
 *   face index wins.  Four fixed launches; workspace: eprecon_render_visibility_workspace_bytes(queue_capacity).
 *
 * Resolve  (one thread per pixel; every output is optional: a null pointer skips it)
 *   The winning face is rebuilt in the camera frame and its corners weighed by the ray's triple products
 *   w_a : w_b : w_c = d.(b x c) : d.(c x a) : d.(a x b); "the corner" is the one with the largest |w| (the earlier
 *   slot of the face on ties).  depth_out f32 (0 where nothing is hit), face_out int32 (-1), corner_out int32: that
 *   corner's vertex index (-1), label_a_out / label_b_out int32: labels_a / labels_b int32[nv] at that corner
 *   (background_a / background_b), rgb_out u8[n_views,h,w,3]: min(255, floor(c I + 0.5)) with
 *   I = ambient + (1 - ambient) |n^ . d^| (unit face normal, unit pixel ray, fp64) and c the corner's colour in
 *   colors u8[nv,3] (153 when colors is null); (bg_red, bg_green, bg_blue) where nothing is hit.  A word of vis whose face
 *   index is not a drawable face of this mesh counts as no hit.  One launch.
 * ------------------------------------------------------------------------------------------ */
size_t eprecon_render_visibility_workspace_bytes(int64_t queue_capacity);
int eprecon_render_visibility_async(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *cams,
                                    int n_views, int height, int width, float pixel_center, float znear, float zfar,
                                    int cull_back, uint64_t *vis_out, int64_t queue_capacity, void *workspace,
                                    size_t workspace_bytes, void *stream);
int eprecon_render_resolve_async(const uint64_t *vis, const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                                 const double *cams, int n_views, int height, int width, float pixel_center, float *depth_out,
                                 int32_t *face_out, int32_t *corner_out, const int32_t *labels_a, int32_t background_a,
                                 int32_t *label_a_out, const int32_t *labels_b, int32_t background_b, int32_t *label_b_out,
                                 const uint8_t *colors, double ambient, int bg_red, int bg_green, int bg_blue,
                                 uint8_t *rgb_out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Vertex colours from posed colour frames  (csrc/mesh_colorize.hip; the project's own rule)
 *
 * Accumulate  (one thread per vertex, the call's views looped in ascending order, no atomics)
 *   verts f32[nv,3] (world), faces int32[nf,3].  cams f64[9 + 9 + 12 n_views] on the device: K_color (row-major 3x3, the
 *   intrinsics of the frames), K_vis (the intrinsics of the visibility buffer), then per view the world->camera 3x4;
 *   both K with the last row 0 0 1.  frames u8[n_views,hc,wc,3] (hc, wc >= 2), vis u64[n_views,hd,wd]: the
 *   visibility buffer of THIS mesh from the same views (eprecon_render_visibility_async at K_vis).  Everything fp64,
 *   sums associated (a x + b y) + c z.  Per vertex p and view, the pair is kept only if all of these hold:
 *     q = w2c p,  z = q.z,  znear <= z <= zfar;
 *     (u_d, v_d) = (K_vis q) * (1 / z), cd = floor(u_d - pixel_center + 0.5), rd likewise from v_d, inside the buffer;
 *     the word at (rd, cd) is a hit: upper word < 0x7F800000 and its face index a drawable face (< nf, corners in
 *     range: the tests of eprecon_render_resolve_async), and z <= D + tolerance with D the word's fp32 depth;
 *     n = the plane normal (b-a) x (c-a) of that face in the camera frame, |n| > 0, cos = |n.q| / (|n| |q|) >= min_cos;
 *     (u_c, v_c) = (K_color q) * (1 / z), x = u_c - pixel_center, y = v_c - pixel_center, 0 <= x <= wc-1, 0 <= y <= hc-1.
 *   Then x0 = min(floor(x), wc-2), fx = x - x0, the same for y; per channel the bilinear value
 *   (1-fy) ((1-fx) c00 + fx c01) + fy ((1-fx) c10 + fx c11) of the four bytes; w = cos / z^2;
 *   acc f64[nv,4] += (w r, w g, w b, w), seen int32[nv] += 1.  acc and seen are the caller's state (zero before the
 *   first call); each vertex's sums are one sequential chain over the views of a call and over calls, so the result
 *   is bit-identical run to run and however the views are split into calls.  Argument rules return
 *   EPRECON_ERR_ARG; nv == 0 or n_views == 0 is a no-op.  One launch per 64 views.
 *
 * Finish  (one thread per vertex)
 *   rgb_out u8[n,3]: min(255, floor(acc_c / acc_w + 0.5)) where seen >= min_views and acc_w > 0, else the fallback bytes.
 * ------------------------------------------------------------------------------------------ */
int eprecon_colorize_accumulate_async(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *cams,
                                      int n_views, const uint8_t *frames, int hc, int wc, const uint64_t *vis, int hd, int wd,
                                      float pixel_center, float znear, float zfar, double tolerance, double min_cos, double *acc,
                                      int32_t *seen, void *stream);
int eprecon_colorize_finish_async(const double *acc, const int32_t *seen, int64_t n, int min_views, int fallback_red,
                                  int fallback_green, int fallback_blue, uint8_t *rgb_out, void *stream);

/* Depth metrics (eval_depth of tools/evaluation_utils.py, batched): pred, trgt f32[n_frames, n_pix].  sums_out
 * f64[n_frames, 10] per frame, in a fixed order (run-to-run bit-identical): valid pixels (pred > 0, 0 < trgt < 10),
 * pixels with pred > 0, then over the valid pixels sum |p-t|/t, |p-t|, (p-t)^2/t, (p-t)^2, (ln p - ln t)^2 and the
 * counts of max(p/t, t/p) < 1.25, 1.25^2, 1.25^3 (fp64 per element).  workspace: _workspace_bytes(n_frames). */
size_t eprecon_depth_metrics_workspace_bytes(int n_frames);
int eprecon_depth_metrics_async(const float *pred, const float *trgt, int n_frames, int64_t n_pix, double *sums_out,
                                void *workspace, size_t workspace_bytes, void *stream);

/* Bounding box of a point cloud: points f32[n,3] -> out f32[6] (min xyz, max xyz) on the device; n >= 1.
 * workspace: 256 x 6 floats (the per-block partials). */
int eprecon_point_bounds_async(const float *points, int64_t n, float *out, float *workspace, void *stream);

/* Voxel down-sample (open3d VoxelDownSample): idx = floor((p - min_bound) / voxel) in fp64, dims = the index range
 * (from the host); out f32[<= n, 3] = the mean of every occupied voxel's points in voxel-key (x, y, z) order;
 * *n_out_host = voxels.  The per-voxel sums are exact integer sums of 2^-36-voxel fixed-point offsets from the voxel's
 * lowest-index point (no float atomics: bit-identical from run to run; <= 2^27 points per voxel).  Blocking (one host
 * read per x slab).
 * workspace: _workspace_bytes(n, slab_cells), slab_cells >= dims[1] * dims[2]. */
size_t eprecon_voxel_down_sample_workspace_bytes(int64_t n, int64_t slab_cells);
int eprecon_voxel_down_sample(const float *points, int64_t n, const double *min_bound_host, double voxel,
                              const int64_t *dims_host, float *out, int64_t *n_out_host, int64_t slab_cells, void *workspace,
                              size_t workspace_bytes, void *stream);

/* Exact nearest neighbour (nn_correspondance of tools/evaluation_utils.py): for every query point the nearest
 * reference point (squared distance in fp64, the smallest index on ties) -> idx_out int64[n_query], dist_out
 * f32[n_query].  The reference points are bucketed into a uniform grid (lo_host, cell, dims_host from the host; every
 * reference point inside it); each query visits shells of cells until no unvisited cell can beat its best distance.
 * n_ref, n_query >= 1.  workspace: _workspace_bytes(n_ref, dims[0] * dims[1] * dims[2]). */
size_t eprecon_nn_search_workspace_bytes(int64_t n_ref, int64_t n_cells);
int eprecon_nn_search_async(const float *ref, int64_t n_ref, const float *query, int64_t n_query, const double *lo_host,
                            double cell, const int32_t *dims_host, int64_t *idx_out, float *dist_out, void *workspace,
                            size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Panoptic export: voxel labels onto mesh vertices  (tools/generate_semantic_instance.py)
 *
 * The sites are the cells of a dense label volume (semantic, instance int32[X,Y,Z], dims_host int32[3]) whose class
 * maps to a non-zero id: mapping_host int32[n_map] (host memory, 1 <= n_map <= 256), site <=> mapping[semantic] != 0.
 * A site's world coordinate per axis is fl64(fl64(i) * voxel_size) + fl64(origin_host[a]) (numpy's
 * idx * voxel_size + origin with a float64 voxel size and a float32 origin); no cloud of them is ever built.
 * More than 2^31 - 1 cells: EPRECON_ERR_UNSUPPORTED.
 *
 * eprecon_label_bricks_async: masks_out uint64[ceil(X/4) * ceil(Y/4) * ceil(Z/4)] (brick (bx, by, bz) at
 *   (bx * BY + by) * BZ + bz), bit (x & 3) << 4 | (y & 3) << 2 | (z & 3) of a brick's word = that cell is a site (cells
 *   outside the volume: 0).  status_out int32[2] on the device (cleared here): [0] != 0 when a semantic value lies outside
 *   [0, n_map) (the masks are then not to be used), [1] the number of sites.
 * eprecon_label_transfer_async: query f32[n_query,3] -> per vertex the nearest site in squared fp64 distance
 *   (dx*dx + dy*dy) + dz*dz, every operation rounded on its own; among equal distances the smallest linear cell index
 *   (x * Y + y) * Z + z.  idx_out int32 (that index), dist_out f32 (of the fp64 root), sem_out int32
 *   (mapping[semantic[idx]]), ins_out int32 (instance[idx]); no site at all: -1, +inf, 0, 0.  One thread per vertex
 *   walks its own brick and near_shells shells of bricks around it; a vertex not decided by then is queued on the
 *   device and finished by one wave each (near_shells < 0: every vertex goes to the waves; near_shells > 2^30: none).
 *   The result does not depend on the path.  n_query == 0 is a no-op.
 *   workspace: eprecon_label_transfer_workspace_bytes(dims_host, n_query) (0 for an unsupported volume).
 * eprecon_instance_vote_async: mapped_sem int32[n] in [0, n_class), rank int32[n] in [0, n_inst) -> per instance rank
 *   class_out int32[n_inst] = the class with the most vertices, among equal counts the one whose first vertex has the
 *   smallest index (CPython's Counter(...).most_common(1)), count_out int32[n_inst] = its vertices (all classes).
 *   Integer atomics only.  workspace: n_inst * n_class * 8 bytes (+ 256); entries out of range are ignored.
 * ------------------------------------------------------------------------------------------ */
size_t eprecon_label_transfer_workspace_bytes(const int32_t *dims_host, int64_t n_query);
int eprecon_label_bricks_async(const int32_t *semantic, const int32_t *dims_host, const int32_t *mapping_host, int n_map,
                               uint64_t *masks_out, int32_t *status_out, void *stream);
int eprecon_label_transfer_async(const uint64_t *masks, const int32_t *semantic, const int32_t *instance,
                                 const int32_t *dims_host, const float *origin_host, double voxel_size,
                                 const int32_t *mapping_host, int n_map, const float *query, int64_t n_query, int near_shells,
                                 int32_t *idx_out, float *dist_out, int32_t *sem_out, int32_t *ins_out, void *workspace,
                                 size_t workspace_bytes, void *stream);
int eprecon_instance_vote_async(const int32_t *mapped_sem, const int32_t *rank, int64_t n, int n_inst, int n_class,
                                int32_t *class_out, int32_t *count_out, void *workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------------------------
 * Panoptic scoring: the contingency table of predicted and ground-truth segments  (eprecon_amd/panoptic_score.py;
 * the reference ships no scoring code: the rules are DESIGN.md 5b's)
 *
 * counts int64[(n_pred + 1) * (n_gt + 2)], row-major, cleared by the call: counts[p * (n_gt + 2) + g] = the sites of
 * predicted segment p and ground-truth segment g.  A predicted rank lies in [-1, n_pred): -1 ("no prediction") is row
 * n_pred.  A ground-truth rank lies in [-1, n_gt]: n_gt is the void column, -1 ("no ground truth here") is column
 * n_gt + 1.  A site with a rank outside its range is skipped and status[0] (int32[2] on the device, cleared by the call)
 * is set; status[1] is not used.  One integer add per distinct pair of a wave at the most (a wave carries the pair it met
 * last from one round of sites to the next); a table of up to 8,192 entries is summed per workgroup in LDS first
 * (EPRECON_PC_LDS=0: never).  Integer adds only: the table depends neither on the order nor on that path.
 * n_pred, n_gt < 0: EPRECON_ERR_ARG; (n_pred + 1) * (n_gt + 2) > 2^22: EPRECON_ERR_UNSUPPORTED, before any launch.
 *
 * eprecon_pair_count_async: the sites are the n entries of two rank lists.
 * eprecon_voxel_pair_count_async: the sites are the cells k of a lattice box (lattice_lo_host int32[3] its first cell,
 *   which may be negative, lattice_dims_host int32[3] its extent, z fastest, fewer than 2^31 cells) on the PREDICTION's
 *   grid.  World position per axis w = fl64(pred_origin_host[a]) + fl64(k) * pred_voxel.  The prediction's rank is
 *   pred_rank[k] when k lies inside pred_dims_host, else -1.  The ground-truth cell is j = floor((w - fl64(gt_origin_host[a]))
 *   / gt_voxel + 0.5), every operation in fp64 and rounded on its own; the ground-truth rank is gt_rank[j] when j lies inside
 *   gt_dims_host and fabsf(gt_tsdf[j]) < gt_surface (compared in fp32), else -1.  Volumes are [X,Y,Z] with z fastest.
 * ------------------------------------------------------------------------------------------ */
int eprecon_pair_count_async(const int32_t *pred_rank, const int32_t *gt_rank, int64_t n, int n_pred, int n_gt, int64_t *counts,
                             int32_t *status, void *stream);
int eprecon_voxel_pair_count_async(const int32_t *pred_rank, const int32_t *gt_rank, const float *gt_tsdf,
                                   const int32_t *pred_dims_host, const int32_t *gt_dims_host, const float *pred_origin_host,
                                   const float *gt_origin_host, double pred_voxel, double gt_voxel, float gt_surface,
                                   const int32_t *lattice_lo_host, const int32_t *lattice_dims_host, int n_pred, int n_gt,
                                   int64_t *counts, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Object inventory: per-segment statistics of voxel rows  (csrc/segment_stats.hip, eprecon_amd/scene_objects.py; the
 * reference has no counterpart: the rule is DESIGN.md 5b's)
 *
 * coords int32[m,3] (x, y, z) and rank int32[m] on the device; m < 2^24 and n_segments <= 2^24, else
 * EPRECON_ERR_UNSUPPORTED before any launch.  Row i takes part when 0 <= rank[i] < n_segments and every |coordinate| is at
 * most 2^19 - 2 (the hash grid's range).  The rank is looked at first: -1 ("nothing here") and n_segments (void) are skipped
 * silently; any other rank outside the range is skipped and sets status |= 1; a row with a rank in range and a coordinate
 * out of range is skipped and sets status |= 2.  status int32[1] and the whole output are initialised by the call (one
 * launch), so the caller passes uninitialised buffers; a segment without rows keeps the initial values.  m == 0 or
 * n_segments == 0: nothing but that initialisation is launched and no row is looked at.
 *
 * eprecon_segment_moments_async: table int64[n_segments,16]: column 0 the count; 1-3 the sums of x, y, z; 4-9 the sums of
 *   xx, xy, xz, yy, yz, zz (below 2^62 under the limits above); 10-12 min x, y, z (initially INT32_MAX); 13-15 max x, y, z
 *   (initially INT32_MIN).
 * eprecon_segment_extents_async: with (c, s) = dirs[rank] (double[n_segments,2], finite), u = fl(fl(x c) + fl(y s)) and
 *   v = fl(fl(y c) - fl(x s)) in fp64, ext double[n_segments,4] = (min u, max u, min v, max v), initially (+inf, -inf,
 *   +inf, -inf).  A zero counts as +0, so the bits are the same on every run.
 *
 * Integer sums and min / max only: the output depends neither on the order nor on the path.  With up to
 * eprecon_segment_stats_lds_segments() segments the updates are combined per workgroup in LDS first and sent to memory once
 * per workgroup (EPRECON_SS_LDS=0: never); above it every update goes straight to memory.
 * ------------------------------------------------------------------------------------------ */
int32_t eprecon_segment_stats_lds_segments(void);
int eprecon_segment_moments_async(const int32_t *coords, const int32_t *rank, int64_t m, int32_t n_segments, int64_t *table,
                                  int32_t *status, void *stream);
int eprecon_segment_extents_async(const int32_t *coords, const int32_t *rank, int64_t m, int32_t n_segments, const double *dirs,
                                  double *ext, int32_t *status, void *stream);

/* ------------------------------------------------------------------------------------------
 * Mesh simplification: quadric vertex clustering  (csrc/mesh_simplify.hip, eprecon_amd/simplify.py; the reference has no
 * counterpart, its users run open3d's simplify_vertex_clustering on the .ply: the rule is DESIGN.md 5b's)
 *
 * verts f32[n,3], faces int32[m,3] on the device; origin_host double[3] and cell > 0 on the host; n < 2^31 and 3 m < 2^31,
 * at most eprecon_simplify_max_clusters() = 2^21 clusters, else EPRECON_ERR_UNSUPPORTED before any launch.  status int32[1]
 * is cleared by the call that takes it and collects: 1 a face index outside [0, n); 2 a vertex that is not finite; 4 a cell
 * outside [-2^20, 2^20).
 *
 * eprecon_simplify_keys_async: key int64[n] = (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20) with
 *   c = floor((double(v) - origin) / cell) per axis, every operation rounded in fp64; -1 for a vertex with status 2 or 4.
 * eprecon_simplify_faces_async: cluster int32[n] (the caller's ranks, in [0, n_clusters)) -> tri int32[m,3] the clusters of
 *   the corners (-1 three times for a face with status 1: such a face has no corner entries); face_key int64[m] the sorted
 *   triple, 21 bits each (-1 for a face with status 1 or with two equal clusters); referenced uint8[n_clusters] (cleared by
 *   the call) 1 for every cluster of a face with three different clusters.
 * eprecon_simplify_quadrics_async: with the CSR lists of eprecon_segment_lists_async over tri (3 m entries) and over
 *   cluster (n entries): per cluster, relative to the centre origin + (c + 0.5) cell of its cell, the mean of its members,
 *   the area-weighted plane quadrics (A, b) and the sum of the face normals over its corner entries in ascending order
 *   (faces of zero area skipped), x* from (A + l I) x = b + l mean with l = regularize trace(A) / 3 (the mean when the trace
 *   is 0), and pos double[n_clusters,3] = centre + mean + t (x* - mean) with the largest t in [0, 1] that stays in the
 *   cell's closed box; normal f32[n_clusters,3] the normalised normal sum (0 when its length is 0); with colors uint8[n,3],
 *   rgb uint8[n_clusters,3] = (2 sum + count) / (2 count) in integers.  One lane per cluster, every sum in list order: the
 *   same bits on every run.  regularize > 0.
 * ------------------------------------------------------------------------------------------ */
int32_t eprecon_simplify_max_clusters(void);
int eprecon_simplify_keys_async(const float *verts, int64_t n, const double *origin_host, double cell, int64_t *key, int32_t *status,
                                void *stream);
int eprecon_simplify_faces_async(const int32_t *faces, int64_t m, const int32_t *cluster, int64_t n, int32_t n_clusters, int32_t *tri,
                                 int64_t *face_key, uint8_t *referenced, int32_t *status, void *stream);
int eprecon_simplify_quadrics_async(const float *verts, int64_t n, const int32_t *faces, int64_t m, const uint8_t *colors,
                                    const int64_t *key, const int32_t *corner_offsets, const int32_t *corner_order,
                                    const int32_t *member_offsets, const int32_t *member_order, int32_t n_clusters,
                                    const double *origin_host, double cell, double regularize, double *pos, float *normal, uint8_t *rgb,
                                    void *stream);

/* ------------------------------------------------------------------------------------------
 * Nearest finest-level voxel  (K18)
 *
 * Replaces  torch.cdist + argmin(dim=1)                 models/mask3dformer.py:361-367
 * out_index[i] = row of the reference voxel (ref_coords int32[m,4] (b,x,y,z), hashed in `table`)
 * nearest to query_coords[i] (a voxel of a coarser level, multiple of `quantum`) in exact integer
 * Euclidean distance, smallest row on ties, same batch element; -1 when that batch element has no
 * reference voxel.
 * ------------------------------------------------------------------------------------------ */
int eprecon_nearest_voxel_async(const void *table, uint32_t capacity, const int32_t *ref_coords,
                                int64_t m, const int32_t *query_coords, int64_t n, int quantum,
                                int32_t *out_index, void *stream);

/* ------------------------------------------------------------------------------------------
 * Voxel side of the mask-transformer decoder  (K19)
 *
 * Replaces  the per-level inputs of MultiScaleMaskedTransformerDecoder.forward      models/mask3dformer.py:346-357
 *           (PositionEmbeddingCoordsSine "fourier", normalize=True                   models/voxel_position_encoding.py:123-152)
 *           the masked cross-attention of a decoder layer                            models/mask3dformer.py:383-397
 *           with the attention mask of forward_prediction_heads                      models/mask3dformer.py:429-445
 *
 * eprecon_decoder_keys_async: coords int32 rows (x, y, z) with row pitch ld_coords ints, feats f32[n, ld_feats]:
 *   src[i, c] = feats[i, c] + level_embed[c];  keys[i, c] = src[i, c] + pos[i, c],
 *   pos = [sin(P), cos(P)], P = (2 pi * coords / extent) @ gauss_b   (gauss_b f32[3, channels / 2], extent_host f32[3] HOST)
 *
 * eprecon_masked_attention_async: out f32[H, Q, D] = softmax_over_allowed_keys(scale * q k^T) v per head; q element
 *   (h, i, d) at q[h * q_stride_head + i * q_stride_query + d] (the head-split VIEW of a [Q, H * D] in-projection is taken as is),
 *   k / v f32[n_keys, ld] rows whose H * D channels are the heads side by side (what nn.MultiheadAttention's in-projection
 *   produces).  Key n is BLOCKED for query i when sigmoid(mask_logits_t[row(n), i]) < 0.5 with row(n) = mask_rows[n]
 *   (NULL: n); mask_logits_t f32[n_mask_rows, ld_mask] is the TRANSPOSED mask-logit matrix (voxel-major).  A query whose
 *   mask blocks every key attends to all keys (models/mask3dformer.py:388).  mask_logits_t NULL: no mask.
 *   Shapes taken: D = 6, H even, Q * H / 2 <= 512, Q <= 255, k / v 16-byte aligned with ld % 4 == 0;
 *   EPRECON_ERR_UNSUPPORTED otherwise (callers keep the dense PyTorch path).  Deterministic (fixed merge order).
 * ------------------------------------------------------------------------------------------ */
int eprecon_decoder_keys_async(const int32_t *coords, int ld_coords, const float *feats, int ld_feats, const float *level_embed,
                               const float *gauss_b, const float *extent_host, int64_t n, int channels, float *src_out,
                               float *keys_out, void *stream);
size_t eprecon_masked_attention_workspace_bytes(int64_t n_keys, int n_queries, int n_heads, int head_dim);
int eprecon_masked_attention_async(const float *q, int q_stride_head, int q_stride_query, const float *k, int ld_k, const float *v, int ld_v, int64_t n_keys,
                                   const float *mask_logits_t, int ld_mask, const int32_t *mask_rows, int64_t n_mask_rows,
                                   int n_queries, int n_heads, int head_dim, float scale, float *out, void *workspace,
                                   size_t workspace_bytes, void *stream);

/*
 * Query side of a decoder layer (static shape [Q, C]): out-projection + residual + LayerNorm of the cross-attention whose
 * per-head output is o_attn (eprecon_masked_attention_async), self-attention over the queries, FFN (post-norm blocks,
 * models/mask3dformer.py:33-196,399-427), the prediction head's class logits and mask embedding (:429-436) and the NEXT layer's
 * in-projected queries — two launches instead of ~25.  Every weight matrix is given TRANSPOSED, f32[in][out] row-major
 * (nn.Linear stores [out][in]); self_in_wt is nn.MultiheadAttention.in_proj_weight transposed: f32[C][3C] with the q | k | v
 * columns side by side.  workspace: 4 * Q * C floats.  Shapes taken: Q <= 128, C <= 64 with C % H == 0, H <= 8,
 * ffn_dim / mask_hidden <= 256, n_class_logits <= 64 (EPRECON_ERR_UNSUPPORTED otherwise).
 */
typedef struct eprecon_decoder_layer_desc {
    int n_queries; int channels; int n_heads; int ffn_dim; int n_class_logits; int mask_hidden;
    const float *o_attn;        /* f32[H][Q][C/H] */
    const float *state_in;      /* f32[Q][C] queries entering the layer */
    const float *query_pos;     /* f32[Q][C] */
    const float *cross_out_wt; const float *cross_out_b; const float *cross_ln_g; const float *cross_ln_b;
    const float *self_in_wt; const float *self_in_b; const float *self_out_wt; const float *self_out_b;
    const float *self_ln_g; const float *self_ln_b;
    const float *ffn1_wt; const float *ffn1_b; const float *ffn2_wt; const float *ffn2_b; const float *ffn_ln_g; const float *ffn_ln_b;
    const float *dec_ln_g; const float *dec_ln_b; const float *cls_wt; const float *cls_b;
    const float *m1_wt; const float *m1_b; const float *m2_wt; const float *m2_b; const float *m3_wt; const float *m3_b;
    const float *next_q_wt; const float *next_q_b;     /* the next layer's cross-attention q in-projection, or NULL */
    float ln_eps;
    float *state_out;           /* f32[Q][C] */
    float *cls_out;             /* f32[Q][n_class_logits] */
    float *mask_embed_out;      /* f32[Q][C] */
    float *next_q_out;          /* f32[Q][C] or NULL */
    float *workspace;
} eprecon_decoder_layer_desc;
int eprecon_decoder_query_side_async(const eprecon_decoder_layer_desc *desc, void *stream);

/*
 * panoptic_inference on the voxel side (models/mask3dformer.py:515-581 after the per-query softmax / keep decision):
 *   mask_logits f32[Q][ld] (the final head's pred_masks of one batch element), scores f32[Q], keep int32[Q] (label != 0 and
 *   score > threshold) -> owner_out int32[n]: the kept query with the largest score * sigmoid(logit) (first on ties, -1 when
 *   no query is kept), confident_out u8[n]: sigmoid(logit of the owner) >= 0.5, counts_out int32[3][Q]: voxels owned,
 *   voxels with sigmoid >= 0.5, both (zeroed by the call).  Integer atomics only: deterministic.
 * eprecon_panoptic_assign_async: seg[v] = idmap[owner[v]] where the owner is confident, else 0 (idmap int32[Q]: the segment id
 *   the host gave the query, 0 for rejected ones).
 */
int eprecon_panoptic_stats_async(const float *mask_logits, int64_t ld, const float *scores, const int32_t *keep, int n_queries,
                                 int64_t n, int32_t *owner_out, uint8_t *confident_out, int32_t *counts_out, void *stream);
int eprecon_panoptic_assign_async(const int32_t *owner, const uint8_t *confident, const int32_t *idmap, int64_t n, int32_t *seg_out,
                                  void *stream);

/*
 * The per-voxel heads as one launch  (models/modules.py:273-311 Linear4xTrans: Linear(C, 4C) - LayerNorm - ReLU -
 * Linear(4C, C) - LayerNorm - ReLU - Linear(C, C_out), + the second hidden layer as a skip when C == C_out; callers
 * models/neucon_network.py:437-438 tsdf_preds / occ_preds — `heads` = 2: both run on the same rows — and :546-548
 * panoptic_preds).  A wave owns 16 voxels; the chain stays in its registers (csrc/heads.hip).
 *   x f32[n][ld_x]: the first `channels` columns of a row are the input.  y of head h: f32[n][ld_y], out_channels columns.
 *   Weights are handed over PACKED for the kernel's operand order (eprecon_amd/sparse.py pack_mlp4x; all 16-byte aligned):
 *     layer with weight Wt f32[K][M] (in x out)  ->  f32[ceil(M/16)][ceil(K/16)][64][4],
 *     block (t, c), lane l = 16 q + m, component i  =  Wt[16 c + 4 q + i][16 t + m]   (0 outside the matrix);
 *     bias / LayerNorm weight / LayerNorm bias vectors padded with zeros to a multiple of 16.
 * Shapes taken (eprecon_mlp4x_supported): channels 24 / 48 / 96 with out_channels <= 16, channels 48 / 88 / 176 with
 * out_channels 33..48; EPRECON_ERR_ARG otherwise (the caller keeps those on separate launches).
 */
typedef struct eprecon_mlp4x_head {
    const float *w1; const float *b1; const float *g1; const float *be1;   /* Linear(C, 4C), LayerNorm(4C) */
    const float *w2; const float *b2; const float *g2; const float *be2;   /* Linear(4C, C), LayerNorm(C) */
    const float *w3; const float *b3;                                      /* Linear(C, C_out) */
    float *y; int64_t ld_y;
} eprecon_mlp4x_head;
typedef struct eprecon_mlp4x_desc {
    const float *x; int64_t ld_x; int64_t n;
    int channels; int out_channels; int heads; int residual;
    float eps1; float eps2;
    eprecon_mlp4x_head head[2];
} eprecon_mlp4x_desc;
int eprecon_mlp4x_supported(int channels, int out_channels);
int eprecon_mlp4x_async(const eprecon_mlp4x_desc *desc, void *stream);

/* ------------------------------------------------------------------------------------------
 * The 2D feeder's memory-bound layers  (models/backbone.py:22-77 MnasMulti, called once per view in train mode:
 * models/neuralrecon.py:53-54, main.py:357).  Channels-last maps x f32[n][h][w][c], c % 4 == 0, 16-byte aligned.
 *
 * Replaces  nn.Conv2d(groups == channels) of torchvision's MNASNet inverted-residual blocks and the nn.BatchNorm2d behind
 *           every convolution of the trunk, for a batch of views whose statistics must not mix (one BatchNorm call per
 *           view in the reference).
 *
 * eprecon_bn2d_views_stats_async: rows [views][rows_per_view][channels] (a view's images x pixels) -> affine_out
 *   f32[views][2][channels] = (scale, shift) of the train-mode BatchNorm of each view (biased variance, eps inside the root):
 *   y = x * scale + shift.  workspace: eprecon_bn2d_views_workspace_bytes.  Two launches (range summaries, merge in range
 *   order): deterministic.  channels <= 480.
 * eprecon_bn2d_views_apply_async: out = [relu](x * scale + shift) [+ residual]; out may be x.
 * eprecon_dwconv2d_nhwc_async: depthwise ksize x ksize (3 or 5), stride 1 or 2, zero padding ksize / 2, no bias;
 *   weight_taps f32[ksize * ksize][channels] (tap-major: torch's [C,1,k,k] weight transposed).  affine (optional,
 *   f32[views][2][channels]): the producer's pending BatchNorm (+ ReLU when relu != 0) applied to every loaded input value
 *   (padding stays zero); image i belongs to view i / imgs_per_view.  out f32[n][ho][wo][channels].
 * ------------------------------------------------------------------------------------------ */
int eprecon_bn2d_views_chunks(int64_t rows_per_view, int channels);
size_t eprecon_bn2d_views_workspace_bytes(int views, int64_t rows_per_view, int channels);
int eprecon_bn2d_views_stats_async(const float *x, int views, int64_t rows_per_view, int channels, const float *gamma,
                                   const float *beta, float eps, float *affine_out, void *workspace,
                                   size_t workspace_bytes, void *stream);
int eprecon_bn2d_views_apply_async(const float *x, int views, int64_t rows_per_view, int channels, const float *affine, int relu,
                                   const float *residual, float *out, void *stream);
int eprecon_dwconv2d_nhwc_async(const float *x, int n, int height, int width, int channels, const float *weight_taps, int ksize,
                                int stride, const float *affine, int imgs_per_view, int relu, float *out, void *stream);

/*
 * The rest of a GRU-fusion level's geometry after its host read (sizes known), in one call (csrc/gru_stage_finish.hip): for the
 * two voxelisations shared by the six SConv3d of the level's ConvGRUs — CSR point lists (offsets int32[m+1], order int32[n]),
 * 3x3x3 kernel maps int32[27][m], the first voxelisation's trilinear corner tables (idx8 int32[n][8], weight8 f32[n][8]) and
 *   literal != 0 (the reference's convr, models/modules.py:216-217): the hash order of both sets (perm / rank int32[m]) and
 *                idx8_2 = the FIRST tables' indices carried to the second set in hash order (eprecon_remap_index_async);
 *   literal == 0: the second voxelisation's own corner tables (idx8_2, weight8_2 from scaled2).
 * Replaces the same sequence of single calls (eprecon_segment_lists_async, eprecon_kernel_map_async,
 * eprecon_trilinear_map_async, eprecon_sphash_order_async, eprecon_remap_index_async): bit-identical outputs.
 * The second voxelisation's chain is issued on a side stream the library owns (one per caller stream, forked from and joined to
 * `stream` with events inside the call): on return everything is ordered on `stream` as usual.  Like every call that forks, it
 * must not be issued while `stream` is being captured into a HIP graph.  (eprecon_spvcnn_geometry_async does the same.)
 */
typedef struct eprecon_gru_finish_desc {
    int64_t n; int64_t m1; int64_t m2;
    const int32_t *inverse1; const int32_t *inverse2;      /* int32[n]: point -> voxel */
    const int32_t *uniq1; const int32_t *uniq2;            /* int32[m][4] */
    const void *table1; const void *table2; uint32_t table_capacity;
    const float *scaled1; const float *scaled2;            /* f32[n][4] points in voxel units (scaled2: literal == 0 only) */
    int literal;
    int32_t *offsets1; int32_t *order1; int32_t *offsets2; int32_t *order2;
    int32_t *nbr1; int32_t *nbr2;
    int32_t *idx8_1; float *weight8_1; int32_t *idx8_2; float *weight8_2;
    int32_t *perm1; int32_t *rank1; int32_t *perm2; int32_t *rank2;   /* literal != 0 only */
    void *workspace; size_t workspace_bytes;
} eprecon_gru_finish_desc;
size_t eprecon_gru_stage_finish_workspace_bytes(int64_t n, int64_t m1, int64_t m2);
int eprecon_gru_stage_finish_async(const eprecon_gru_finish_desc *desc, void *stream);

/*
 * The BODY of one SPVCNN pass as ONE stream-ordered call (models/modules.py:148-175: stem, two k2s2 stages with residual
 * blocks :46-72, two transposed stages with skip concatenation, three scatter-means and three trilinear devoxelisations
 * ops/torchsparse_utils.py:40-105, two point MLPs models/modules.py:125-136; every BatchNorm in train mode, main.py:357).
 * Replaces ~115 calls issued one by one from the host: 27 x eprecon_conv_desc_async, eprecon_batchnorm_finalize_affine_async,
 * eprecon_batchnorm_apply_partials[_res]_async, eprecon_segment_mean_async, eprecon_devoxelize_async — the same entry points,
 * descriptors and order, issued from inside the library (bit-identical results).  The geometry comes from
 * eprecon_spvcnn_geometry_async.  conv[] / bn[] slots, in launch order:
 *    0 stem | 1 stage1 down, 2-4 res (conv, conv, 1x1 skip), 5-6 res | 7 stage2 down, 8-10 res, 11-12 res | 13 point MLP 0 |
 *   14 up1 transposed, 15-17 res, 18-19 res | 20 up2 transposed, 21-23 res, 24-25 res | 26 point MLP 1
 * weight f32[kvol][cin][cout] (kvol 27: x-fastest offsets, 8: z-fastest, 1: a [cin][cout] matrix); packed_weight (kvol 27) and
 * packed_weight16 (kvol 27 or 1, cout <= 64) are the operand-order copies of eprecon_conv_pack_weight[16]_async.
 * cs[5]: the channel plan (32, 64, 128, 96, 96) x cr.  feat f32[n, cin] point features, out f32[n, cs[4]].
 * workspace: eprecon_spvcnn_forward_workspace_bytes(desc) bytes, 256-byte aligned (every intermediate of the pass).
 */
#define EPRECON_SPVCNN_CONVS 27
typedef struct eprecon_spvcnn_conv {
    const float *weight; const float *packed_weight; const float *packed_weight16;
    int kvol; int cin; int cout;
} eprecon_spvcnn_conv;
typedef struct eprecon_spvcnn_bn {
    const float *gamma; const float *beta; float eps;
} eprecon_spvcnn_bn;
typedef struct eprecon_spvcnn_forward_desc {
    int64_t n, n1, n2, n4;
    int cin; int cs[5];
    const float *feat; int ld_feat;
    const int32_t *offsets1, *order1, *offsets4, *order4;
    const int32_t *k1, *k2, *k4, *down12, *up21, *down24, *up42;
    const int32_t *idx8_1; const float *weight8_1; const int32_t *idx8_4; const float *weight8_4;
    eprecon_spvcnn_conv conv[EPRECON_SPVCNN_CONVS];
    eprecon_spvcnn_bn bn[EPRECON_SPVCNN_CONVS];
    float *out; int ld_out;
    void *workspace; size_t workspace_bytes;
} eprecon_spvcnn_forward_desc;
size_t eprecon_spvcnn_forward_workspace_bytes(const eprecon_spvcnn_forward_desc *desc);
int eprecon_spvcnn_forward_async(const eprecon_spvcnn_forward_desc *desc, void *stream);

/*
 * The geometry of one SPVCNN pass after its host read (the sizes n1, n2, n4 of the voxel sets at tensor strides 1, 2, 4, numbered
 * by three queued eprecon_unique_coords(_dn)_async calls), in one call (csrc/spvcnn_geometry.hip): CSR point lists of strides 1
 * and 4 (offsets int32[m+1], order int32[n]; idx4 int32[n] = the stride-4 voxel of every point), the k2s2 maps down12 int32[8][n2],
 * down24 int32[8][n4] and their transposes up21 int32[8][n1], up42 int32[8][n2], the 3x3x3 kernel maps k1 / k2 / k4
 * int32[27][n1 / n2 / n4], trilinear corner tables of strides 1 and 4 (int32[n][8], f32[n][8]).  parent2 int32[n1] / parent4
 * int32[n2]: the inverse index of the stride-2 / stride-4 numbering.  Replaces the same sequence of single calls: bit-identical.
 */
typedef struct eprecon_spvcnn_geometry_desc {
    int64_t n; int64_t n1; int64_t n2; int64_t n4;
    const float *scaled; const int32_t *vox; const int32_t *inverse1;     /* points: f32[n][4], int32[n][4], int32[n] */
    const int32_t *coords1; const int32_t *coords2; const int32_t *coords4;
    const int32_t *parent2; const int32_t *parent4;
    const void *table1; const void *table2; const void *table4;
    uint32_t capacity1; uint32_t capacity2; uint32_t capacity4;
    int32_t *offsets1; int32_t *order1; int32_t *idx4; int32_t *offsets4; int32_t *order4;
    int32_t *down12; int32_t *up21; int32_t *down24; int32_t *up42;
    int32_t *k1; int32_t *k2; int32_t *k4;
    int32_t *idx8_1; float *weight8_1; int32_t *idx8_4; float *weight8_4;
    void *workspace; size_t workspace_bytes;
} eprecon_spvcnn_geometry_desc;
size_t eprecon_spvcnn_geometry_workspace_bytes(int64_t n, int64_t n1, int64_t n4);
int eprecon_spvcnn_geometry_async(const eprecon_spvcnn_geometry_desc *desc, void *stream);

/* x2 bilinear upsampling of channels-last maps, in f32[n,h,w,c] -> out f32[n,2h,2w,c], c % 4 == 0
 * (F.interpolate(scale_factor=2, mode="bilinear") in feat_fusion_pre,
 * models/occupancy_initialization.py:46) */
int eprecon_upsample2x_nhwc_async(const float *in, float *out, int n, int h, int w, int channels,
                                  void *stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the sparse operators  (training, main.py:181-313 loss.backward())
 *
 * Replaces  the autograd of spnn.Conv3d / spconv SubMConv3d, torchsparse.nn.functional.spdevoxelize and
 *           spvoxelize (ops/torchsparse_utils.py:35,63,100), which the reference gets from the two libraries.
 *
 * For y[i] = bias + sum_k x[nbr[k][i]] @ W[k]:
 *   dW[k]  = sum_i x[nbr[k][i]]^T dy[i]                eprecon_sparse_conv_wgrad_async (fp32 MFMA, deterministic:
 *                                                       row chunks reduced in chunk order through `workspace`)
 *   dx[j]  = sum_k dy[inv[k][j]] @ W[k]^T              eprecon_sparse_conv_async on the inverted map
 *   inv[k][j] = i  <=>  nbr[k][i] = j                  eprecon_invert_map_async (a kernel map is injective per offset)
 *   dbias  = column sums of dy                          (host: one reduction)
 * devoxelize:  d voxel_feat[idx8[p][c]] += weight8[p][c] * d out[p]   (hardware float atomics; dvoxel_feat is zeroed)
 * segment mean (voxelize): d point_feat[p] = d mean[idx[p]] * scale[idx[p]], scale = 1 / count
 * ------------------------------------------------------------------------------------------ */
size_t eprecon_sparse_conv_wgrad_workspace_bytes(int kvol, int64_t n_out, int cin, int cout);
int eprecon_sparse_conv_wgrad_async(const float *x, int ld_x, const float *dy, int ld_dy, const int32_t *nbr, int kvol,
                                    int64_t n_out, int cin, int cout, float *dweight, void *workspace,
                                    size_t workspace_bytes, void *stream);
int eprecon_invert_map_async(const int32_t *nbr, int kvol, int64_t n_out, int64_t n_in, int32_t *inv, void *stream);
int eprecon_devoxelize_backward_async(const float *dout, int ld_out, const int32_t *idx8, const float *weight8, int64_t n,
                                      int channels, int64_t n_voxels, float *dvoxel_feat, int ld_feat, void *stream);
/* the same without float atomics (run-to-run bit-identical): offsets int32[n_voxels + 1] / order int32[<= 8 n] = the CSR lists
 * of eprecon_segment_lists_async over the flattened idx8 (entry e = 8 p + corner; entries of missing corners are skipped);
 * dvoxel_feat[v] = sum over the voxel's entries in list order of weight8[e] * dout[e / 8].  The lists depend on the corner
 * table only: build once, reuse for every layer that devoxelises with it. */
int eprecon_devoxelize_backward_csr_async(const float *dout, int ld_out, const float *weight8, const int32_t *offsets,
                                          const int32_t *order, int64_t n_voxels, int channels, float *dvoxel_feat, int ld_feat,
                                          void *stream);
int eprecon_gather_rows_scaled_async(const float *src, int ld_src, const int32_t *idx, const float *scale, int64_t n,
                                     int channels, float *dst, int ld_dst, void *stream);
/* back-projection: d feats[view][b][y][x][c] (channels-last, zeroed here) from d out f32[n_valid, ld_dout] (and, mode
 * VARIANCE, the optional d mean f32[n_valid, C]) at the VALID voxels `coords_valid` the forward returned
 * (ops/back_project.py:47-61 / models/occupancy_initialization.py:113-128 under autograd: grid_sample's backward,
 * the masked mean / variance).  Hardware float atomics. */
int eprecon_back_project_backward_async(const int32_t *coords_valid, int64_t n_valid, const float *origin, int batch,
                                        float voxel_size, const float *feats_nhwc, const float *krcam, int n_views,
                                        int channels, int height, int width, int mode, const float *dout, int ld_dout,
                                        const float *dmean, float *dfeats_nhwc, void *stream);
/* the same, run-to-run bit-identical: contributions are accumulated as 64-bit fixed point (2^-40 resolution, |sum| < 8.4e6) with
 * integer atomics — order-independent — in `workspace` (eprecon_back_project_backward_workspace_bytes) and converted at the end.
 * A single contribution (tap weight x gradient) that the word cannot hold — NaN, Inf, or finite with magnitude above 8.0e6 — is not
 * added: the map element it touches comes back NaN, exactly as for a non-finite gradient.  The SUM of in-range contributions to one
 * element is the caller's to keep below 2^23 = 8.4e6 (it wraps beyond). */
size_t eprecon_back_project_backward_workspace_bytes(int batch, int n_views, int channels, int height, int width);
int eprecon_back_project_backward_det_async(const int32_t *coords_valid, int64_t n_valid, const float *origin, int batch,
                                            float voxel_size, const float *feats_nhwc, const float *krcam, int n_views,
                                            int channels, int height, int width, int mode, const float *dout, int ld_dout,
                                            const float *dmean, float *dfeats_nhwc, void *workspace, size_t workspace_bytes,
                                            void *stream);

/* ------------------------------------------------------------------------------------------
 * View preparation  (csrc/prepare_views.hip: what the data loader does to a fragment's frames before the network sees
 * them — datasets/transforms.py ResizeImage + ToTensor, datasets/scannet.py:57-63 — in one launch each)
 *
 * eprecon_prepare_views_async: frames uint8[n_views, height, width, 3] (decoded RGB) -> out f32[n_views, 3, out_h, out_w],
 *   every element the 8-bit bilinear resize of the frame standing between pad_top and pad_bottom black rows (which are
 *   never materialised), as a float.  The arithmetic is two integer passes, horizontal first, each
 *       clamp((2^21 + sum_x pixel[xmin + x] * k[x]) >> 22, 0, 255)   stored as uint8,
 *   over the taps a table names.  table_x int32[out_w][2 + ksize_x] and table_y int32[out_h][2 + ksize_y] (DEVICE memory,
 *   built once per (in, out) pair on the host) hold per output index: xmin, n (<= ksize), then ksize coefficients (22
 *   fractional bits, the unused ones 0); xmin and xmin + n must not decrease along a table.  table_y indexes the padded
 *   rows 0 .. pad_top + height + pad_bottom.
 *   A workgroup owns EPRECON_VIEWS_TILE_W x EPRECON_VIEWS_TILE_H output pixels of one view and keeps the horizontally
 *   resampled source rows of its vertical window in LDS: lds_rows = the largest such window over the row tiles of table_y
 *   (rows ymin of the tile's first output row .. ymin + n of its last), computed by the caller from the table it built.
 *   A tap the tables name outside the frame, or outside the LDS window, is skipped (never read): wrong tables give wrong
 *   values, not wild accesses.
 *   EPRECON_ERR_ARG: a NULL pointer, a size <= 0, a negative padding, ksize outside 1..EPRECON_VIEWS_MAX_KSIZE;
 *   EPRECON_ERR_UNSUPPORTED: an LDS window beyond what a workgroup may ask for, more than 2^31 - 1 source bytes or outputs.
 *
 * eprecon_depth_to_metres_async: depth_mm uint16[n] -> out f32[n] = (float)d / 1000.0f (IEEE division), 0 where that
 *   exceeds max_depth.
 * ------------------------------------------------------------------------------------------ */
#define EPRECON_VIEWS_TILE_W 64
#define EPRECON_VIEWS_TILE_H 16
#define EPRECON_VIEWS_MAX_KSIZE 9      /* scale <= 4 per axis: 2 * ceil(4) + 1 */
int eprecon_prepare_views_async(const uint8_t *frames, int n_views, int height, int width, int pad_top, int pad_bottom,
                                const int32_t *table_x, int ksize_x, const int32_t *table_y, int ksize_y, int lds_rows,
                                int out_h, int out_w, float *out, void *stream);
int eprecon_depth_to_metres_async(const uint16_t *depth_mm, int64_t n, float max_depth, float *out, void *stream);

/* ------------------------------------------------------------------------------------------
 * Optimiser step  (csrc/optim.hip: main.py:308-310, torch.nn.utils.clip_grad_norm_(parameters, 1.0) and
 * torch.optim.Adam.step() over every trainable parameter, in two or three launches)
 *
 * A SEGMENT is one parameter's contiguous fp32 storage with its gradient and Adam moments.  The host cuts the segments
 * into CHUNKS of one segment each (start and count in floats, start a multiple of the chunk length) and uploads both
 * tables when a pointer or the membership changes; one workgroup works on one chunk.  flags: the float4 form is taken where
 * the addresses it would use are 16-byte aligned (ALL: param, grad, exp_avg and exp_avg_sq at `start`; GRAD: grad alone,
 * for the norm), the scalar form otherwise; a count that is no multiple of 4 ends in scalar elements.
 *
 * eprecon_grad_sqsum_async: partials f64[nchunks], partials[c] = sum of the squares of chunk c's gradient, accumulated in
 *   double (every square exact) and reduced in a fixed order: no atomics, the same bits on every run.
 * eprecon_grad_norm_finish_async: one workgroup sums the partials in a fixed order -> norm_coef f32[2] = {norm,
 *   coef = min(1, max_norm / (norm + 1e-6))}, float arithmetic as clip_grad_norm_ has it; a NaN norm gives a NaN coef.
 * eprecon_adam_update_async: for every element, with the segment's seg_scalars f32[nsegments][2] = {lr / bias_correction1,
 *   sqrt(bias_correction2)} (the host forms them in double from the parameter's own step count):
 *       g = coef * grad (+ weight_decay * p);  m += lerp_weight * (g - m);  v = beta2 * v + one_minus_beta2 * g * g;
 *       p += -(lr / bias1) * (m / (sqrt(v) / sqrt(bias2) + eps))
 *   — torch's non-amsgrad Adam.  coef: 1 when partials and norm_coef are NULL (no clipping); norm_coef[1] as the finish
 *   launch left it when partials is NULL; with partials given, every workgroup sums them itself (the finish launch's order
 *   and bits; none is needed then) and workgroup 0 stores norm_coef.  The gradients are read, never written: they stay
 *   unclipped.
 * EPRECON_EMPTY: nchunks == 0 (nothing launched).
 * ------------------------------------------------------------------------------------------ */
#define EPRECON_ADAM_ALL_ALIGNED 1
#define EPRECON_ADAM_GRAD_ALIGNED 2
typedef struct eprecon_adam_segment {
    float *param; const float *grad; float *exp_avg; float *exp_avg_sq;
} eprecon_adam_segment;
typedef struct eprecon_adam_chunk {
    int32_t segment; int32_t start; int32_t count; int32_t flags;
} eprecon_adam_chunk;
int eprecon_grad_sqsum_async(const eprecon_adam_segment *segs_dev, const eprecon_adam_chunk *chunks_dev, int nchunks,
                             double *partials, void *stream);
int eprecon_grad_norm_finish_async(const double *partials, int nchunks, float max_norm, float *norm_coef, void *stream);
int eprecon_adam_update_async(const eprecon_adam_segment *segs_dev, const eprecon_adam_chunk *chunks_dev, int nchunks,
                              const float *seg_scalars, float lerp_weight, float beta2, float one_minus_beta2, float eps,
                              float weight_decay, const double *partials, float max_norm, float *norm_coef, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* EPRECON_HIP_H */
