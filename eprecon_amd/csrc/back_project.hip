// Multi-view back-projection for gfx950 (MI355X): image-feature pyramid -> voxel list.
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

#include "back_project_common.hpp"

namespace {
using namespace ep;

// Two gather kernels are in the build: bp_gather_mlp_kernel (per-pair taps in LDS, cheap projection, buffer loads: 122 us on the
// dense 96^3 level, C = 24, 120x160 maps) and bp_gather_kernel (taps recomputed: 134 us; takes C % 4 != 0).  2 / 3 / 4 views of
// loads in flight per lane measured 126 / 129 / 138 us: the L1 access rate bounds the kernel (23 accesses per wave load), not
// latency.  The other variants tried and removed, with their figures: DESIGN.md 3a and the git history of this file.

struct BpParams {
    const int32_t *coords;
    int n;
    const float *origin;
    int batch;
    float voxel_size;
    const float *feats_nhwc;  // [V*B][H*W][C]
    const float *krcam;       // [V*B][16]
    int V, C, H, W;
    int Cs;  // pixel stride of the channels-last maps in floats (>= C)
    int min_view;
    float *out_feats;
    float *out_mean;
    int32_t *out_coords;
    float *count;
    float *out_grid;
    uint8_t *out_mask;
    int32_t *n_valid_dev;  // [1 + B]
    int32_t *block_offsets;  // exclusive scan of the tile totals (bp_scan_kernel), or the raw totals when `fold` is set
    int fold;                // 1: no scan launch ran; every gather workgroup sums the totals in front of its tile (tile_base)
    int ntile;               // tiles of the gather (= its grid)
    const int32_t *blk_batch;  // [nblk_count][batch] per-batch valid counts of the count workgroups (batch > 1), else null
    int nblk_count;
    int xcd_slabs;  // 1 (default): every XCD walks one contiguous range of tiles (ep::xcd_remap); 0: tile = hardware block id
    int32_t *rank;  // [n + 1] or null: list entry -> output row or -1, then one word 0 (eprecon_back_project_rank_out)
};

// Cheap projection with bit-exact visibility.  The fma chains for (px, py, pz) are the contract's;
// the three IEEE divisions per axis are replaced by one v_rcp_f32 + Newton step, and the exact
// sequence is re-evaluated only when the cheap normalised coordinate lands within 1e-4 of the
// frustum boundary |g| = 1 (the cheap value is within 1e-6 of the exact one, so outside that band
// both agree).  u, v are the pixel coordinates used for sampling (<= 1e-5 px from the reference's
// grid -> pixel round trip), clamped into the image.
struct ProjFast {
    float u, v, pz;
    bool vis;
};

__device__ __forceinline__ ProjFast project_fast(const float *P, float X, float Y, float Z, float wm1, float hm1,
                                                 float kx, float ky)
{
    const float px = __fmaf_rn(P[3], 1.0f, __fmaf_rn(P[2], Z, __fmaf_rn(P[1], Y, __fmul_rn(P[0], X))));
    const float py = __fmaf_rn(P[7], 1.0f, __fmaf_rn(P[6], Z, __fmaf_rn(P[5], Y, __fmul_rn(P[4], X))));
    const float pz = __fmaf_rn(P[11], 1.0f, __fmaf_rn(P[10], Z, __fmaf_rn(P[9], Y, __fmul_rn(P[8], X))));
    float r = __builtin_amdgcn_rcpf(pz);
    r = r * fmaf(-pz, r, 2.0f);
    const float u = px * r, v = py * r;
    const float gx = fmaf(u, kx, -1.0f), gy = fmaf(v, ky, -1.0f);
    ProjFast o;
    o.pz = pz;
    const bool near_edge = fabsf(fabsf(gx) - 1.0f) < 1e-4f || fabsf(fabsf(gy) - 1.0f) < 1e-4f;
    if (near_edge) {
        const float ue = __fdiv_rn(px, pz), ve = __fdiv_rn(py, pz);
        const float gxe = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, ue), wm1), 1.0f);
        const float gye = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, ve), hm1), 1.0f);
        o.vis = (fabsf(gxe) <= 1.0f) && (fabsf(gye) <= 1.0f) && (pz > 0.0f);
    } else {
        o.vis = (fabsf(gx) <= 1.0f) && (fabsf(gy) <= 1.0f) && (pz > 0.0f);
    }
    o.u = fminf(fmaxf(u, 0.0f), wm1);
    o.v = fminf(fmaxf(v, 0.0f), hm1);
    return o;
}

// ---------------------------------------------------------------------------------------------
// K1: visible-view count for every voxel, valid totals per block and per batch element
// ---------------------------------------------------------------------------------------------
// One thread per voxel, 256 per workgroup.  The valid totals are produced per TILE of VOX consecutive
// voxels (VOX = 256, 64 or 16: the tile the gather kernel hands to one workgroup).
template <int VOX>
__device__ __forceinline__ void count_body(char *smem, const BpParams &p, int32_t *tile_sums, int32_t *blk_batch, int bid)
{
    constexpr int BLOCK = 256;
    float *sP = reinterpret_cast<float *>(smem);
    int *sBatch = reinterpret_cast<int *>(sP + p.V * p.batch * 12);
    int *sWave = sBatch + p.batch;
    const int tid = threadIdx.x;
    stage_matrices(sP, p.krcam, p.V * p.batch, tid, BLOCK);
    for (int b = tid; b < p.batch; b += BLOCK) sBatch[b] = 0;
    __syncthreads();

    const int i = bid * BLOCK + tid;
    bool valid = false;
    int vbatch = 0;
    if (i < p.n) {
        const int4 c = reinterpret_cast<const int4 *>(p.coords)[i];
        int cnt = 0;
        const bool in_range = c.x >= 0 && c.x < p.batch;
        if (in_range) {
            float X, Y, Z;
            voxel_centre(c, p.origin, p.voxel_size, X, Y, Z);
            const float wm1 = (float)(p.W - 1), hm1 = (float)(p.H - 1);
            const float kx = 2.0f / wm1, ky = 2.0f / hm1;
            for (int v = 0; v < p.V; ++v)
                cnt += project_fast(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1, kx, ky).vis ? 1 : 0;
        }
        p.count[i] = (float)cnt;
        valid = in_range && cnt >= p.min_view;
        vbatch = c.x;
    }
    const unsigned long long m = __ballot(valid);
    const int lane = tid & (kWave - 1);
    {   // per-batch valid counts: lists are grouped by batch, so a wave almost always holds one batch
        // element -> one LDS atomic per wave instead of one per voxel
        const int b0 = __shfl(vbatch, m ? (__ffsll((long long)m) - 1) : 0);
        const bool uniform = __ballot(valid && vbatch != b0) == 0ull;
        if (uniform) {
            if (m && lane == (__ffsll((long long)m) - 1)) atomicAdd(&sBatch[b0], __popcll(m));
        } else if (valid) {
            atomicAdd(&sBatch[vbatch], 1);
        }
    }
    if constexpr (VOX >= kWave) {
        // tile = VOX / 64 whole waves: per-wave popcounts through LDS
        if (lane == 0) sWave[tid / kWave] = __popcll(m);
        __syncthreads();
        constexpr int WPT = VOX / kWave;  // waves per tile
        if (tid < BLOCK / VOX) {
            int t = 0;
            for (int w = 0; w < WPT; ++w) t += sWave[tid * WPT + w];
            const int tile = bid * (BLOCK / VOX) + tid;
            if ((long long)tile * VOX < p.n) tile_sums[tile] = t;
        }
    } else {
        if ((lane % VOX) == 0 && i < p.n) tile_sums[i / VOX] = __popcll((m >> lane) & ((1ull << VOX) - 1ull));
        __syncthreads();
    }
    // per-batch totals: per-workgroup rows reduced by bp_scan_kernel (3,456 same-address global atomics
    // cost ~40 us on the dense 96^3 level: device-scope atomics serialise at the memory side)
    if (blk_batch) {
        __syncthreads();
        for (int b = tid; b < p.batch; b += BLOCK) blk_batch[(size_t)bid * p.batch + b] = sBatch[b];
    }
}

template <int VOX>
__global__ __launch_bounds__(256) void bp_count_kernel(BpParams p, int32_t *tile_sums, int32_t *blk_batch)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    count_body<VOX>(smem, p, tile_sums, blk_batch, (int)blockIdx.x);
}

// exclusive scan of the block totals, one workgroup; also publishes n_valid
__global__ __launch_bounds__(1024) void bp_scan_kernel(int32_t *block_sums, int nblk,
                                                       int32_t *n_valid_dev, const int32_t *blk_batch = nullptr,
                                                       int nblk_count = 0, int batch = 0)
{
    __shared__ int sWave[1024 / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    int carry = 0;
    for (int base = 0; base < nblk; base += 1024) {
        const int i = base + tid;
        const int v = i < nblk ? block_sums[i] : 0;
        int x = v;
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == kWave - 1) sWave[wid] = x;
        __syncthreads();
        int woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 1024 / kWave; ++w) {
            const int c = sWave[w];
            woff += (w < wid) ? c : 0;
            tot += c;
        }
        if (i < nblk) block_sums[i] = carry + woff + x - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0) n_valid_dev[0] = carry;
    // per-batch valid totals from the count kernel's per-workgroup rows
    if (batch == 1) {
        if (tid == 0) n_valid_dev[1] = carry;
    } else if (blk_batch) {
        for (int b = 0; b < batch; ++b) {
            int x = 0;
            for (int i = tid; i < nblk_count; i += 1024) x += blk_batch[(size_t)i * batch + b];
#pragma unroll
            for (int d = kWave / 2; d > 0; d >>= 1) x += __shfl_xor(x, d);
            __syncthreads();
            if (lane == 0) sWave[wid] = x;
            __syncthreads();
            if (tid == 0) {
                int t = 0;
                for (int w = 0; w < 1024 / kWave; ++w) t += sWave[w];
                n_valid_dev[1 + b] = t;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The scan folded into the gather (BpParams::fold): the count launch has finished, so its tile totals are plain
// read-only data, and a gather workgroup gets the output row of its tile by summing the totals in front of it
// (the pattern of kernel_map.hip's scan_apply<true>) -- at 3,456 tiles at most 13.5 four-byte L2 loads per
// thread -- instead of the whole chip waiting for one scanning workgroup between two launches.  No look-back,
// no ticket, no spin: nothing here waits for another workgroup.
//   tile_base_partials   before phase 1: per-wave partial sums -> sFold (2 x BLOCK/64 ints)
//   tile_base_finish     after the next barrier of the caller (block_exclusive_rank's): the sums; the workgroup
//                        of the last tile publishes n_valid_dev[0 .. B] (what bp_scan_kernel published), and
//                        has to do so before the caller's `if (nloc == 0) return;`
// `all` (block-uniform): the sum runs over every tile, which also gives n_valid -- wanted by that last workgroup
// and by every workgroup when out_grid / out_mask are written (n_valid is their view stride).
// ---------------------------------------------------------------------------------------------
struct TileBase {
    int base, n_valid;
};

__device__ __forceinline__ bool tile_base_all(const BpParams &p, int lb)
{
    return p.out_grid != nullptr || p.out_mask != nullptr || lb == p.ntile - 1;
}

__device__ __forceinline__ void tile_base_partials(const BpParams &p, int lb, int *sFold)
{
    constexpr int BLOCK = 256;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int end = tile_base_all(p, lb) ? p.ntile : lb;
    int acc = 0, tot = 0;
#pragma unroll 4
    for (int t = tid; t < end; t += BLOCK) {
        const int x = p.block_offsets[t];
        tot += x;
        acc += t < lb ? x : 0;
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) {
        acc += __shfl_xor(acc, d);
        tot += __shfl_xor(tot, d);
    }
    if (lane == 0) {
        sFold[wid] = acc;
        sFold[BLOCK / kWave + wid] = tot;
    }
}

__device__ __forceinline__ TileBase tile_base_finish(const BpParams &p, int lb, int *sFold)
{
    constexpr int BLOCK = 256, NW = BLOCK / kWave;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    TileBase r = {0, 0};
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        r.base += sFold[w];
        r.n_valid += sFold[NW + w];
    }
    if (lb == p.ntile - 1) {   // block-uniform
        if (tid == 0) {
            p.n_valid_dev[0] = r.n_valid;
            if (p.batch == 1) p.n_valid_dev[1] = r.n_valid;
        }
        if (p.batch > 1 && p.blk_batch) {
            for (int b = 0; b < p.batch; ++b) {
                int x = 0;
                for (int i = tid; i < p.nblk_count; i += BLOCK) x += p.blk_batch[(size_t)i * p.batch + b];
#pragma unroll
                for (int d = kWave / 2; d > 0; d >>= 1) x += __shfl_xor(x, d);
                __syncthreads();   // (sFold: the sums above, then the row before, have been read)
                if (lane == 0) sFold[wid] = x;
                __syncthreads();
                if (tid == 0) {
                    int t = 0;
                    for (int w = 0; w < NW; ++w) t += sFold[w];
                    p.n_valid_dev[1 + b] = t;
                }
            }
        }
    }
    return r;
}

// The rank volume of a list that IS the x-major raster of a dense grid (list entry e = cell e; back_project.mark_dense): the
// gather has just given every entry of its tile an output row or none, which is what eprecon_grid_rank_async would recompute
// from the compacted coordinates with two clears and a scatter.  Every entry of every tile is written (tiles without a valid
// voxel too: before their early return); the workgroup of the last tile adds the trailing "not on the grid" word, 0 here.
__device__ __forceinline__ void gather_rank_store(const BpParams &p, int lb, int e, bool mine, bool valid, int orow)
{
    if (mine) p.rank[e] = valid ? orow : -1;
    if (lb == (int)gridDim.x - 1 && threadIdx.x == 0) p.rank[p.n] = 0;
}

// ---------------------------------------------------------------------------------------------
// K2 + K3 (+K4): compaction and bilinear gather
// ---------------------------------------------------------------------------------------------

// QT > 0: channel groups per voxel known at compile time (fast div/mod); QT == 0: runtime
template <int VOX, int MODE, int VEC, int QT>
__global__ __launch_bounds__(256) void bp_gather_kernel(BpParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BLOCK = 256;
    // LDS carve (every offset a multiple of 16 bytes)
    float2 *sPix = reinterpret_cast<float2 *>(smem);                     // [VOX][V] pixel coords
    float *sP = reinterpret_cast<float *>(sPix + VOX * p.V);             // [V*B][12]
    const int nP = (p.V * p.batch * 12 + 3) & ~3;
    uint32_t *sVis = reinterpret_cast<uint32_t *>(sP + nP);              // [VOX] view bitmask
    float *sDen = reinterpret_cast<float *>(sVis + VOX);                 // [VOX] divisor
    int *sBatch = reinterpret_cast<int *>(sDen + VOX);                   // [VOX] batch index
    int *sSlot = sBatch + VOX;                                           // [VOX] rank -> thread
    int *sOut = sSlot + VOX;                                             // [VOX] thread -> output row
    int *sWave = sOut + VOX;                                             // [BLOCK/64]
    int *sFold = sWave + BLOCK / kWave;                                  // [2 * BLOCK/64] (tile_base)

    const int tid = threadIdx.x;
    const int lb = p.xcd_slabs ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    stage_matrices(sP, p.krcam, p.V * p.batch, tid, BLOCK);
    if (p.fold) tile_base_partials(p, lb, sFold);
    __syncthreads();

    const int e = lb * VOX + tid;
    const int i = e;
    const float wm1 = (float)(p.W - 1), hm1 = (float)(p.H - 1);
    bool valid = false;
    int4 c = make_int4(0, 0, 0, 0);
    float X = 0.f, Y = 0.f, Z = 0.f, zsum = 0.f;
    int cnt = 0;
    uint32_t vis = 0;
    if (tid < VOX && e < p.n) {
        c = reinterpret_cast<const int4 *>(p.coords)[i];
        if (c.x >= 0 && c.x < p.batch) {
            voxel_centre(c, p.origin, p.voxel_size, X, Y, Z);
            for (int v = 0; v < p.V; ++v) {
                const Proj pr = project(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1);
                // grid -> pixel exactly as grid_sample(align_corners=True) un-normalises
                const float ix = __fmul_rn(__fdiv_rn(__fadd_rn(pr.gx, 1.0f), 2.0f), wm1);
                const float iy = __fmul_rn(__fdiv_rn(__fadd_rn(pr.gy, 1.0f), 2.0f), hm1);
                sPix[tid * p.V + v] = make_float2(ix, iy);
                if (pr.vis) {
                    vis |= 1u << v;
                    cnt += 1;
                    zsum += pr.pz;
                }
            }
            valid = cnt >= p.min_view;
        }
    }
    int nloc;
    const int rank = block_exclusive_rank<BLOCK>(valid, sWave, nloc);
    TileBase tb = {0, 0};
    if (p.fold) tb = tile_base_finish(p, lb, sFold);
    const int base = p.fold ? tb.base : p.block_offsets[lb];
    if (p.rank) gather_rank_store(p, lb, e, tid < VOX && e < p.n, valid, base + rank);
    if (nloc == 0) return;
    const int n_valid = p.fold ? tb.n_valid : p.n_valid_dev[0];
    const int cout = (MODE == EPRECON_BP_MEAN_DEPTH) ? p.C + 1 : p.C;
    if (valid) {
        const int o = base + rank;
        sSlot[rank] = tid;
        sOut[tid] = o;
        sVis[tid] = vis;
        const float den = (float)(cnt > 0 ? cnt : 1);
        sDen[tid] = den;
        sBatch[tid] = c.x;
        reinterpret_cast<int4 *>(p.out_coords)[o] = c;
        if (MODE == EPRECON_BP_MEAN_DEPTH) p.out_feats[(size_t)o * cout + p.C] = __fdiv_rn(zsum, den);
        if (p.out_grid || p.out_mask) {
            for (int v = 0; v < p.V; ++v) {
                const Proj pr = project(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1);
                if (p.out_grid)
                    reinterpret_cast<float2 *>(p.out_grid)[(size_t)v * n_valid + o] = make_float2(pr.gx, pr.gy);
                if (p.out_mask) p.out_mask[(size_t)v * n_valid + o] = pr.vis ? 1 : 0;
            }
        }
    }
    __syncthreads();

    const int Q = QT > 0 ? QT : p.C / VEC;
    const size_t map_elems = (size_t)p.H * p.W * p.Cs;
    const bool aligned16 = (MODE != EPRECON_BP_MEAN_DEPTH);
    for (int w = tid; w < nloc * Q; w += BLOCK) {
        const int r = w / Q;
        const int q = w - r * Q;
        const int t = sSlot[r];
        const uint32_t vm = sVis[t];
        const float den = sDen[t];
        const int b = sBatch[t];
        const float *fb = p.feats_nhwc + (size_t)b * map_elems + q * VEC;
        const size_t vstride = (size_t)p.batch * map_elems;
        Chan<VEC> acc = Chan<VEC>::zero();
        for (int v = 0; v < p.V; ++v) {
            if (vm & (1u << v)) {
                const float2 px = sPix[t * p.V + v];
                const Taps tp = make_taps(px.x, px.y, p.W, p.H, p.Cs);
                acc.add(Chan<VEC>::sample(fb + (size_t)v * vstride, tp));
            }
        }
        const int orow = sOut[t];
        float *dst = p.out_feats + (size_t)orow * cout + q * VEC;
        if (MODE == EPRECON_BP_VARIANCE) {
            // models/occupancy_initialization.py:127-128: population variance over visible views
            const Chan<VEC> mean = acc.div(den);
            Chan<VEC> sq = Chan<VEC>::zero();
            for (int v = 0; v < p.V; ++v) {
                if (vm & (1u << v)) {
                    const float2 px = sPix[t * p.V + v];
                    const Taps tp = make_taps(px.x, px.y, p.W, p.H, p.Cs);
                    sq.add_sqdiff(Chan<VEC>::sample(fb + (size_t)v * vstride, tp), mean);
                }
            }
            sq.div(den).store(dst, true);
            if (p.out_mean) mean.store(p.out_mean + (size_t)orow * p.C + q * VEC, true);
        } else {
            acc.div(den).store(dst, aligned16);
        }
    }
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// K2 + K3 (+K4), default for C % 4 == 0: direct gather with per-pair taps in LDS and U views of loads
// in flight per lane (U = 1 by default: measured, the kernel is bound by the L1 access rate and extra
// loads in flight only cost registers).
//   phase 1a  one thread per (voxel, view): cheap bit-exact projection; byte offset of tap (x0, y0)
//             (base pixel clamped to [0, W-2] x [0, H-2], so all four taps are in the image and the
//             border weight is exactly 0 where the reference pads with zeros) and the two fractional
//             weights -> LDS, 12 bytes per pair, computed once instead of once per channel group;
//   phase 1b  one thread per voxel: visible count, validity, stable in-tile compaction, output row;
//   phase 2   one thread per (valid voxel, 4 channels): the visible views are walked U at a time:
//             4 U buffer loads (32-bit offsets; the other three taps are scalar offsets of the
//             first) are issued before the first fma; slots past the last visible view point out of
//             the buffer range, which costs no memory traffic.  Views accumulate in ascending order.
// ---------------------------------------------------------------------------------------------
// Tiles up to which the scan is folded into the gather (tile_base).  >= 3,456 (dense 96^3 at 256 voxels); the sweep of list
// lengths behind the figure is profiles/r12/fold_cap.txt.  tests/test_back_project_launches_gpu.py restates the
// figure (DEFAULT_CAP) and reads the tile totals at offset 0 of the workspace: change them together.
constexpr int kFoldCapDefault = 6144;

constexpr int kOobOffset = (int)0x80000000u;  // >= num_records (maps are limited to < 2 GiB here)

template <int U, class F>
__device__ __forceinline__ void visit_visible_samples(__amdgpu_buffer_rsrc_t rsrc, const int *sOffRow,
                                                      const float2 *sWxyRow, uint32_t vm, int qbyte, int s10,
                                                      int s01, int s11, F &&f)
{
    uint32_t m = vm;
    while (m) {
        int off[U];
        float2 wxy[U];
        bool on[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            on[u] = m != 0;
            const int v = on[u] ? __builtin_ctz(m) : 0;
            m &= m - 1;
            wxy[u] = sWxyRow[v];
            off[u] = on[u] ? sOffRow[v] + qbyte : kOobOffset;
        }
        u32x4 a[U], b[U], c[U], d[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            a[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[u], 0, 0);
            b[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[u], s10, 0);
            c[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[u], s01, 0);
            d[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off[u], s11, 0);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float wx1 = wxy[u].x, wy1 = wxy[u].y;
            const float wx0 = 1.0f - wx1, wy0 = 1.0f - wy1;  // exact: wx1 is a multiple of ulp(ix) in [0, 1]
            const float w00 = wx0 * wy0, w10 = wx1 * wy0, w01 = wx0 * wy1, w11 = wx1 * wy1;
            float4 r;
#define EP_TAP(k) fmaf(__uint_as_float(d[u].k), w11, fmaf(__uint_as_float(c[u].k), w01, fmaf(__uint_as_float(b[u].k), w10, __uint_as_float(a[u].k) * w00)))
            r.x = EP_TAP(x); r.y = EP_TAP(y); r.z = EP_TAP(z); r.w = EP_TAP(w);
#undef EP_TAP
            if (on[u]) f(r);
        }
    }
}

template <int VOX, int MODE, int QT, int U>
__global__ __launch_bounds__(256) void bp_gather_mlp_kernel(BpParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int BLOCK = 256;
    constexpr int VPT = BLOCK / VOX;  // threads per voxel in phase 1a (1, 4 or 16)
    float2 *sWxy = reinterpret_cast<float2 *>(smem);                      // [VOX*V] fractional weights
    int *sOff = reinterpret_cast<int *>(sWxy + VOX * p.V);                // [VOX*V] byte offset of tap (x0, y0)
    float *sP = reinterpret_cast<float *>(sOff + VOX * p.V);              // [V*B][12]
    const int nP = (p.V * p.batch * 12 + 3) & ~3;
    uint32_t *sVis = reinterpret_cast<uint32_t *>(sP + nP);               // [VOX] view bitmask
    int *sSlot = reinterpret_cast<int *>(sVis + VOX);                     // [VOX] rank -> voxel
    int *sOut = sSlot + VOX;                                              // [VOX] voxel -> output row
    int *sWave = sOut + VOX;                                              // [BLOCK/64]
    int *sFold = sWave + BLOCK / kWave;                                   // [2 * BLOCK/64] (tile_base)

    const int tid = threadIdx.x;
    const int lb = p.xcd_slabs ? xcd_remap(blockIdx.x, gridDim.x) : (int)blockIdx.x;
    stage_matrices(sP, p.krcam, p.V * p.batch, tid, BLOCK);
    if (VPT > 1 && tid < VOX) sVis[tid] = 0;
    if (p.fold) tile_base_partials(p, lb, sFold);
    __syncthreads();

    const float wm1 = (float)(p.W - 1), hm1 = (float)(p.H - 1);
    const float kx = 2.0f / wm1, ky = 2.0f / hm1;
    const int map_elems = p.H * p.W * p.Cs;
    // ---- phase 1a: thread -> (voxel tid % VOX, views tid / VOX, + VPT, ...) ----
    const int vx = tid % VOX;
    const int e = lb * VOX + vx;
    int4 c = make_int4(-1, 0, 0, 0);
    if (e < p.n) c = reinterpret_cast<const int4 *>(p.coords)[e];
    const bool in_batch = c.x >= 0 && c.x < p.batch;
    uint32_t vis = 0;
    if (in_batch) {
        float X, Y, Z;
        voxel_centre(c, p.origin, p.voxel_size, X, Y, Z);
        for (int v = tid / VOX; v < p.V; v += VPT) {
            const ProjFast q = project_fast(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1, kx, ky);
            if (!q.vis) continue;
            const float x0f = fminf(floorf(q.u), wm1 - 1.0f), y0f = fminf(floorf(q.v), hm1 - 1.0f);
            sWxy[vx * p.V + v] = make_float2(q.u - x0f, q.v - y0f);
            sOff[vx * p.V + v] = ((v * p.batch + c.x) * map_elems + ((int)y0f * p.W + (int)x0f) * p.Cs) * 4;
            vis |= 1u << v;
        }
        if (VPT > 1 && vis) atomicOr(&sVis[vx], vis);
    }
    if (VPT > 1) {
        __syncthreads();
        vis = sVis[vx];
    }
    // ---- phase 1b ----
    const int cnt = __popc(vis);
    const bool valid = tid < VOX && in_batch && cnt >= p.min_view;
    int nloc;
    const int rank = block_exclusive_rank<BLOCK>(valid, sWave, nloc);
    TileBase tb = {0, 0};
    if (p.fold) tb = tile_base_finish(p, lb, sFold);
    const int o = (p.fold ? tb.base : p.block_offsets[lb]) + rank;
    if (p.rank) gather_rank_store(p, lb, e, tid < VOX && e < p.n, valid, o);
    if (nloc == 0) return;
    const int n_valid = p.fold ? tb.n_valid : p.n_valid_dev[0];
    const int cout = (MODE == EPRECON_BP_MEAN_DEPTH) ? p.C + 1 : p.C;
    if (valid) {
        sSlot[rank] = tid;
        sOut[tid] = o;
        if (VPT == 1) sVis[tid] = vis;
        reinterpret_cast<int4 *>(p.out_coords)[o] = c;
        if (MODE == EPRECON_BP_MEAN_DEPTH || p.out_grid || p.out_mask) {
            float X, Y, Z, zsum = 0.0f;
            voxel_centre(c, p.origin, p.voxel_size, X, Y, Z);
            for (int v = 0; v < p.V; ++v) {
                const Proj pr = project(sP + (v * p.batch + c.x) * 12, X, Y, Z, wm1, hm1);
                if (pr.vis) zsum += pr.pz;
                if (p.out_grid)
                    reinterpret_cast<float2 *>(p.out_grid)[(size_t)v * n_valid + o] = make_float2(pr.gx, pr.gy);
                if (p.out_mask) p.out_mask[(size_t)v * n_valid + o] = pr.vis ? 1 : 0;
            }
            if (MODE == EPRECON_BP_MEAN_DEPTH)
                p.out_feats[(size_t)o * cout + p.C] = __fdiv_rn(zsum, (float)(cnt > 0 ? cnt : 1));
        }
    }
    __syncthreads();
    // ---- phase 2 ----
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.feats_nhwc), 0, p.V * p.batch * map_elems * 4, 0x00020000);
    const int Q = QT > 0 ? QT : p.C / 4;
    const int s10 = p.Cs * 4, s01 = p.W * p.Cs * 4, s11 = s01 + s10;
    for (int w = tid; w < nloc * Q; w += BLOCK) {
        const int r = w / Q, q = w - r * Q;
        const int t = sSlot[r];
        const uint32_t vm = sVis[t];
        const float den = (float)max(__popc(vm), 1);
        const int *offRow = sOff + t * p.V;
        const float2 *wxyRow = sWxy + t * p.V;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        visit_visible_samples<U>(rsrc, offRow, wxyRow, vm, q * 16, s10, s01, s11, [&](const float4 &f) {
            acc.x += f.x; acc.y += f.y; acc.z += f.z; acc.w += f.w;
        });
        const int orow = sOut[t];
        float *dst = p.out_feats + (size_t)orow * cout + q * 4;
        const float4 mean = make_float4(__fdiv_rn(acc.x, den), __fdiv_rn(acc.y, den), __fdiv_rn(acc.z, den),
                                        __fdiv_rn(acc.w, den));
        if (MODE == EPRECON_BP_VARIANCE) {
            // models/occupancy_initialization.py:127-128: population variance over visible views
            float4 sq = make_float4(0.f, 0.f, 0.f, 0.f);
            visit_visible_samples<U>(rsrc, offRow, wxyRow, vm, q * 16, s10, s01, s11, [&](const float4 &f) {
                const float dx = f.x - mean.x, dy = f.y - mean.y, dz = f.z - mean.z, dw = f.w - mean.w;
                sq.x = fmaf(dx, dx, sq.x); sq.y = fmaf(dy, dy, sq.y); sq.z = fmaf(dz, dz, sq.z); sq.w = fmaf(dw, dw, sq.w);
            });
            *reinterpret_cast<float4 *>(dst) = make_float4(__fdiv_rn(sq.x, den), __fdiv_rn(sq.y, den),
                                                           __fdiv_rn(sq.z, den), __fdiv_rn(sq.w, den));
            if (p.out_mean) *reinterpret_cast<float4 *>(p.out_mean + (size_t)orow * p.C + q * 4) = mean;
        } else if (MODE == EPRECON_BP_MEAN_DEPTH) {
            dst[0] = mean.x; dst[1] = mean.y; dst[2] = mean.z; dst[3] = mean.w;  // rows of C + 1 floats
        } else {
            *reinterpret_cast<float4 *>(dst) = mean;
        }
    }
}

// ops/back_project.py:69-75 — per batch element: mu = mean(d[d>0]); sigma = ||d[d>0]-mu||_2 + 1e-5;
// d_hat = (d-mu)/sigma, 0 where d <= 0.  One workgroup per batch element, three sweeps.
__global__ __launch_bounds__(1024) void bp_depth_norm_kernel(float *out_feats, int cout,
                                                             const int32_t *n_valid_dev)
{
    __shared__ float sRed[1024 / kWave];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    int start = 0;
    for (int k = 0; k < b; ++k) start += n_valid_dev[1 + k];
    const int len = n_valid_dev[1 + b];
    float *d = out_feats + (size_t)start * cout + (cout - 1);

    auto block_sum = [&](float x) -> float {
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) x += __shfl_xor(x, s);
        __syncthreads();
        if (lane == 0) sRed[wid] = x;
        __syncthreads();
        float t = 0.f;
#pragma unroll
        for (int w = 0; w < 1024 / kWave; ++w) t += sRed[w];
        return t;
    };
    float s = 0.f, m = 0.f;
    for (int j = tid; j < len; j += 1024) {
        const float x = d[(size_t)j * cout];
        if (x > 0.f) { s += x; m += 1.f; }
    }
    const float tot = block_sum(s), cntp = block_sum(m);
    const float mu = tot / cntp;
    float ss = 0.f;
    for (int j = tid; j < len; j += 1024) {
        const float x = d[(size_t)j * cout];
        if (x > 0.f) ss = fmaf(x - mu, x - mu, ss);
    }
    const float sigma = sqrtf(block_sum(ss)) + 1e-5f;
    for (int j = tid; j < len; j += 1024) {
        const float x = d[(size_t)j * cout];
        d[(size_t)j * cout] = x > 0.f ? (x - mu) / sigma : 0.f;
    }
}

// zero / zero_n (optional): int32 words the first block clears on its way — the valid-voxel counters of the back-projection
// this re-layout is the first launch of (the EPRECON_BP_FOLD=0 chain: one launch less than a memset in front of it)
template <bool VEC4>
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const float *__restrict__ in,
                                                           float *__restrict__ out, int C, int hw, int Cs,
                                                           int32_t *zero = nullptr, int zero_n = 0)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (blockIdx.x == 0 && blockIdx.y == 0 && (int)threadIdx.x < zero_n) zero[threadIdx.x] = 0;
    relayout_body<VEC4>(smem, in, out, C, hw, Cs, (int)blockIdx.y, (int)blockIdx.x * kTrPix);
}

// The first launch of a back-projection on NCHW maps: blocks [0, R) re-lay the maps out (R = maps x 64-pixel tiles), the rest
// count (count_body).  The two halves do not depend on each other; the gather that follows needs both.  The count is
// arithmetic on 16 bytes per voxel and runs under the copy.  Dynamic LDS: the larger of the two bodies'.
template <int VOX, bool VEC4>
__global__ __launch_bounds__(256) void bp_prepare_kernel(BpParams p, int32_t *tile_sums, int32_t *blk_batch,
                                                         const float *__restrict__ in, float *__restrict__ out, int hw,
                                                         int tiles, int R)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bid = blockIdx.x;
    if (bid < R) {   // block-uniform
        const int map = bid / tiles;
        relayout_body<VEC4>(smem, in, out, p.C, hw, p.Cs, map, (bid - map * tiles) * kTrPix);
    } else {
        count_body<VOX>(smem, p, tile_sums, blk_batch, bid - R);
    }
}

// The prepare launches of several back-projections (levels) as ONE grid: the concatenation, level after level, of a level's re-layout
// blocks and its count blocks.  A workgroup finds its level from block-uniform compares of its index against the levels' last
// blocks (kernel arguments), then its half, and runs the body bp_prepare_kernel would have run with the level's own arguments:
// the same tile totals, the same workspace, the same bits.  The levels do not depend on each other and nothing here waits for
// another workgroup.  A channels-last level has no re-layout blocks, a level without a list no count blocks.
constexpr int kMaxLevels = 4;
struct BpLevelDev {
    int end_relayout, end;   // one past the level's last re-layout block / last block in the concatenated grid
    int vox, vec4, hw, tiles;
    const float *in;
    float *out;
    int32_t *tile_sums, *blk_batch;
    BpParams p;
};
struct BpLevelTable {
    BpLevelDev lv[kMaxLevels];   // (slots behind the last level: end = the grid, so that no block selects them)
};

__global__ __launch_bounds__(256) void bp_prepare_levels_kernel(BpLevelTable t)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int bid = blockIdx.x;
    int l = 0, begin = 0;
#pragma unroll
    for (int k = 0; k + 1 < kMaxLevels; ++k) {   // block-uniform
        const int e = t.lv[k].end;
        if (bid >= e) {
            l = k + 1;
            begin = e;
        }
    }
    const BpLevelDev &L = t.lv[l];
    if (bid < L.end_relayout) {
        const int r = bid - begin, map = r / L.tiles, p0 = (r - map * L.tiles) * kTrPix;
        if (L.vec4) relayout_body<true>(smem, L.in, L.out, L.p.C, L.hw, L.p.Cs, map, p0);
        else relayout_body<false>(smem, L.in, L.out, L.p.C, L.hw, L.p.Cs, map, p0);
    } else {
        const int cb = bid - L.end_relayout;
        if (L.vox == 256) count_body<256>(smem, L.p, L.tile_sums, L.blk_batch, cb);
        else if (L.vox == 64) count_body<64>(smem, L.p, L.tile_sums, L.blk_batch, cb);
        else count_body<16>(smem, L.p, L.tile_sums, L.blk_batch, cb);
    }
}

// dynamic LDS of a gather workgroup: 12 (mlp: two weights and an offset) or 8 (pixel coordinates) bytes per (voxel, view), the
// matrices, 3 or 5 words per voxel, sWave and sFold
size_t gather_lds_bytes(bool mlp, int vox, int V, int B)
{
    const size_t nP = ((size_t)V * B * 12 + 3) & ~(size_t)3;
    return (size_t)vox * V * (mlp ? 12 : 8) + nP * 4 + (size_t)vox * (mlp ? 3 : 5) * 4 + (size_t)(256 / kWave) * 4 * 3;
}

// QT, the channel groups of four per voxel: the model's widths at compile time (C = 24: 1/4-res level, 32: fused initialisation
// maps, 40: 1/8-res, 80: 1/16-res), any other at run time; C % 4 != 0 takes the scalar kernel.  mlp: U = 1 (2 / 3 / 4 views of
// loads in flight per lane: slower, see above).
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

// One-shot, per host thread: the NEXT eprecon_back_project_async / eprecon_back_project call of this thread also writes
// rank int32[n + 1] (BpParams::rank).  The call takes the pointer whatever it returns, so it never reaches a later call.
thread_local int32_t *t_rank_out = nullptr;

// The arguments of the forward entry points (host only).  phase: 0, the whole call, or one of its halves for channels-last maps
// (EPRECON_BP_COUNT / EPRECON_BP_GATHER, include/eprecon_hip.h: the count half reads coordinates and matrices only).
struct BpArgs {
    int phase; const int32_t *coords; int64_t n; const float *origin; int batch; float voxel_size;
    const float *feats; int feats_layout; const float *krcam; int n_views, channels, height, width, min_view, mode;
    float *out_feats, *out_mean; int32_t *out_coords; float *count, *out_grid; uint8_t *out_mask; int32_t *n_valid_dev;
    void *workspace; size_t workspace_bytes; void *stream;
    int32_t *rank;  // bp_validate: the armed rank pointer (t_rank_out), consumed
};

int bp_validate(BpArgs &a)
{
    a.rank = nullptr;
    if (a.phase != EPRECON_BP_COUNT) {      // (the count half writes no rows: the pointer waits for the gather half)
        a.rank = t_rank_out;
        t_rank_out = nullptr;
    }
    if (a.rank && a.batch != 1) return EPRECON_ERR_ARG;      // (the rows of several batch elements interleave: no single raster)
    if (a.phase != 0 && a.feats_layout != EPRECON_LAYOUT_NHWC) return EPRECON_ERR_ARG;    // (NCHW: re-layout and count are one grid)
    if (a.phase == EPRECON_BP_COUNT && !a.feats) a.feats = a.krcam;   // (not read by this half)
    if (a.n < 0 || a.n > 0x7fffffff / 64 || a.batch <= 0 || a.n_views <= 0 || a.n_views > 32 || a.channels <= 0 ||
        a.height <= 1 || a.width <= 1 || a.mode < 0 || a.mode > 2)
        return EPRECON_ERR_ARG;
    if (!a.origin || !a.feats || !a.krcam || !a.n_valid_dev || !a.workspace) return EPRECON_ERR_ARG;
    if (a.n > 0 && (!a.coords || !a.count || (a.phase != EPRECON_BP_COUNT && (!a.out_feats || !a.out_coords))))
        return EPRECON_ERR_ARG;
    if ((size_t)a.n_views * a.batch * 12 * sizeof(float) > 32 * 1024) return EPRECON_ERR_UNSUPPORTED;
    if (a.workspace_bytes < eprecon_back_project_workspace_bytes(a.n, a.batch, a.n_views, a.channels, a.height, a.width,
                                                                 a.feats_layout))
        return EPRECON_ERR_WORKSPACE;
    if ((size_t)a.n_views * a.batch * a.channels * a.height * a.width > 0x7fffffffull) return EPRECON_ERR_UNSUPPORTED;
    if (a.feats_layout != EPRECON_LAYOUT_NCHW && a.feats_layout != EPRECON_LAYOUT_NHWC) return EPRECON_ERR_ARG;
    return EPRECON_OK;
}

// Every decision of a call, taken once: the two switches, the tile, the launch chain, the workspace carve, the kernel arguments.
struct BpPlan {
    bool nchw, chain4, clear_in_relayout, mlp;   // mlp: bp_gather_mlp_kernel (else bp_gather_kernel)
    int vox, ntile, nblk_count;                  // (the scan is folded into the gather where p.fold is set)
    size_t lds_relayout, lds_count;
    int32_t *tile_sums, *blk_batch;              // workspace: tile totals at offset 0, then the count workgroups' per-batch rows
    float *nhwc;                                 // (null for one batch element), then the channels-last maps of an NCHW call
    BpParams p;
};

BpPlan bp_plan(const BpArgs &a)
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
    pl.tile_sums = reinterpret_cast<int32_t *>(ws);
    ws += ep::align_up((size_t)ep::ceil_div(n, 16) * sizeof(int32_t), 256);
    pl.blk_batch = a.batch > 1 ? reinterpret_cast<int32_t *>(ws) : nullptr;
    ws += ep::align_up((size_t)ep::ceil_div(n, 256) * a.batch * sizeof(int32_t), 256);
    pl.nhwc = reinterpret_cast<float *>(ws);
    pl.lds_relayout = (size_t)a.channels * (kTrPix + 1) * sizeof(float);
    pl.lds_count = ((size_t)a.n_views * a.batch * 12 + a.batch + 256 / ep::kWave) * 4 + 16;

    BpParams &p = pl.p;
    p.coords = a.coords; p.n = (int)n; p.origin = a.origin; p.batch = a.batch; p.voxel_size = a.voxel_size;
    p.feats_nhwc = pl.nchw ? pl.nhwc : a.feats; p.krcam = a.krcam;
    p.V = a.n_views; p.C = a.channels; p.Cs = a.channels; p.H = a.height; p.W = a.width;
    p.min_view = a.min_view; p.out_feats = a.out_feats; p.out_mean = a.out_mean; p.out_coords = a.out_coords;
    p.count = a.count; p.out_grid = a.out_grid; p.out_mask = a.out_mask; p.n_valid_dev = a.n_valid_dev;
    p.block_offsets = pl.tile_sums; p.rank = a.rank;
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

// the counters' memset where one is needed, then prepare (re-layout + count in one grid) or [re-layout,] count, then the scan
template <int VOX>
int bp_queue_count(const BpArgs &a, const BpPlan &pl)
{
    const BpParams &p = pl.p;
    hipStream_t st = (hipStream_t)a.stream;
    if (a.n == 0 || (pl.chain4 && !pl.clear_in_relayout))
        EP_HIP_CHECK(hipMemsetAsync(a.n_valid_dev, 0, sizeof(int32_t) * (size_t)(1 + a.batch), st));
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
    if (!p.fold) {
        hipLaunchKernelGGL(bp_scan_kernel, dim3(1), dim3(1024), 0, st, pl.tile_sums, pl.ntile, a.n_valid_dev,
                           (const int32_t *)pl.blk_batch, pl.nblk_count, a.batch);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

// the gather inside the profile bracket, then the depth normalisation of MEAN_DEPTH
template <int VOX>
int bp_queue_gather(const BpArgs &a, const BpPlan &pl)
{
    hipStream_t st = (hipStream_t)a.stream;
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

template <int VOX>
int bp_queue(const BpArgs &a, const BpPlan &pl)
{
    const int rc = a.phase != EPRECON_BP_GATHER ? bp_queue_count<VOX>(a, pl) : EPRECON_OK;
    return rc != EPRECON_OK || a.phase == EPRECON_BP_COUNT ? rc : bp_queue_gather<VOX>(a, pl);
}

int bp_async_impl(BpArgs a)
{
    const int rc = bp_validate(a);
    if (rc != EPRECON_OK) return rc;
    const BpPlan pl = bp_plan(a);
    switch (pl.vox) {   // the one place where the tile size becomes a template argument
        case 256: return bp_queue<256>(a, pl);
        case 64: return bp_queue<64>(a, pl);
        default: return bp_queue<16>(a, pl);
    }
}

// ---------------------------------------------------------------------------------------------
// eprecon_back_project_prepare_levels_async (host)
// ---------------------------------------------------------------------------------------------
BpArgs level_args(const eprecon_bp_level &lv, void *stream)
{
    return {EPRECON_BP_COUNT, lv.coords, lv.n, lv.origin, lv.batch, lv.voxel_size, lv.feats, lv.feats_layout, lv.krcam, lv.n_views,
            lv.channels, lv.height, lv.width, lv.min_view, lv.mode, nullptr, nullptr, nullptr, lv.count, nullptr, nullptr,
            lv.n_valid_dev, lv.workspace, lv.workspace_bytes, stream, nullptr};
}

// what bp_validate asks of a count half, for maps of either layout; a level without a list (coords == NULL) has its maps re-laid
// out into the workspace, where a list of n entries leaves them, and needs neither counters nor matrices
int bp_validate_level(BpArgs &a, bool listed)
{
    if (a.feats_layout != EPRECON_LAYOUT_NCHW && a.feats_layout != EPRECON_LAYOUT_NHWC) return EPRECON_ERR_ARG;
    if (listed && a.feats_layout == EPRECON_LAYOUT_NHWC && !a.feats) a.feats = a.krcam;   // (not read by a count)
    if (a.n < 0 || a.n > 0x7fffffff / 64 || a.batch <= 0 || a.n_views <= 0 || a.n_views > 32 || a.channels <= 0 ||
        a.height <= 1 || a.width <= 1 || a.mode < 0 || a.mode > 2)
        return EPRECON_ERR_ARG;
    if (!a.feats || !a.workspace) return EPRECON_ERR_ARG;
    if (listed && (!a.origin || !a.krcam || !a.n_valid_dev || (a.n > 0 && !a.count))) return EPRECON_ERR_ARG;
    if ((size_t)a.n_views * a.batch * 12 * sizeof(float) > 32 * 1024) return EPRECON_ERR_UNSUPPORTED;
    if (a.workspace_bytes < eprecon_back_project_workspace_bytes(a.n, a.batch, a.n_views, a.channels, a.height, a.width,
                                                                 a.feats_layout))
        return EPRECON_ERR_WORKSPACE;
    if ((size_t)a.n_views * a.batch * a.channels * a.height * a.width > 0x7fffffffull) return EPRECON_ERR_UNSUPPORTED;
    return EPRECON_OK;
}

int bp_prepare_levels_impl(const eprecon_bp_level *levels, int n_levels, hipStream_t st)
{
    if (!levels || n_levels <= 0 || n_levels > kMaxLevels) return EPRECON_ERR_ARG;
    BpArgs args[kMaxLevels];
    BpPlan plans[kMaxLevels];
    bool listed[kMaxLevels];
    for (int l = 0; l < n_levels; ++l) {
        args[l] = level_args(levels[l], st);
        listed[l] = levels[l].coords != nullptr;
        const int rc = bp_validate_level(args[l], listed[l]);
        if (rc != EPRECON_OK) return rc;
        plans[l] = bp_plan(args[l]);
        if (plans[l].nchw && plans[l].lds_relayout > 64 * 1024) return EPRECON_ERR_UNSUPPORTED;
    }
    // EPRECON_BP_LEVELS=0 (read per call), and the four-launch chain of EPRECON_BP_FOLD=0: every level's own launches, as the
    // one-level call queues them
    if (!eprecon_bp_levels() || plans[0].chain4) {
        for (int l = 0; l < n_levels; ++l) {
            const BpArgs &a = args[l];
            const BpPlan &pl = plans[l];
            int rc = EPRECON_OK;
            if (listed[l]) rc = pl.vox == 256 ? bp_queue_count<256>(a, pl) : (pl.vox == 64 ? bp_queue_count<64>(a, pl) : bp_queue_count<16>(a, pl));
            else if (pl.nchw)
                rc = eprecon_nchw_to_nhwc_async(a.feats, pl.nhwc, a.n_views * a.batch, a.channels, a.height * a.width, st);
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
            const BpArgs &a = args[l];
            const BpPlan &pl = plans[l];
            const bool count = listed[l] && a.n > 0;     // (an empty list: the counters are cleared, nothing else runs)
            if (listed[l] && a.n == 0)
                EP_HIP_CHECK(hipMemsetAsync(a.n_valid_dev, 0, sizeof(int32_t) * (size_t)(1 + a.batch), st));
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
        const BpArgs &a = args[l];
        const BpPlan &pl = plans[l];
        if (listed[l] && a.n > 0 && !pl.p.fold) {
            hipLaunchKernelGGL(bp_scan_kernel, dim3(1), dim3(1024), 0, st, pl.tile_sums, pl.ntile, a.n_valid_dev,
                               (const int32_t *)pl.blk_batch, pl.nblk_count, a.batch);
            EP_LAUNCH_CHECK();
        }
    }
    return EPRECON_OK;
}

}  // namespace

extern "C" {

size_t eprecon_back_project_workspace_bytes(int64_t n, int batch, int n_views, int channels,
                                            int height, int width, int feats_layout)
{
    size_t bytes = ep::align_up((size_t)ep::ceil_div(n > 0 ? n : 1, 16) * sizeof(int32_t), 256);
    bytes += ep::align_up((size_t)ep::ceil_div(n > 0 ? n : 1, 256) * (batch > 0 ? batch : 1) * sizeof(int32_t), 256);
    if (feats_layout == EPRECON_LAYOUT_NCHW)
        bytes += ep::align_up((size_t)n_views * batch * channels * height * width * sizeof(float), 256);
    return bytes + 256;
}

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

int eprecon_back_project_rank_out(int32_t *rank) { t_rank_out = rank; return EPRECON_OK; }

int eprecon_init_glue(void) { return ep::switch_off("EPRECON_INIT_GLUE") ? 0 : 1; }

int eprecon_back_project_async(const int32_t *coords, int64_t n, const float *origin, int batch, float voxel_size, const float *feats,
                               int feats_layout, const float *krcam, int n_views, int channels, int height, int width,
                               int min_view, int mode, float *out_feats, float *out_mean, int32_t *out_coords, float *count,
                               float *out_grid, uint8_t *out_mask, int32_t *n_valid_dev, void *workspace, size_t workspace_bytes,
                               void *stream)
{
    return bp_async_impl({0, coords, n, origin, batch, voxel_size, feats, feats_layout, krcam, n_views, channels, height, width,
                          min_view, mode, out_feats, out_mean, out_coords, count, out_grid, out_mask, n_valid_dev, workspace,
                          workspace_bytes, stream, nullptr});
}

int eprecon_back_project_phase_async(int phase, const int32_t *coords, int64_t n, const float *origin, int batch, float voxel_size,
                                     const float *feats, int feats_layout, const float *krcam, int n_views, int channels,
                                     int height, int width, int min_view, int mode, float *out_feats, float *out_mean,
                                     int32_t *out_coords, float *count, float *out_grid, uint8_t *out_mask, int32_t *n_valid_dev,
                                     void *workspace, size_t workspace_bytes, void *stream)
{
    if (phase != EPRECON_BP_COUNT && phase != EPRECON_BP_GATHER) return EPRECON_ERR_ARG;
    return bp_async_impl({phase, coords, n, origin, batch, voxel_size, feats, feats_layout, krcam, n_views, channels, height, width,
                          min_view, mode, out_feats, out_mean, out_coords, count, out_grid, out_mask, n_valid_dev, workspace,
                          workspace_bytes, stream, nullptr});
}

int eprecon_back_project(const int32_t *coords, int64_t n, const float *origin, int batch, float voxel_size, const float *feats,
                         int feats_layout, const float *krcam, int n_views, int channels, int height, int width, int min_view,
                         int mode, int min_valid_per_batch, float *out_feats, float *out_mean, int32_t *out_coords, float *count,
                         float *out_grid, uint8_t *out_mask, int32_t *n_valid_dev, int32_t *n_valid_host, void *workspace,
                         size_t workspace_bytes, void *stream)
{
    if (!n_valid_host) return EPRECON_ERR_ARG;
    const int rc = eprecon_back_project_async(coords, n, origin, batch, voxel_size, feats, feats_layout, krcam, n_views, channels,
                                              height, width, min_view, mode, out_feats, out_mean, out_coords, count, out_grid,
                                              out_mask, n_valid_dev, workspace, workspace_bytes, stream);
    if (rc != EPRECON_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    EP_HIP_CHECK(hipMemcpyAsync(n_valid_host, n_valid_dev, sizeof(int32_t) * (size_t)(1 + batch), hipMemcpyDeviceToHost, st));
    EP_HIP_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < batch; ++b)
        if (n_valid_host[1 + b] < min_valid_per_batch) return EPRECON_EMPTY;
    return EPRECON_OK;
}

size_t eprecon_back_project_workspace_maps_offset(int64_t n, int batch)
{
    return ep::align_up((size_t)ep::ceil_div(n, 16) * sizeof(int32_t), 256) +
           ep::align_up((size_t)ep::ceil_div(n, 256) * batch * sizeof(int32_t), 256);
}

int eprecon_bp_levels(void) { return ep::switch_off("EPRECON_BP_LEVELS") ? 0 : 1; }

int eprecon_back_project_prepare_levels_async(const eprecon_bp_level *levels, int n_levels, void *stream)
{
    return bp_prepare_levels_impl(levels, n_levels, (hipStream_t)stream);
}

}  // extern "C"
