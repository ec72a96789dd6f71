// Back-projection, device code of the second half (only back_project.hip includes this): the output row of a tile from
// the tile totals (tile_base_*), the rank volume of a dense raster (gather_rank_store), the two gather kernels and the
// depth normalisation of MEAN_DEPTH.  BpParams, project_fast and the count: back_project_count.hpp.
#pragma once
#include "back_project_count.hpp"

namespace {

// Two gather kernels are in the build: bp_gather_mlp_kernel (per-pair taps in LDS, cheap projection, buffer loads: 122 us on the
// dense 96^3 level, C = 24, 120x160 maps) and bp_gather_kernel (taps recomputed: 134 us; takes C % 4 != 0).  2 / 3 / 4 views of
// loads in flight per lane measured 126 / 129 / 138 us: the L1 access rate bounds the kernel (23 accesses per wave load), not
// latency.  The other variants tried and removed, with their figures: DESIGN.md 3a and the git history of this file.

// ---------------------------------------------------------------------------------------------
// The scan folded into the gather (BpParams::fold): the count launch has finished, so its tile totals are plain
// read-only data, and a gather workgroup gets the output row of its tile by summing the totals in front of it
// (the pattern of kernel_map.hip's scan_apply<true>) -- at 3,456 tiles at most 13.5 four-byte L2 loads per
// thread -- instead of the whole chip waiting for one scanning workgroup between two launches.  No look-back,
// no ticket, no spin: nothing here waits for another workgroup.
//   tile_base_partials   before phase 1: per-wave partial sums -> sFold (2 x BLOCK/64 ints)
//   tile_base_finish     after the next barrier of the caller (block_exclusive_rank's): the sums; the workgroup
//                        of the last tile publishes n_valid_dev[0 .. B] (what bp_scan_kernel published; its thread 0
//                        also hands them to the host through the call's count mailbox, when it has one), and
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
        if (tid == 0 && p.counts_host) mailbox_publish(p.counts_host, p.counts_seq, p.n_valid_dev, 1 + p.batch);
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

}  // namespace
