// Back-projection, device code of the first half (only back_project.hip includes this): the arguments every kernel of the
// family takes (BpParams), the cheap bit-exact projection, the visible-view count with its tile totals (count_body), and the
// kernels that run it -- alone (bp_count_kernel), in one grid with the re-layout of NCHW maps (bp_prepare_kernel), or for
// several levels at once (bp_prepare_levels_kernel) -- the scan of the tile totals for lists the gather does not fold it
// into (bp_scan_kernel), and the re-layout kernel on its own.  The gather: back_project_gather.hpp.  Host: back_project.hip.
#pragma once
#include "back_project_common.hpp"

namespace {
using namespace ep;

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
    int32_t *rank;  // [n + 1] or null: list entry -> output row or -1, then one word 0 (eprecon_bp_call::rank)
    int32_t *counts_host;  // count mailbox (eprecon_bp_call::counts_host / counts_seq) or null: whoever writes n_valid_dev[0 .. B]
    uint32_t counts_seq;   // publishes the same words there (ep::mailbox_publish)
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

// exclusive scan of the block totals, one workgroup; also publishes n_valid -- to n_valid_dev[0 .. batch] and, for a call with
// a count mailbox (mb_payload, mb_seq), to the host.  write_back = 0: the totals are left as they are (the early publish of a
// count half whose gather folds the scan in and wants the raw totals): only the counters are written.
__global__ __launch_bounds__(1024) void bp_scan_kernel(int32_t *block_sums, int nblk,
                                                       int32_t *n_valid_dev, const int32_t *blk_batch = nullptr,
                                                       int nblk_count = 0, int batch = 0, int write_back = 1,
                                                       int32_t *mb_payload = nullptr, uint32_t mb_seq = 0)
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
        if (write_back && i < nblk) block_sums[i] = carry + woff + x - v;
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
    if (tid == 0 && mb_payload) mailbox_publish(mb_payload, mb_seq, n_valid_dev, 1 + batch);   // (its own stores, read back)
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

}  // namespace
