// Panoptic scoring (eprecon_amd/panoptic_score.py): the contingency table of predicted and ground-truth segments
// over the sites of a scene, int64[(n_pred + 1) * (n_gt + 2)].  The sites are either two rank lists (mesh vertices) or the cells of
// a lattice on the prediction's grid, whose ground-truth cell is found in fp64 per site: no site arrays, no resampled copy of
// the ground truth.
//
// Both kernels feed one combining step.  Neighbouring sites mostly share their pair (a wall, the empty space between the
// surfaces), so a wave counts its lanes per distinct pair with ballots (the leader loop of lt_vote_kernel, label_transfer.hip)
// and, on top of that, keeps the pair it met last in registers from one round of 64 sites to the next: a run of rounds over
// one pair ends in ONE atomic, where one add per round would queue ~10^5 of them on the single word of "nothing here on
// either side".  What is left is one add per pair a round holds beside the carried one, and in a room those land on a handful of
// words (the floor's pair is in almost every column of cells): sent to memory they queue on those words, and the voxel kernel
// took 0.97 ms at 270 x 265 x 120.  So a table of up to 8,192 entries (a scene of ~90 x 90 segments) is first summed per
// workgroup in 32 KB of LDS, in 32-bit words (a workgroup sees fewer than 2^31 sites), and every workgroup adds its non-zero
// words to memory once at its end; a larger table takes the adds straight to memory.  EPRECON_PC_LDS=0 turns the LDS table
// off (timing, tests).  Only integer adds are involved, so the table does not depend on the order or on the path.
#include <algorithm>

#include "common.hpp"

namespace {

using namespace ep;

constexpr int64_t kMaxTable = (int64_t)1 << 22;
constexpr int kMaxBlocks = 2048;      // table in memory: 8 workgroups of 4 waves per CU; the waves stride over the rest
constexpr int kLdsEntries = 8192;     // table in LDS: 32 KB a workgroup,
constexpr int kLdsBlocks = 1024;      //   4 workgroups per CU

struct PcCarry {
    int e;                      // table entry the wave is holding a count for (-1: none); wave-uniform
    unsigned long long n;
};

// the table the adds go to: the workgroup's LDS copy, or memory
template <bool LDS>
struct PcTable {
    unsigned long long *counts;
    unsigned *lds;
    __device__ __forceinline__ void add(int e, unsigned long long n) const
    {
        if (LDS) atomicAdd(&lds[e], (unsigned)n);
        else atomicAdd(&counts[e], n);
    }
};

template <bool LDS>
__device__ __forceinline__ void pc_table_begin(unsigned *lds, int entries)
{
    if (!LDS) return;
    for (int e = threadIdx.x; e < entries; e += 256) lds[e] = 0;
    __syncthreads();
}

// (every thread of the workgroup arrives here: the kernels have no early exit)
template <bool LDS>
__device__ __forceinline__ void pc_table_end(const unsigned *lds, int entries, unsigned long long *counts)
{
    if (!LDS) return;
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += 256)
        if (lds[e]) atomicAdd(&counts[e], (unsigned long long)lds[e]);
}

// e: this lane's table entry, -1 for a lane without a site.  Every lane of the wave calls it (the ballots need them all).
template <bool LDS>
__device__ __forceinline__ void pc_combine(int e, int lane, const PcTable<LDS> &T, PcCarry &carry)
{
    unsigned long long left = __ballot(e >= 0);
    if (!left) return;
    const unsigned long long held = __ballot(e >= 0 && e == carry.e);
    if (held) {
        carry.n += __popcll(held);
        left &= ~held;
    } else {
        if (carry.n && lane == 0) T.add(carry.e, carry.n);
        const int leader = __builtin_ctzll(left);
        carry.e = __shfl(e, leader);
        const unsigned long long same = __ballot(e == carry.e);
        carry.n = __popcll(same);
        left &= ~same;
    }
    while (left) {      // the other pairs of this round: one atomic each
        const int leader = __builtin_ctzll(left);
        const unsigned long long same = __ballot(e == __shfl(e, leader));
        if (lane == leader) T.add(e, (unsigned long long)__popcll(same));
        left &= ~same;
    }
}

template <bool LDS>
__device__ __forceinline__ void pc_flush(int lane, const PcTable<LDS> &T, const PcCarry &carry)
{
    if (carry.n && lane == 0) T.add(carry.e, carry.n);
}

// ranks -> table entry; -1 (and `bad`) when one of them is outside its range, so that it never reaches an atomic
__device__ __forceinline__ int pc_entry(int32_t p, int32_t g, int n_pred, int n_gt, bool &bad)
{
    if (p < -1 || p >= n_pred || g < -1 || g > n_gt) {
        bad = true;
        return -1;
    }
    return (p < 0 ? n_pred : p) * (n_gt + 2) + (g < 0 ? n_gt + 1 : g);      // (< 2^22: the host checked)
}

template <bool LDS>
__global__ __launch_bounds__(256) void pc_pair_count_kernel(const int32_t *pred_rank, const int32_t *gt_rank, int64_t n, int n_pred,
                                                            int n_gt, unsigned long long *counts, int32_t *status)
{
    __shared__ unsigned s_table[LDS ? kLdsEntries : 1];
    const int entries = (n_pred + 1) * (n_gt + 2);
    const PcTable<LDS> T{counts, s_table};
    pc_table_begin<LDS>(s_table, entries);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t stride = (int64_t)gridDim.x * 256;
    PcCarry carry{-1, 0};
    bool bad = false;
    // (base is the same in all lanes of a wave: they leave the loop together)
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < n; base += stride) {
        const int64_t i = base + lane;
        const int e = i < n ? pc_entry(pred_rank[i], gt_rank[i], n_pred, n_gt, bad) : -1;
        pc_combine(e, lane, T, carry);
    }
    pc_flush(lane, T, carry);
    if (__ballot(bad) && lane == 0) atomicOr(&status[0], 1);
    pc_table_end<LDS>(s_table, entries, counts);
}

struct PcGrid {
    double o[3], vs;      // fl64(origin_f32), voxel size
    int dims[3];
};

struct PcLattice {
    int lo[3];
    unsigned dims[3];
};

template <bool LDS>
__global__ __launch_bounds__(256) void pc_voxel_pair_count_kernel(const int32_t *pred_rank, const int32_t *gt_rank, const float *gt_tsdf,
                                                                  PcGrid P, PcGrid G, float gt_surface, PcLattice L, int64_t n,
                                                                  int n_pred, int n_gt, unsigned long long *counts, int32_t *status)
{
    __shared__ unsigned s_table[LDS ? kLdsEntries : 1];
    const int entries = (n_pred + 1) * (n_gt + 2);
    const PcTable<LDS> T{counts, s_table};
    pc_table_begin<LDS>(s_table, entries);
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t stride = (int64_t)gridDim.x * 256;
    PcCarry carry{-1, 0};
    bool bad = false;
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < n; base += stride) {
        const int64_t i = base + lane;
        int e = -1;
        if (i < n) {
            const unsigned s = (unsigned)i, xy = s / L.dims[2];      // (n < 2^31)
            const int k[3] = {L.lo[0] + (int)(xy / L.dims[1]), L.lo[1] + (int)(xy % L.dims[1]), L.lo[2] + (int)(s % L.dims[2])};
            int32_t p = -1, g = -1;
            if (k[0] >= 0 && k[0] < P.dims[0] && k[1] >= 0 && k[1] < P.dims[1] && k[2] >= 0 && k[2] < P.dims[2])
                p = pred_rank[((int64_t)k[0] * P.dims[1] + k[1]) * P.dims[2] + k[2]];
            int j[3];
            bool inside = true;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                // (-ffp-contract=off: the product, the sums and the quotient are each rounded, as numpy rounds them)
                const double w = P.o[a] + (double)k[a] * P.vs;
                const double f = floor((w - G.o[a]) / G.vs + 0.5);
                inside = inside && f >= 0.0 && f < (double)G.dims[a];
                j[a] = inside ? (int)f : 0;
            }
            if (inside) {
                const int64_t c = ((int64_t)j[0] * G.dims[1] + j[1]) * G.dims[2] + j[2];
                if (fabsf(gt_tsdf[c]) < gt_surface) {
                    g = gt_rank[c];
                    if (g == -1) bad = true, g = -2;      // (a present cell is a segment or void, never "absent")
                }
            }
            e = pc_entry(p, g, n_pred, n_gt, bad);
        }
        pc_combine(e, lane, T, carry);
    }
    pc_flush(lane, T, carry);
    if (__ballot(bad) && lane == 0) atomicOr(&status[0], 1);
    pc_table_end<LDS>(s_table, entries, counts);
}

// the table is summed in LDS first when it fits
bool pc_use_lds(int n_pred, int n_gt) { return (n_pred + 1) * (n_gt + 2) <= kLdsEntries && !switch_off("EPRECON_PC_LDS"); }

int pc_table_check(int n_pred, int n_gt, const int64_t *counts, const int32_t *status)
{
    if (n_pred < 0 || n_gt < 0 || !counts || !status) return EPRECON_ERR_ARG;
    if (((int64_t)n_pred + 1) * ((int64_t)n_gt + 2) > kMaxTable) return EPRECON_ERR_UNSUPPORTED;
    return EPRECON_OK;
}

int pc_clear(int n_pred, int n_gt, int64_t *counts, int32_t *status, hipStream_t st)
{
    EP_HIP_CHECK(hipMemsetAsync(counts, 0, (size_t)(n_pred + 1) * (n_gt + 2) * sizeof(int64_t), st));
    EP_HIP_CHECK(hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st));
    return EPRECON_OK;
}

bool pc_dims_ok(const int32_t *dims) { return dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1; }

int64_t pc_cells(const int32_t *dims) { return (int64_t)dims[0] * dims[1] * dims[2]; }

}  // namespace

extern "C" {

int eprecon_pair_count_async(const int32_t *pred_rank, const int32_t *gt_rank, int64_t n, int n_pred, int n_gt, int64_t *counts,
                             int32_t *status, void *stream)
{
    if (n < 0 || (n > 0 && (!pred_rank || !gt_rank))) return EPRECON_ERR_ARG;
    if (const int rc = pc_table_check(n_pred, n_gt, counts, status)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = pc_clear(n_pred, n_gt, counts, status, st)) return rc;
    if (n == 0) return EPRECON_OK;
    const bool lds = pc_use_lds(n_pred, n_gt) && n < ((int64_t)1 << 40);      // (32-bit LDS words: < 2^31 sites a workgroup)
    const int blocks = (int)std::min<int64_t>(ceil_div(n, 256), lds ? kLdsBlocks : kMaxBlocks);
    hipLaunchKernelGGL(lds ? pc_pair_count_kernel<true> : pc_pair_count_kernel<false>, dim3(blocks), dim3(256), 0, st, pred_rank,
                       gt_rank, n, n_pred, n_gt, reinterpret_cast<unsigned long long *>(counts), status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_voxel_pair_count_async(const int32_t *pred_rank, const int32_t *gt_rank, const float *gt_tsdf,
                                   const int32_t *pred_dims_host, const int32_t *gt_dims_host, const float *pred_origin_host,
                                   const float *gt_origin_host, double pred_voxel, double gt_voxel, float gt_surface,
                                   const int32_t *lattice_lo_host, const int32_t *lattice_dims_host, int n_pred, int n_gt,
                                   int64_t *counts, int32_t *status, void *stream)
{
    if (!pred_rank || !gt_rank || !gt_tsdf || !pred_dims_host || !gt_dims_host || !pred_origin_host || !gt_origin_host ||
        !lattice_lo_host || !lattice_dims_host || !(pred_voxel > 0.0) || !(gt_voxel > 0.0) || !pc_dims_ok(pred_dims_host) ||
        !pc_dims_ok(gt_dims_host) || !pc_dims_ok(lattice_dims_host))
        return EPRECON_ERR_ARG;
    if (const int rc = pc_table_check(n_pred, n_gt, counts, status)) return rc;
    const int64_t n = pc_cells(lattice_dims_host);
    if (n > 0x7fffffffll || pc_cells(pred_dims_host) > 0x7fffffffll || pc_cells(gt_dims_host) > 0x7fffffffll)
        return EPRECON_ERR_UNSUPPORTED;
    PcGrid P, G;
    PcLattice L;
    for (int a = 0; a < 3; ++a) {
        P.o[a] = (double)pred_origin_host[a], G.o[a] = (double)gt_origin_host[a];
        P.dims[a] = pred_dims_host[a], G.dims[a] = gt_dims_host[a];
        L.lo[a] = lattice_lo_host[a], L.dims[a] = (unsigned)lattice_dims_host[a];
        // (lo + extent must stay an int: the kernel adds a cell's offset to lo)
        if ((int64_t)lattice_lo_host[a] + lattice_dims_host[a] > 0x7fffffffll) return EPRECON_ERR_UNSUPPORTED;
    }
    P.vs = pred_voxel, G.vs = gt_voxel;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = pc_clear(n_pred, n_gt, counts, status, st)) return rc;
    const bool lds = pc_use_lds(n_pred, n_gt);
    const int blocks = (int)std::min<int64_t>(ceil_div(n, 256), lds ? kLdsBlocks : kMaxBlocks);
    hipLaunchKernelGGL(lds ? pc_voxel_pair_count_kernel<true> : pc_voxel_pair_count_kernel<false>, dim3(blocks), dim3(256), 0, st,
                       pred_rank, gt_rank, gt_tsdf, P, G, gt_surface, L, n, n_pred, n_gt,
                       reinterpret_cast<unsigned long long *>(counts), status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
