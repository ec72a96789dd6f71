// Object inventory of a saved scene (eprecon_amd/scene_objects.py): per segment of the voxel rows, the integer
// moments (count, sums, sums of products, min / max per axis) and the extents of the rows along a direction per segment.
//
// Every statistic is an integer sum, an integer min / max or a min / max of doubles, so the result depends neither on the order
// the lanes ran in nor on the path below.  Rows come in raster or file order: neighbouring rows mostly share their segment and
// a handful of segments (floor, wall) own most rows, so sent to memory the updates queue on a few words.  As in
// panoptic_score.hip, a table of up to kLdsSegments segments is therefore first combined per workgroup in LDS (128 B a
// segment for the moments: 32 KB, four workgroups a CU; 32 B for the extents) and every workgroup sends its non-identity
// entries to memory once at its end; a larger table takes every update straight to memory.  EPRECON_SS_LDS=0 turns the LDS
// table off (timing, tests).  There is no wave-level leader loop in front of the LDS table: see DESIGN.md 7aj.
//
// min / max of doubles as 64-bit integer atomics on the doubles' own bits: among values >= +0 the bits order like the values
// as signed or unsigned integers, among values < 0 they order the other way round, and every negative value's bits are
// negative as a signed and above every non-negative value's as an unsigned integer.  So a minimum takes a value >= +0 with a
// signed min and a negative one with an unsigned max; a maximum takes a value >= +0 with a signed max and a negative one with
// an unsigned min.  -0 is stored as +0 (the one pair of equal doubles with different bits).
#include <algorithm>

#include "common.hpp"

namespace {

using namespace ep;

constexpr int kLdsSegments = 256;     // table in LDS: 32 KB a workgroup for the moments
constexpr int kLdsBlocks = 512;       //   two workgroups per CU, each over several rounds of rows
constexpr int kMaxBlocks = 2048;      // table in memory: the waves stride over the rest
constexpr int64_t kMaxRows = (int64_t)1 << 24;
constexpr int kMaxSegments = 1 << 24;
constexpr int kCoordLimit = (1 << 19) - 2;      // the hash grid's range (hashgrid.hpp)
constexpr int kMomentCols = 16, kExtentCols = 4;
constexpr long long kPosInf = 0x7ff0000000000000ll, kNegInf = (long long)0xfff0000000000000ull;

__device__ __forceinline__ long long moment_identity(int col) { return col < 10 ? 0 : col < 13 ? 0x7fffffffll : -0x80000000ll; }

__device__ __forceinline__ long long extent_identity(int col) { return (col & 1) ? kNegInf : kPosInf; }

// column `col` of a moments row takes v
template <int SCOPE>
__device__ __forceinline__ void moment_update(long long *row, int col, long long v)
{
    if (col < 10) __hip_atomic_fetch_add(row + col, v, __ATOMIC_RELAXED, SCOPE);
    else if (col < 13) __hip_atomic_fetch_min(row + col, v, __ATOMIC_RELAXED, SCOPE);
    else __hip_atomic_fetch_max(row + col, v, __ATOMIC_RELAXED, SCOPE);
}

// column `col` of an extents row (min, max, min, max) takes the double whose bits are b (never -0, never a NaN)
template <int SCOPE>
__device__ __forceinline__ void extent_update(long long *row, int col, long long b)
{
    unsigned long long *urow = reinterpret_cast<unsigned long long *>(row);
    if (col & 1) {
        if (b >= 0) __hip_atomic_fetch_max(row + col, b, __ATOMIC_RELAXED, SCOPE);
        else __hip_atomic_fetch_min(urow + col, (unsigned long long)b, __ATOMIC_RELAXED, SCOPE);
    } else {
        if (b >= 0) __hip_atomic_fetch_min(row + col, b, __ATOMIC_RELAXED, SCOPE);
        else __hip_atomic_fetch_max(urow + col, (unsigned long long)b, __ATOMIC_RELAXED, SCOPE);
    }
}

__device__ __forceinline__ long long double_bits(double d)
{
    const long long b = __double_as_longlong(d);
    return b == (long long)0x8000000000000000ull ? 0 : b;
}

// -> the row takes part; a rank outside [-1, n] sets bit 1, a coordinate outside the hash grid's range bit 2 of `flags`
__device__ __forceinline__ bool ss_row(const int32_t *coords, const int32_t *rank, int64_t i, int n, int &r, int &x, int &y, int &z,
                                       int &flags)
{
    r = rank[i];
    if (r < 0 || r >= n) {
        if (r != -1 && r != n) flags |= 1;
        return false;
    }
    x = coords[3 * i], y = coords[3 * i + 1], z = coords[3 * i + 2];
    if (x < -kCoordLimit || x > kCoordLimit || y < -kCoordLimit || y > kCoordLimit || z < -kCoordLimit || z > kCoordLimit) {
        flags |= 2;
        return false;
    }
    return true;
}

__global__ __launch_bounds__(256) void ss_init_kernel(long long *table, int64_t entries, int cols, int32_t *status)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e == 0) status[0] = 0;
    if (e < entries) {
        const int col = (int)(e % cols);
        table[e] = cols == kMomentCols ? moment_identity(col) : extent_identity(col);
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void ss_moments_kernel(const int32_t *coords, const int32_t *rank, int64_t m, int n, long long *table,
                                                         int32_t *status)
{
    __shared__ long long s_table[LDS ? kLdsSegments * kMomentCols : 1];
    constexpr int SCOPE = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    const int entries = LDS ? n * kMomentCols : 0;      // (n <= kLdsSegments on this path)
    if (LDS) {
        for (int e = threadIdx.x; e < entries; e += 256) s_table[e] = moment_identity(e & (kMomentCols - 1));
        __syncthreads();
    }
    int flags = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
        int r, x, y, z;
        if (!ss_row(coords, rank, i, n, r, x, y, z, flags)) continue;
        long long *row = (LDS ? s_table : table) + (int64_t)r * kMomentCols;
        const long long lx = x, ly = y, lz = z;
        const long long v[kMomentCols] = {1, lx, ly, lz, lx * lx, lx * ly, lx * lz, ly * ly, ly * lz, lz * lz, lx, ly, lz, lx, ly, lz};
#pragma unroll
        for (int c = 0; c < kMomentCols; ++c) moment_update<SCOPE>(row, c, v[c]);
    }
    if (flags) atomicOr(&status[0], flags);
    if (LDS) {
        // (every thread of the workgroup arrives here: there is no early exit above)
        __syncthreads();
        for (int e = threadIdx.x; e < entries; e += 256) {
            const int col = e & (kMomentCols - 1);
            const long long v = s_table[e];
            if (v != moment_identity(col)) moment_update<__HIP_MEMORY_SCOPE_AGENT>(table + (e - col), col, v);
        }
    }
}

template <bool LDS>
__global__ __launch_bounds__(256) void ss_extents_kernel(const int32_t *coords, const int32_t *rank, int64_t m, int n, const double *dirs,
                                                         long long *ext, int32_t *status)
{
    __shared__ long long s_table[LDS ? kLdsSegments * kExtentCols : 1];
    constexpr int SCOPE = LDS ? __HIP_MEMORY_SCOPE_WORKGROUP : __HIP_MEMORY_SCOPE_AGENT;
    const int entries = LDS ? n * kExtentCols : 0;
    if (LDS) {
        for (int e = threadIdx.x; e < entries; e += 256) s_table[e] = extent_identity(e);
        __syncthreads();
    }
    int flags = 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += stride) {
        int r, x, y, z;
        if (!ss_row(coords, rank, i, n, r, x, y, z, flags)) continue;
        const double c = dirs[2 * (int64_t)r], s = dirs[2 * (int64_t)r + 1];
        // (-ffp-contract=off: the products, the sum and the difference are each rounded, as numpy rounds them)
        const double u = (double)x * c + (double)y * s;
        const double v = (double)y * c - (double)x * s;
        if (u != u || v != v) continue;      // (a direction that is not finite: the caller's; NaN bits never reach an atomic)
        long long *row = (LDS ? s_table : ext) + (int64_t)r * kExtentCols;
        const long long bu = double_bits(u), bv = double_bits(v);
        extent_update<SCOPE>(row, 0, bu);
        extent_update<SCOPE>(row, 1, bu);
        extent_update<SCOPE>(row, 2, bv);
        extent_update<SCOPE>(row, 3, bv);
    }
    if (flags) atomicOr(&status[0], flags);
    if (LDS) {
        __syncthreads();
        for (int e = threadIdx.x; e < entries; e += 256) {
            const int col = e & (kExtentCols - 1);
            const long long b = s_table[e];
            if (b != extent_identity(col)) extent_update<__HIP_MEMORY_SCOPE_AGENT>(ext + (e - col), col, b);
        }
    }
}

bool ss_use_lds(int n) { return n <= kLdsSegments && !switch_off("EPRECON_SS_LDS"); }

int ss_check(const int32_t *coords, const int32_t *rank, int64_t m, int n, const void *table, const int32_t *status)
{
    if (m < 0 || n < 0 || !status || (m > 0 && (!coords || !rank)) || (n > 0 && !table)) return EPRECON_ERR_ARG;
    if (m >= kMaxRows || n > kMaxSegments) return EPRECON_ERR_UNSUPPORTED;
    return EPRECON_OK;
}

int ss_init(void *table, int n, int cols, int32_t *status, hipStream_t st)
{
    const int64_t entries = (int64_t)n * cols;
    hipLaunchKernelGGL(ss_init_kernel, dim3((unsigned)std::max<int64_t>(ceil_div(entries, 256), 1)), dim3(256), 0, st,
                       static_cast<long long *>(table), entries, cols, status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int ss_blocks(int64_t m, bool lds) { return (int)std::min<int64_t>(ceil_div(m, 256), lds ? kLdsBlocks : kMaxBlocks); }

}  // namespace

extern "C" {

int32_t eprecon_segment_stats_lds_segments(void) { return kLdsSegments; }

int eprecon_segment_moments_async(const int32_t *coords, const int32_t *rank, int64_t m, int32_t n_segments, int64_t *table,
                                  int32_t *status, void *stream)
{
    if (const int rc = ss_check(coords, rank, m, n_segments, table, status)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = ss_init(table, n_segments, kMomentCols, status, st)) return rc;
    if (m == 0 || n_segments == 0) return EPRECON_OK;
    const bool lds = ss_use_lds(n_segments);
    hipLaunchKernelGGL(lds ? ss_moments_kernel<true> : ss_moments_kernel<false>, dim3(ss_blocks(m, lds)), dim3(256), 0, st, coords, rank,
                       m, n_segments, reinterpret_cast<long long *>(table), status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_segment_extents_async(const int32_t *coords, const int32_t *rank, int64_t m, int32_t n_segments, const double *dirs,
                                  double *ext, int32_t *status, void *stream)
{
    if (const int rc = ss_check(coords, rank, m, n_segments, ext, status)) return rc;
    if (n_segments > 0 && !dirs) return EPRECON_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (const int rc = ss_init(ext, n_segments, kExtentCols, status, st)) return rc;
    if (m == 0 || n_segments == 0) return EPRECON_OK;
    const bool lds = ss_use_lds(n_segments);
    hipLaunchKernelGGL(lds ? ss_extents_kernel<true> : ss_extents_kernel<false>, dim3(ss_blocks(m, lds)), dim3(256), 0, st, coords, rank,
                       m, n_segments, dirs, reinterpret_cast<long long *>(ext), status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
