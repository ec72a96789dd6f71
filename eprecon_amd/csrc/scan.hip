// Device-wide exclusive scan of int32 (n up to 2^31): one to three launches, deterministic.  Every compaction and numbering of the
// library runs on it (unique voxel ids, marching cubes, the global map, voxel down-sampling, segment lists, ...).
//
// Forms, by length: one workgroup up to 32,768 elements; one decoupled look-back launch up to 4,096 tiles of kScanTile
// (scan.hpp) elements; beyond that, or with EPRECON_SCAN_LOOKBACK=0, tile sums + apply, with a launch that scans the sums in
// between above 4,096 tiles.  Only the tile-sum forms touch the caller's scratch: scan_scratch_ints(n) int32, one per tile.
//
// Look-back state, as it is today: the tile words and the two counters of a launch live in process-global __device__ arrays
// (g_lb_state, g_lb_ctr) cut into 64 sets.  A host-side counter hands every launch the next set in rotation, and the last
// tile of a launch zeroes its set.  A set is tied neither to a stream nor to a device (the symbol addresses are looked up once
// per process): nothing keeps a launch from sharing its set with the launch issued 64 scans later on another stream.  That is the
// open finding at the head of ADVICE.md; its fix (per-launch state carved from the caller's scratch) starts from
// scan_scratch_ints, the one place that sizes the scratch.
#include <atomic>

#include "scan.hpp"

namespace {
using namespace ep;

constexpr int kScanBlock = 256;
constexpr int kScanItems = 8;                       // per thread
static_assert(kScanTile == kScanBlock * kScanItems, "scan.hpp sizes the callers' scratch by this tile");

// (n_dev, optional: the live length is min(n, *n_dev) — the launch is sized by the capacity n, the count lives on the device)
__global__ __launch_bounds__(kScanBlock) void scan_tile_sums(const int32_t *in, int n, int32_t *sums, const int32_t *n_dev)
{
    __shared__ int sWave[kScanBlock / kWave];
    if (n_dev) n = min(n, *n_dev);
    const int base = blockIdx.x * kScanTile;
    int s = 0;
    for (int k = 0; k < kScanItems; ++k) {
        const int i = base + k * kScanBlock + threadIdx.x;
        if (i < n) s += in[i];
    }
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) s += __shfl_xor(s, d);
    if ((threadIdx.x & (kWave - 1)) == 0) sWave[threadIdx.x / kWave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kScanBlock / kWave; ++w) t += sWave[w];
        sums[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void scan_sums_inplace(int32_t *sums, int nblk, int32_t *total)
{
    __shared__ int sWave[1024 / kWave];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    int carry = 0;
    for (int base = 0; base < nblk; base += 1024) {
        const int i = base + tid;
        const int v = i < nblk ? sums[i] : 0;
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
        if (i < nblk) sums[i] = carry + woff + x - v;
        carry += tot;
        __syncthreads();
    }
    if (tid == 0 && total) *total = carry;
}

// out[i] = exclusive prefix of in[0..i); each block rescans its tile of kScanTile elements in LDS.
// RAW: `sums` holds the tile totals as scan_tile_sums left them and every workgroup adds up the totals in front of its own
// tile itself (a few hundred values: cheaper than the third launch that used to scan them); the last workgroup also
// publishes the grand total.
template <bool RAW>
__global__ __launch_bounds__(kScanBlock) void scan_apply(const int32_t *in, int n, const int32_t *sums,
                                                         int32_t *out, const int32_t *n_dev, int32_t *total)
{
    __shared__ int sWave[kScanBlock / kWave];
    __shared__ int sBase;
    if (n_dev) n = min(n, *n_dev);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    int tile_base;
    if (RAW) {
        int acc = 0;
        for (int j = tid; j < (int)blockIdx.x; j += kScanBlock) acc += sums[j];
#pragma unroll
        for (int d = kWave / 2; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) sWave[wid] = acc;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < kScanBlock / kWave; ++w) t += sWave[w];
            sBase = t;
            if (total && blockIdx.x == gridDim.x - 1) *total = t + sums[blockIdx.x];
        }
        __syncthreads();
        tile_base = sBase;
        __syncthreads();      // (sWave is reused below)
    } else {
        tile_base = sums[blockIdx.x];
    }
    const int base = blockIdx.x * kScanTile + tid * kScanItems;  // blocked arrangement
    int v[kScanItems];
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        s += v[k];
    }
    int x = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == kWave - 1) sWave[wid] = x;
    __syncthreads();
    int off = tile_base + x - s;
    for (int w = 0; w < wid; ++w) off += sWave[w];
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < n) out[base + k] = off;
        off += v[k];
    }
}

// short inputs: the whole scan in ONE workgroup and (round 6) ONE pass: 1024 threads x ITEMS items held in registers (8 / 16 /
// 32 by length), one barrier — the carried rounds of the first form (8 items per thread and round, two barriers each) made a
// 32,768-element scan a chain of four round trips: 12 us per launch, 21 launches per cfg4 fragment
constexpr int kSmallScanMax = 32768;
template <int ITEMS>
__global__ __launch_bounds__(1024) void scan_small_kernel(const int32_t *in, int n, int32_t *out, int32_t *total,
                                                          const int32_t *n_dev)
{
    __shared__ int sWave[1024 / kWave];
    if (n_dev) n = min(n, *n_dev);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int b0 = tid * ITEMS;  // blocked arrangement
    int v[ITEMS];
    int s = 0;
    if (b0 + ITEMS <= n && (reinterpret_cast<uintptr_t>(in) & 15) == 0) {
#pragma unroll
        for (int k = 0; k < ITEMS; k += 4) {
            const int4 q = *reinterpret_cast<const int4 *>(in + b0 + k);
            v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) v[k] = (b0 + k < n) ? in[b0 + k] : 0;
    }
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) s += v[k];
    int x = s;
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
    int off = woff + x - s;
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        if (b0 + k < n) out[b0 + k] = off;
        off += v[k];
    }
    if (tid == 0 && total) *total = tot;
}

// ---- long inputs in ONE launch (round 6): decoupled look-back -------------------------------------------------------------
// A tile (256 threads x 8 items) takes its index from a device counter (tiles start in index order, so every predecessor of a
// running tile has started: the look-back cannot wait for a workgroup that is not scheduled), publishes its total as
// {1, sum}, sums its predecessors' words 64 at a time with one wave until it meets an inclusive prefix {2, ...}, publishes its
// own inclusive prefix and scans its items behind that base.  One 64-bit word per tile carries flag and value together (no
// fence: a single agent-scope atomic store / load).  The words and the two counters live in a zero-initialised device array, one
// set per launch in rotation; the last tile to finish clears its set (graph replays reuse theirs).  Replaces tile-sums + apply
// (two launches) for up to kLbMaxTiles tiles; bit-identical results (integer sums).
constexpr int kLbSlots = 64, kLbMaxTiles = 4096;
__device__ unsigned long long g_lb_state[kLbSlots * kLbMaxTiles];
__device__ unsigned int g_lb_ctr[kLbSlots * 2];

__global__ __launch_bounds__(kScanBlock) void scan_lookback_kernel(const int32_t *in, int n, int32_t *out, int32_t *total,
                                                                   const int32_t *n_dev, unsigned long long *state, unsigned int *ctr)
{
    __shared__ int sWave[kScanBlock / kWave];
    __shared__ int sTile, sBase;
    if (n_dev) n = min(n, *n_dev);
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    const int ntiles = (int)gridDim.x;
    if (tid == 0) sTile = (int)atomicAdd(&ctr[0], 1u);
    __syncthreads();
    const int tile = sTile;
    const int base = tile * kScanTile + tid * kScanItems;  // blocked arrangement
    int v[kScanItems];
    int s = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = (base + k < n) ? in[base + k] : 0;
        s += v[k];
    }
    int x = s;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == kWave - 1) sWave[wid] = x;
    __syncthreads();
    int woff = 0, agg = 0;
#pragma unroll
    for (int w = 0; w < kScanBlock / kWave; ++w) {
        const int c = sWave[w];
        woff += (w < wid) ? c : 0;
        agg += c;
    }
    if (wid == 0) {      // one wave publishes and looks back
        int prefix = 0;
        if (tile > 0) {
            if (lane == 0)
                __hip_atomic_store(&state[tile], (1ull << 62) | (unsigned int)agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            int win = tile - 1;           // (wave-uniform) nearest predecessor of the current window of 64
            while (true) {
                const int j = win - lane;
                unsigned long long w = 0ull;
                if (j >= 0) {
                    do {
                        w = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } while ((w >> 62) == 0ull);
                }
                // lanes are ordered nearest predecessor first: everything up to (and including) the first inclusive prefix counts
                const unsigned long long incl = __ballot(j >= 0 && (w >> 62) == 2ull);
                const int first = incl ? __builtin_ctzll(incl) : kWave;
                int part = (j >= 0 && lane <= first) ? (int)(unsigned int)w : 0;
#pragma unroll
                for (int d = kWave / 2; d > 0; d >>= 1) part += __shfl_xor(part, d);
                prefix += part;
                if (incl || win < kWave) break;      // an inclusive prefix closes the sum; so does reaching tile 0
                win -= kWave;
            }
        }
        if (lane == 0) {
            __hip_atomic_store(&state[tile], (2ull << 62) | (unsigned int)(prefix + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            sBase = prefix;
            if (total && tile == ntiles - 1) *total = prefix + agg;
        }
    }
    __syncthreads();
    int off = sBase + woff + x - s;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        if (base + k < n) out[base + k] = off;
        off += v[k];
    }
    // the last tile to get here puts the set back to zero (every tile has read what it needed: it is past its look-back)
    __syncthreads();
    if (tid == 0) sTile = (int)atomicAdd(&ctr[1], 1u);
    __syncthreads();
    if (sTile == ntiles - 1) {
        for (int t = tid; t < ntiles; t += kScanBlock) __hip_atomic_store(&state[t], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid == 0) {
            __hip_atomic_store(&ctr[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&ctr[1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

namespace ep {
// scratch: scan_scratch_ints(n) int32.  `total_dev` (optional) receives the grand total.  n_dev (optional, device): the live
// length is min(n, *n_dev); launches are sized by n.
int exclusive_scan_i32_dn(const int32_t *in, int n, const int32_t *n_dev, int32_t *out, int32_t *scratch, int32_t *total_dev,
                          hipStream_t st)
{
    if (n <= 0) {
        if (total_dev) EP_HIP_CHECK(hipMemsetAsync(total_dev, 0, sizeof(int32_t), st));
        return EPRECON_OK;
    }
    if (n <= kSmallScanMax) {
        if (n <= 8192) hipLaunchKernelGGL(scan_small_kernel<8>, dim3(1), dim3(1024), 0, st, in, n, out, total_dev, n_dev);
        else if (n <= 16384) hipLaunchKernelGGL(scan_small_kernel<16>, dim3(1), dim3(1024), 0, st, in, n, out, total_dev, n_dev);
        else hipLaunchKernelGGL(scan_small_kernel<32>, dim3(1), dim3(1024), 0, st, in, n, out, total_dev, n_dev);
        EP_LAUNCH_CHECK();
        return EPRECON_OK;
    }
    const int nblk = (int)scan_scratch_ints(n);      // one scratch word per tile
    // EPRECON_SCAN_LOOKBACK=0: long scans as tile sums + apply (two launches, rounds 1-5; read per call)
    if (nblk <= kLbMaxTiles && !switch_off("EPRECON_SCAN_LOOKBACK")) {
        static unsigned long long *state_base = nullptr;
        static unsigned int *ctr_base = nullptr;
        if (!state_base) {
            EP_HIP_CHECK(hipGetSymbolAddress(reinterpret_cast<void **>(&state_base), HIP_SYMBOL(g_lb_state)));
            EP_HIP_CHECK(hipGetSymbolAddress(reinterpret_cast<void **>(&ctr_base), HIP_SYMBOL(g_lb_ctr)));
        }
        static std::atomic<unsigned> slot{0};
        const unsigned sidx = slot.fetch_add(1u) % (unsigned)kLbSlots;
        hipLaunchKernelGGL(scan_lookback_kernel, dim3(nblk), dim3(kScanBlock), 0, st, in, n, out, total_dev, n_dev,
                           state_base + (size_t)sidx * kLbMaxTiles, ctr_base + 2 * sidx);
        EP_LAUNCH_CHECK();
        return EPRECON_OK;
    }
    hipLaunchKernelGGL(scan_tile_sums, dim3(nblk), dim3(kScanBlock), 0, st, in, n, scratch, n_dev);
    EP_LAUNCH_CHECK();
    if (nblk <= 4096) {       // (8.4 M elements: two launches; the tile totals are summed by the consumers)
        hipLaunchKernelGGL(scan_apply<true>, dim3(nblk), dim3(kScanBlock), 0, st, in, n, scratch, out, n_dev, total_dev);
        EP_LAUNCH_CHECK();
        return EPRECON_OK;
    }
    hipLaunchKernelGGL(scan_sums_inplace, dim3(1), dim3(1024), 0, st, scratch, nblk, total_dev);
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_apply<false>, dim3(nblk), dim3(kScanBlock), 0, st, in, n, scratch, out, n_dev, (int32_t *)nullptr);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
int exclusive_scan_i32(const int32_t *in, int n, int32_t *out, int32_t *scratch, int32_t *total_dev, hipStream_t st)
{
    return exclusive_scan_i32_dn(in, n, nullptr, out, scratch, total_dev, st);
}
}  // namespace ep

extern "C" {

/* out[i] = sum of in[0 .. i) (int32, n < 2^31); *total (optional) = the grand total; scratch: one int32 per kScanTile elements (used by the
 * tile-sum forms only).  The device-wide scan every compaction / numbering of the path runs on: one workgroup up to 32,768
 * elements, one decoupled look-back launch up to 8.4 M. */
int eprecon_exclusive_scan_async(const int32_t *in, int64_t n, int32_t *out, int32_t *total, int32_t *scratch, void *stream)
{
    if (n < 0 || n > 0x7fffffff || (n > 0 && (!in || !out || !scratch))) return EPRECON_ERR_ARG;
    return ep::exclusive_scan_i32(in, (int)n, out, scratch, total, (hipStream_t)stream);
}

}  // extern "C"
