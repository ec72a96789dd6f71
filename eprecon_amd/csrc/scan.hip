// Device-wide exclusive scan of int32 (n up to 2^31): one to three launches, deterministic.  Every compaction and numbering of the
// library runs on it (unique voxel ids, marching cubes, the global map, voxel down-sampling, segment lists, ...).
//
// Forms, by length: one workgroup up to 32,768 elements; beyond that tile sums + apply over tiles of kScanTile (scan.hpp)
// elements, with a launch that scans the sums in between above 4,096 tiles.
//
// State: a launch touches only the scratch its caller handed it, scan_scratch_ints(n) int32 (scan.hpp): the tile sums, written
// by one launch and read by the next on the same stream.  No workgroup waits for another, nothing is polled, nothing outlives
// a call and nothing is shared between calls, streams or devices.  (The one-launch decoupled look-back form of round 6 handed
// tile words between workgroups through process-global arrays in rotation.  Given private, freshly zeroed words in the
// caller's scratch it was slower than these two launches at both lengths measured, 7.4 against 7.0 us on 100,003 elements and
// 9.6 against 7.2 us on 320,868, and it left: profiles/r21/scan_private_state.txt.)
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

/* int32 of scratch a scan over n elements takes (0 for n <= 0 or n >= 2^31): one per tile of kScanTile elements. */
size_t eprecon_exclusive_scan_scratch_ints(int64_t n) { return n > 0 && n <= 0x7fffffff ? (size_t)ep::scan_scratch_ints(n) : 0; }

/* out[i] = sum of in[0 .. i) (int32, n < 2^31); *total (optional) = the grand total; scratch: eprecon_exclusive_scan_scratch_ints(n)
 * int32.  The call cannot see how much it was given: the query is the contract.  The device-wide scan every compaction /
 * numbering of the path runs on: one workgroup up to 32,768 elements, tile sums + apply beyond. */
int eprecon_exclusive_scan_async(const int32_t *in, int64_t n, int32_t *out, int32_t *total, int32_t *scratch, void *stream)
{
    if (n < 0 || n > 0x7fffffff || (n > 0 && (!in || !out || !scratch))) return EPRECON_ERR_ARG;
    return ep::exclusive_scan_i32(in, (int)n, out, scratch, total, (hipStream_t)stream);
}

}  // extern "C"
