// Shared device/host helpers for libeprecon_hip.so (gfx950 only; wave = 64, 8 XCDs).
//
// The whole library is compiled with -ffp-contract=off: wherever a fused multiply-add is part of
// the arithmetic contract (or wanted for speed) it is written as fmaf()/__fmaf_rn explicitly, and
// nowhere else may the compiler fuse — bit-exact voxel indices depend on it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "../../include/eprecon_hip.h"

#define EP_HIP_CHECK(expr)                                            \
    do {                                                              \
        hipError_t e_ = (expr);                                       \
        if (e_ != hipSuccess) return EPRECON_ERR_HIP_BASE - (int)e_;  \
    } while (0)
#define EP_LAUNCH_CHECK() EP_HIP_CHECK(hipGetLastError())

namespace ep {

constexpr int kWave = 64;
constexpr int kXcd = 8;

static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
static inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// an on/off environment switch that defaults to on: NAME=0 turns it off.  Read at every call: tests flip the switches.
inline bool switch_off(const char *name)
{
    const char *e = getenv(name);
    return e && e[0] == '0';
}
// ... and one that defaults to off (an opt-in): NAME=1 turns it on
inline bool switch_on(const char *name)
{
    const char *e = getenv(name);
    return e && e[0] == '1';
}

// A run-time value picks a template argument: f (a generic lambda) gets, as a std::integral_constant, the X of the list that
// equals x; the last X of the list takes every other value.
template <int X, int... Rest, class F>
int pick(int x, F &&f)
{
    if constexpr (sizeof...(Rest) == 0) return f(std::integral_constant<int, X>{});
    else return x == X ? f(std::integral_constant<int, X>{}) : pick<Rest...>(x, f);
}

// Dynamic LDS a workgroup may ask for when its kernel has not opted in to more (hipFuncAttributeMaxDynamicSharedMemorySize; the
// back-projection kernels do not): what the device reports per workgroup (a property query), and never more than 64 KiB.
static inline size_t dynamic_lds_limit()
{
    static const size_t limit = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess || v <= 0)
            v = 64 * 1024;
        return (size_t)(v < 64 * 1024 ? v : 64 * 1024);
    }();
    return limit;
}

// Hardware block id -> logical block id.  The dispatcher places hardware block h on XCD h % 8
// (observed, speed only); this bijection gives every XCD one contiguous range of logical blocks
// so that neighbouring tiles, which touch neighbouring image regions, share one L2.
__device__ __forceinline__ int xcd_remap(int hw_bid, int nblk)
{
    const int q = nblk / kXcd, r = nblk % kXcd;
    const int xcd = hw_bid % kXcd, k = hw_bid / kXcd;
    const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
    return start + k;
}

// The count mailbox, device side (count_mailbox.hip; eprecon_mailbox_slot::payload_dev and ::seq): called by ONE thread -- the
// one that has just written the same n words to device memory -- it stores them into the slot's payload (host-coherent pinned
// memory), fences at system scope, and release-stores the sequence word in front of the payload, which is what the host
// spins on.  Stores only: nothing on the device reads the mailbox or waits for the host.
__device__ __forceinline__ void mailbox_publish(int32_t *payload, uint32_t seq, const int32_t *values, int n)
{
    for (int i = 0; i < n; ++i) payload[i] = values[i];
    __threadfence_system();
    __hip_atomic_store(reinterpret_cast<uint32_t *>(payload) - 1, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Exclusive rank of this thread among the threads of its block for which `pred` holds, by wave
// ballot + popcount and a per-wave count table in LDS (`wave_counts` holds BLOCK/64 ints).
// Contains one __syncthreads(); every thread of the block must call it.
template <int BLOCK>
__device__ __forceinline__ int block_exclusive_rank(bool pred, int *wave_counts, int &block_total)
{
    const unsigned long long m = __ballot(pred);
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = threadIdx.x / kWave;
    const int within = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wave_counts[wid] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < BLOCK / kWave; ++w) {
        const int c = wave_counts[w];
        off += (w < wid) ? c : 0;
        tot += c;
    }
    block_total = tot;
    return off + within;
}

// Several device regions filled with a 32-bit pattern each in ONE launch (instead of a hipMemsetAsync / clear kernel per
// region): the prologues of the stage calls clear a handful of index volumes, counters and hash tables of a few MB each, and
// every launch they do not need is ~5 us of a fragment's chain.  Regions: 4-byte aligned, sizes multiples of 4 bytes.
// (fill.hip; the device-wide scan is declared in scan.hpp, tables and kernel maps in hashgrid.hpp)
struct FillRegion {
    void *p;
    size_t bytes;
    uint32_t value;
};
constexpr int kMaxFillRegions = 12;
int multi_fill(const FillRegion *regions, int count, hipStream_t st);

// eprecon_trilinear_map_async without hash probes (csrc/voxelize.hip): base_row[i] = row of point i's base voxel in the set whose
// 3x3x3 kernel map nbr27 int32[27][m] is given; the corners are that voxel's neighbours at the offsets {0, +1}^3
int trilinear_from_map(const float *points_xyzb, int64_t n, const int32_t *base_row, const int32_t *nbr27, int64_t m, int stride,
                       int32_t *idx8, float *weight8, void *stream);

// A side stream of the library's own per caller stream, for entry points that issue two independent chains of small launches
// (csrc/gru_stage_finish.hip): record ev_fork on the caller's stream and let `side` wait for it, issue the second chain on
// `side`, record ev_join there and let the caller's stream wait for it.
struct Fork {
    hipStream_t main = nullptr, side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
};
int fork_for(hipStream_t main, Fork &out);

// the gather-kernel timing hook of eprecon_profile_enable (profile.hip): every gather variant brackets its launch with these
int profile_bracket_begin(hipStream_t st);
int profile_bracket_end(hipStream_t st, const char *kernel);

}  // namespace ep
