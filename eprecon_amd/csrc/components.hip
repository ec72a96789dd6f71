// Connected components of a sparse voxel set on gfx950: a lock-free union-find over the symmetric 3x3x3 self map
// (kernel_map.hip: eprecon_kernel_map_self_async), in three launches whatever the set looks like.
//
// The reference has no such stage (its users cluster the finished mesh in open3d afterwards); the rule is this project's
//  and is what eprecon_amd/clean_scene.py removes floaters and segment debris with.
//
//   init     parent[i] = i, status = 0
//   hook     one lane per row over the 13 offsets below the centre (the map is symmetric: the other 13 are some other row's):
//            find both roots, CAS the larger root onto the smaller, go on from the value the CAS returns when it loses
//   flatten  label[i] = find(i) behind the kernel boundary (-1 for a row whose key is negative)
//
// parent[i] <= i holds at every moment (a hook only ever stores a smaller root into a root, path halving only ever a smaller
// ancestor into a non-root), so a find walks strictly decreasing indices and ends; the tree of a component ends in its smallest
// row, whatever the order the lanes ran in: the labels are the same on every run.
//
// Visibility: inside the hooking launch EVERY access of parent[] is a relaxed agent-scope atomic (eight XCDs with private L2s:
// a plain load of a word another workgroup wrote in this launch may be stale).  No workgroup waits on another: there is no
// poll, ticket or grid barrier; every loop is bounded (n steps for a chain) and an overrun sets a bit of the status word and
// leaves the loop.  A stale read would cost steps, never the result: any value ever stored in parent[x] is an ancestor of x.
#include "common.hpp"

namespace {
using namespace ep;

constexpr int kBlock = 256;
constexpr int kStatusFindOverrun = 1;     // a chain longer than n (hook or flatten)
constexpr int kStatusHookOverrun = 2;     // a link retried more than n times

__device__ __forceinline__ int32_t load_parent(int32_t *parent, int32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x with path halving; every access atomic at agent scope.  false: more than `bound` steps (the caller stops)
__device__ __forceinline__ bool find_root(int32_t *parent, int32_t &x, int32_t bound)
{
    for (int32_t step = 0; step <= bound; ++step) {
        const int32_t p = load_parent(parent, x);
        if (p == x) return true;
        const int32_t g = load_parent(parent, p);
        // x is no root and never becomes one again; g is an ancestor of x below p (or p itself)
        if (g != p) __hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = g;
    }
    return false;
}

__global__ __launch_bounds__(kBlock) void components_init_kernel(int32_t *parent, int32_t n, int32_t *status)
{
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) *status = 0;
    if (i < n) parent[i] = i;
}

// max |d| <= 1 always holds in the 3x3x3 map; offset k (x fastest) has sum |d| = the number of its non-zero components
__device__ __forceinline__ int offset_norm1(int k)
{
    return (k % 3 != 1) + ((k / 3) % 3 != 1) + (k / 9 != 1);
}

__global__ __launch_bounds__(kBlock) void components_hook_kernel(const int32_t *__restrict__ nbr, const int32_t *__restrict__ keys,
                                                                 int32_t n, int max_norm1, int32_t *parent, int32_t *status)
{
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t key = keys ? keys[i] : 0;
    if (key < 0) return;
    for (int k = 0; k < 13; ++k) {
        if (offset_norm1(k) > max_norm1) continue;
        const int32_t j = nbr[(size_t)k * n + i];
        if (j < 0 || j >= n || j == i) continue;        // (j >= n, j == i: not a self map of distinct rows; nothing is indexed)
        if (keys && keys[j] != key) continue;
        int32_t a = i, b = j;
        bool done = false;
        for (int32_t tries = 0; tries <= n; ++tries) {
            if (!find_root(parent, a, n) || !find_root(parent, b, n)) {
                atomicOr(status, kStatusFindOverrun);
                return;
            }
            if (a == b) { done = true; break; }
            if (a < b) { const int32_t t = a; a = b; b = t; }
            int32_t expected = a;       // a > b: the larger root goes under the smaller
            if (__hip_atomic_compare_exchange_strong(parent + a, &expected, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) { done = true; break; }
            a = expected;               // somebody hooked a first: its new parent (< a) is where this link goes on
        }
        if (!done) {
            atomicOr(status, kStatusHookOverrun);
            return;
        }
    }
}

__global__ __launch_bounds__(kBlock) void components_flatten_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ keys,
                                                                    int32_t n, int32_t *label, int32_t *status)
{
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    if (keys && keys[i] < 0) {
        label[i] = -1;
        return;
    }
    int32_t x = i;
    for (int32_t step = 0; step <= n; ++step) {
        const int32_t p = parent[x];
        if (p == x) {
            label[i] = x;
            return;
        }
        x = p;
    }
    label[i] = x;
    atomicOr(status, kStatusFindOverrun);
}

size_t parent_bytes(int64_t n) { return align_up((size_t)(n > 0 ? n : 1) * sizeof(int32_t), 256); }

}  // namespace

extern "C" {

size_t eprecon_components_workspace_bytes(int64_t n) { return parent_bytes(n); }

int eprecon_components_async(const int32_t *nbr, int64_t n, const int32_t *keys, int connectivity, int32_t *label, int32_t *status,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || n > 0x7fffff00 || (connectivity != 6 && connectivity != 18 && connectivity != 26) || !status ||
        (n > 0 && (!nbr || !label || !workspace)))
        return EPRECON_ERR_ARG;
    if (n > 0 && workspace_bytes < parent_bytes(n)) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int32_t *parent = reinterpret_cast<int32_t *>(workspace);
    const unsigned blocks = (unsigned)ceil_div(n > 0 ? n : 1, kBlock);
    hipLaunchKernelGGL(components_init_kernel, dim3(blocks), dim3(kBlock), 0, st, parent, (int32_t)n, status);
    EP_LAUNCH_CHECK();
    if (n == 0) return EPRECON_OK;
    const int max_norm1 = connectivity == 6 ? 1 : connectivity == 18 ? 2 : 3;
    hipLaunchKernelGGL(components_hook_kernel, dim3(blocks), dim3(kBlock), 0, st, nbr, keys, (int32_t)n, max_norm1, parent, status);
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(components_flatten_kernel, dim3(blocks), dim3(kBlock), 0, st, parent, keys, (int32_t)n, label, status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
