// Open-addressing hash grid over packed voxel keys (device side), shared by the kernel-map,
// voxelise / devoxelise and union kernels.
//
// Replaces torchsparse's F.sphash / F.sphashquery (call sites ops/torchsparse_utils.py:19-21,44-50,
// 73-79 of the reference) and the coordinate bookkeeping spconv does internally.  The hash value
// never leaves the library, so any collision-free key works: a key is the
// exact 64-bit packing of (batch, x, y, z), the table stores the key itself, and a lookup compares
// keys — there are no false positives.
//
//   key  = batch[4 bits] | (x + 2^19)[20] | (y + 2^19)[20] | (z + 2^19)[20]
//   slot = mix64(key) & (capacity - 1), linear probing, capacity = power of two >= 2 * n
//   value = smallest row index that inserted the key (atomicMin) -> duplicates collapse
//           deterministically onto their first occurrence.
//
// A table's memory (table_bytes): a 256-byte header whose first int32 is the status word (bit 0: a key out of range, bit 1:
// table full; the unique hierarchy keeps the level's count in the int32 behind it), then `capacity` 8-byte keys, then
// `capacity` int32 values.  make_table / table_status are the one place that spells this out.
#pragma once

#include "common.hpp"

namespace ep {

constexpr unsigned long long kEmptyKey = 0xFFFFFFFFFFFFFFFFull;
constexpr int kCoordBias = 1 << 19;
constexpr int kCoordLimit = (1 << 19) - 1;  // |coordinate| must stay below this
constexpr int kMaxBatch = 14;               // batch 15 is reserved (all-ones key = empty slot)

struct HashTable {
    unsigned long long *keys;  // [capacity]
    int32_t *vals;             // [capacity]
    uint32_t mask;             // capacity - 1
};

__host__ __device__ __forceinline__ bool key_in_range(int b, int x, int y, int z)
{
    return b >= 0 && b <= kMaxBatch && x > -kCoordLimit && x < kCoordLimit && y > -kCoordLimit &&
           y < kCoordLimit && z > -kCoordLimit && z < kCoordLimit;
}

__host__ __device__ __forceinline__ unsigned long long pack_key(int b, int x, int y, int z)
{
    return ((unsigned long long)(unsigned)b << 60) |
           ((unsigned long long)(unsigned)(x + kCoordBias) << 40) |
           ((unsigned long long)(unsigned)(y + kCoordBias) << 20) |
           (unsigned long long)(unsigned)(z + kCoordBias);
}

__device__ __forceinline__ uint32_t hash_slot(unsigned long long k, uint32_t mask)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)k & mask;
}

// insert (key -> min(row)); returns false if the probe sequence wrapped (table full)
__device__ __forceinline__ bool hash_insert(const HashTable &t, unsigned long long key, int row)
{
    uint32_t s = hash_slot(key, t.mask);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long prev = atomicCAS(&t.keys[s], kEmptyKey, key);
        if (prev == kEmptyKey || prev == key) {
            atomicMin(&t.vals[s], row);
            return true;
        }
        s = (s + 1) & t.mask;
    }
    return false;
}

// lookup after the build kernel has completed (kernel boundary = visibility); -1 when absent
__device__ __forceinline__ int hash_lookup(const HashTable &t, unsigned long long key)
{
    uint32_t s = hash_slot(key, t.mask);
    for (uint32_t probe = 0; probe <= t.mask; ++probe) {
        const unsigned long long k = t.keys[s];
        if (k == key) return t.vals[s];
        if (k == kEmptyKey) return -1;
        s = (s + 1) & t.mask;
    }
    return -1;
}

constexpr size_t kTableHeaderBytes = 256;
static inline size_t table_bytes(uint32_t capacity) { return kTableHeaderBytes + (size_t)capacity * 12; }
// a power of two, at least 1024
static inline bool table_capacity_ok(uint32_t c) { return c >= 1024 && (c & (c - 1)) == 0; }
static inline HashTable make_table(const void *mem, uint32_t capacity)
{
    HashTable t;
    t.keys = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(const_cast<void *>(mem)) + kTableHeaderBytes);
    t.vals = reinterpret_cast<int32_t *>(t.keys + capacity);
    t.mask = capacity - 1;
    return t;
}
static inline int32_t *table_status(const void *mem) { return reinterpret_cast<int32_t *>(const_cast<void *>(mem)); }

static inline uint32_t hash_capacity_for(int64_t n)
{
    uint64_t c = 1024;
    while (c < (uint64_t)(2 * n + 1)) c <<= 1;
    return (uint32_t)c;
}


// the three regions that reset a table (header, keys = empty, values = int max) for ep::multi_fill: hash_unique.hip
int table_clear_regions(void *table, uint32_t capacity, FillRegion *out3);

// Unique voxel ids in first-occurrence order (hash_unique.hip): the body of eprecon_unique_coords_async / _dn_async.  n_dev
// (optional, device): the live length is min(n_cap, *n_dev).  table_cleared: the caller reset the table itself (multi_fill);
// status_copy (optional device int32): receives the table's status word from the call's last launch
int unique_coords_dn(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, int quantum, void *table, uint32_t capacity,
                     int32_t *inverse, int32_t *unique_coords, int32_t *n_unique_dev, void *workspace, size_t workspace_bytes,
                     bool table_cleared, int32_t *status_copy, void *stream);

// The 3x3x3 map of a voxel set against its own table (kernel_map.hip): the body of eprecon_kernel_map_self_async.  prefilled: the
// caller filled the map's upper half (offsets 14 .. 26) with -1 itself — the region kernel_map_self_fill_region names, typically
// inside a multi_fill that resets other things too
FillRegion kernel_map_self_fill_region(int32_t *nbr, int64_t n);
int kernel_map_self(const void *table, uint32_t capacity, const int32_t *coords, int64_t n, int stride, int32_t *nbr, bool prefilled,
                    void *stream);

}  // namespace ep
