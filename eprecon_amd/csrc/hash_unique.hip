// Coordinate bookkeeping for the sparse layers on gfx950: hash-grid build / query, unique
// voxel ids (stable, first-occurrence order) and their three-level hierarchy.  The maps over these tables are in kernel_map.hip,
// all but one: transpose_map_kernel stays in this unit, beside the other kernels that quantise with floor_div.  The compiler
// specialises that file-local helper by the call sites it sees in the unit (apart, the four kernels that call it under q > 1
// compile to other instructions), and this split moves kernels without changing their code.
//
// Replaces (reference call sites; implementations are in the un-vendored torchsparse / spconv):
//   F.sphash + F.sphashquery            ops/torchsparse_utils.py:19-21,44-50,73-79
//   torch.unique(hash) voxel ids        ops/torchsparse_utils.py:20-22   (initial_voxelize)
//   the transpose of spnn.Conv3d's k2 s2 kernel map (call sites: see kernel_map.hip)
// Ordering contract of this build (the reference's voxel order is "ascending hash", i.e. arbitrary
// and never relied on — SURVEY.md appendix A.2): unique voxels are numbered in order of FIRST
// OCCURRENCE in the input list.  All kernels are atomic-free in their outputs except the hash
// insert (atomicCAS on the key, atomicMin on the row index), whose result is order-independent.
#include "hashgrid.hpp"
#include "scan.hpp"

namespace {
using namespace ep;

__device__ __forceinline__ int floor_div(int a, int q) { return (a >= 0) ? a / q : -((-a + q - 1) / q); }

__global__ void hash_clear_kernel(unsigned long long *keys, int32_t *vals, uint32_t cap, int32_t *status)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < cap) {
        keys[i] = kEmptyKey;
        vals[i] = 0x7fffffff;
    }
    if (i == 0) status[0] = 0;
}

// coords int32[n,4] (b,x,y,z); key = floor(c / q) * q per spatial coordinate (q >= 1)
__global__ void hash_insert_kernel(HashTable t, const int4 *coords, int n, int q, int32_t *status, const int32_t *n_dev)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (i >= n) return;
    int4 c = coords[i];
    if (q > 1) {
        c.y = floor_div(c.y, q) * q;
        c.z = floor_div(c.z, q) * q;
        c.w = floor_div(c.w, q) * q;
    }
    if (!key_in_range(c.x, c.y, c.z, c.w)) {
        atomicOr(status, 1);
        return;
    }
    if (!hash_insert(t, pack_key(c.x, c.y, c.z, c.w), i)) atomicOr(status, 2);
}

__global__ void hash_query_kernel(HashTable t, const int4 *queries, int m, int q, int32_t *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    int4 c = queries[i];
    if (q > 1) {
        c.y = floor_div(c.y, q) * q;
        c.z = floor_div(c.z, q) * q;
        c.w = floor_div(c.w, q) * q;
    }
    out[i] = key_in_range(c.x, c.y, c.z, c.w) ? hash_lookup(t, pack_key(c.x, c.y, c.z, c.w)) : -1;
}

// first[i] = 1 when row i is the first occurrence of its (quantised) key
__global__ void first_flag_kernel(HashTable t, const int4 *coords, int n, int q, int32_t *first,
                                  int32_t *owner, const int32_t *n_dev)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (i >= n) return;
    int4 c = coords[i];
    if (q > 1) {
        c.y = floor_div(c.y, q) * q;
        c.z = floor_div(c.z, q) * q;
        c.w = floor_div(c.w, q) * q;
    }
    const int o = key_in_range(c.x, c.y, c.z, c.w) ? hash_lookup(t, pack_key(c.x, c.y, c.z, c.w)) : -1;
    owner[i] = o;
    first[i] = (o == i) ? 1 : 0;
}

// inverse[i] = unique id of row i; unique_coords[uid] = quantised coords of the first occurrence;
// the table values are rewritten from "first row" to "unique id" so later lookups return ids.
// (the launch also covers the table: thread s < cap rewrites slot s — table_vals_to_ids_kernel's job; the two halves touch
// disjoint data, so one launch serves both)
__global__ void unique_finalize_kernel(HashTable t, const int4 *coords, int n, int q,
                                       const int32_t *owner, const int32_t *rank, int32_t *inverse,
                                       int4 *unique_coords, const int32_t *n_dev, uint32_t cap, const int32_t *status,
                                       int32_t *status_copy)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && status_copy) *status_copy = *status;   // (the inserts finished a launch ago: the word is final)
    if ((uint32_t)i < cap && t.keys[i] != kEmptyKey) t.vals[i] = rank[t.vals[i]];
    if (n_dev) n = min(n, *n_dev);
    if (i >= n) return;
    const int o = owner[i];
    if (o < 0) {
        inverse[i] = -1;
        return;
    }
    const int uid = rank[o];
    inverse[i] = uid;
    if (o == i) {
        int4 c = coords[i];
        if (q > 1) {
            c.y = floor_div(c.y, q) * q;
            c.z = floor_div(c.z, q) * q;
            c.w = floor_div(c.w, q) * q;
        }
        unique_coords[uid] = c;
    }
}

// transposed k2s2 map: up[k][i] = parent row of fine voxel i when i is child k of its parent, else -1
__global__ void transpose_map_kernel(const int4 *fine, int n, const int32_t *parent, int fine_stride,
                                     int32_t *up)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int4 c = fine[i];
    const int q = 2 * fine_stride;
    const int bx = (c.y - floor_div(c.y, q) * q) / fine_stride;
    const int by = (c.z - floor_div(c.z, q) * q) / fine_stride;
    const int bz = (c.w - floor_div(c.w, q) * q) / fine_stride;
    const int kk = 4 * bx + 2 * by + bz;
    const int par = parent[i];
    for (int k = 0; k < 8; ++k) up[(size_t)k * n + i] = (k == kk) ? par : -1;
}

__global__ void gather_headers_kernel(const int32_t *t0, const int32_t *t1, const int32_t *t2, int levels, int32_t *out)
{
    const int i = threadIdx.x;      // (status, count) of every level's table, side by side: ONE device -> host read later
    if (i < 2 * levels) out[i] = (i < 2 ? t0 : i < 4 ? t1 : t2)[i & 1];
}

// clear (unless the caller did) and insert: the shared builder of the hash and unique entry points
// (cleared: the caller reset the table with its other regions, ep::multi_fill + ep::table_clear_regions)
int hash_build_impl(const int32_t *coords, int64_t n, const int32_t *n_dev, int quantum, void *table, uint32_t capacity,
                    void *stream, bool cleared)
{
    if (!table || !table_capacity_ok(capacity) || n < 0 || quantum < 1 || (uint64_t)capacity < (uint64_t)n + 1 ||
        (n > 0 && !coords))
        return EPRECON_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HashTable t = make_table(table, capacity);
    if (!cleared) {
        hipLaunchKernelGGL(hash_clear_kernel, dim3((capacity + 255) / 256), dim3(256), 0, st, t.keys, t.vals,
                           capacity, table_status(table));
        EP_LAUNCH_CHECK();
    }
    if (n > 0) {
        hipLaunchKernelGGL(hash_insert_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, t,
                           reinterpret_cast<const int4 *>(coords), (int)n, quantum, table_status(table), n_dev);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}
}  // namespace

namespace ep {
int table_clear_regions(void *table, uint32_t capacity, FillRegion *out3)
{
    if (!table || !table_capacity_ok(capacity)) return EPRECON_ERR_ARG;
    HashTable t = make_table(table, capacity);
    out3[0] = FillRegion{table, 16, 0u};                                          // status word (and the unique count next to it)
    out3[1] = FillRegion{t.keys, (size_t)capacity * 8, 0xFFFFFFFFu};              // kEmptyKey
    out3[2] = FillRegion{t.vals, (size_t)capacity * 4, 0x7fffffffu};
    return EPRECON_OK;
}

int unique_coords_dn(const int32_t *coords, int64_t n, const int32_t *n_dev, int quantum, void *table, uint32_t capacity,
                     int32_t *inverse, int32_t *unique_coords, int32_t *n_unique_dev, void *workspace, size_t workspace_bytes,
                     bool table_cleared, int32_t *status_copy, void *stream)
{
    if (!n_unique_dev || !workspace || workspace_bytes < eprecon_unique_workspace_bytes(n))
        return n_unique_dev && workspace ? EPRECON_ERR_WORKSPACE : EPRECON_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    int rc = hash_build_impl(coords, n, n_dev, quantum, table, capacity, stream, table_cleared);
    if (rc != EPRECON_OK) return rc;
    if (n == 0) {
        EP_HIP_CHECK(hipMemsetAsync(n_unique_dev, 0, sizeof(int32_t), st));
        if (status_copy) EP_HIP_CHECK(hipMemsetAsync(status_copy, 0, sizeof(int32_t), st));
        return EPRECON_OK;
    }
    if (!inverse || !unique_coords) return EPRECON_ERR_ARG;
    char *ws = reinterpret_cast<char *>(workspace);
    const size_t seg = align_up((size_t)n * 4, 256);
    int32_t *first = reinterpret_cast<int32_t *>(ws);
    int32_t *owner = reinterpret_cast<int32_t *>(ws + seg);
    int32_t *rank = reinterpret_cast<int32_t *>(ws + 2 * seg);
    int32_t *scratch = reinterpret_cast<int32_t *>(ws + 3 * seg);
    HashTable t = make_table(table, capacity);
    const dim3 grid((unsigned)ceil_div(n, 256)), block(256);
    const int4 *c4 = reinterpret_cast<const int4 *>(coords);
    hipLaunchKernelGGL(first_flag_kernel, grid, block, 0, st, t, c4, (int)n, quantum, first, owner, n_dev);
    EP_LAUNCH_CHECK();
    rc = exclusive_scan_i32_dn(first, (int)n, n_dev, rank, scratch, n_unique_dev, st);
    if (rc != EPRECON_OK) return rc;
    const int64_t span = n > (int64_t)capacity ? n : (int64_t)capacity;
    hipLaunchKernelGGL(unique_finalize_kernel, dim3((unsigned)ceil_div(span, 256)), block, 0, st, t, c4, (int)n, quantum, owner, rank,
                       inverse, reinterpret_cast<int4 *>(unique_coords), n_dev, capacity, (const int32_t *)table_status(table),
                       status_copy);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
}  // namespace ep

extern "C" {

uint32_t eprecon_hash_capacity(int64_t n) { return ep::hash_capacity_for(n); }
size_t eprecon_hash_table_bytes(uint32_t capacity) { return ep::table_bytes(capacity); }

int eprecon_hash_build_async(const int32_t *coords, int64_t n, int quantum, void *table,
                             uint32_t capacity, void *stream)
{
    return hash_build_impl(coords, n, nullptr, quantum, table, capacity, stream, false);
}

int eprecon_hash_build_dn_async(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, int quantum, void *table,
                                uint32_t capacity, void *stream)
{
    if (!n_dev) return EPRECON_ERR_ARG;
    return hash_build_impl(coords, n_cap, n_dev, quantum, table, capacity, stream, false);
}

int eprecon_hash_query_async(const void *table, uint32_t capacity, const int32_t *queries, int64_t m,
                             int quantum, int32_t *out_index, void *stream)
{
    if (!table || !table_capacity_ok(capacity) || m < 0 || quantum < 1 || (m > 0 && (!queries || !out_index)))
        return EPRECON_ERR_ARG;
    if (m == 0) return EPRECON_OK;
    HashTable t = make_table(table, capacity);
    hipLaunchKernelGGL(hash_query_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0,
                       (hipStream_t)stream, t, reinterpret_cast<const int4 *>(queries), (int)m, quantum,
                       out_index);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_hash_status(const void *table, void *stream)
{
    int32_t s = 0;
    EP_HIP_CHECK(hipMemcpyAsync(&s, table, sizeof(s), hipMemcpyDeviceToHost, (hipStream_t)stream));
    EP_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    return s == 0 ? EPRECON_OK : (s & 1 ? EPRECON_ERR_UNSUPPORTED : EPRECON_ERR_WORKSPACE);
}

// [first | owner | rank | scan scratch | slack], each a 256-byte aligned segment
size_t eprecon_unique_workspace_bytes(int64_t n)
{
    n = n > 0 ? n : 1;
    return align_up((size_t)n * 4, 256) * 3 + scan_scratch_bytes(n) + 256;
}

int eprecon_unique_coords_async(const int32_t *coords, int64_t n, int quantum, void *table,
                                uint32_t capacity, int32_t *inverse, int32_t *unique_coords,
                                int32_t *n_unique_dev, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    return ep::unique_coords_dn(coords, n, nullptr, quantum, table, capacity, inverse, unique_coords, n_unique_dev, workspace,
                                workspace_bytes, false, nullptr, stream);
}

int eprecon_unique_coords_dn_async(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, int quantum, void *table,
                                   uint32_t capacity, int32_t *inverse, int32_t *unique_coords, int32_t *n_unique_dev,
                                   void *workspace, size_t workspace_bytes, void *stream)
{
    if (!n_dev) return EPRECON_ERR_ARG;
    return ep::unique_coords_dn(coords, n_cap, n_dev, quantum, table, capacity, inverse, unique_coords, n_unique_dev, workspace,
                                workspace_bytes, false, nullptr, stream);
}

int eprecon_unique_hierarchy_dn_async(const int32_t *coords, int64_t n_cap, const int32_t *n_dev, int levels, void *const *tables,
                                      const uint32_t *capacities, int32_t *const *inverse, int32_t *const *unique_coords,
                                      int32_t *summary, void *workspace, size_t workspace_bytes, void *stream)
{
    if (levels < 1 || levels > 3 || !tables || !capacities || !inverse || !unique_coords || n_cap < 0) return EPRECON_ERR_ARG;
    ep::FillRegion reg[9];
    for (int l = 0; l < levels; ++l) {
        const int rc = ep::table_clear_regions(tables[l], capacities[l], reg + 3 * l);
        if (rc != EPRECON_OK) return rc;
    }
    int rc = ep::multi_fill(reg, 3 * levels, (hipStream_t)stream);     // ONE launch resets the tables of all strides
    if (rc != EPRECON_OK) return rc;
    const int32_t *src = coords, *live = n_dev;
    for (int l = 0; l < levels; ++l) {
        int32_t *count = reinterpret_cast<int32_t *>(tables[l]) + 1;       // next to the table's status word: one 8-byte read per stride
        rc = ep::unique_coords_dn(src, n_cap, live, 1 << l, tables[l], capacities[l], inverse[l], unique_coords[l], count, workspace,
                                  workspace_bytes, true, nullptr, stream);
        if (rc != EPRECON_OK) return rc;
        src = unique_coords[l];
        live = count;
    }
    if (summary) {
        hipLaunchKernelGGL(gather_headers_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int32_t *)tables[0],
                           (const int32_t *)tables[levels > 1 ? 1 : 0], (const int32_t *)tables[levels > 2 ? 2 : 0], levels, summary);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

int eprecon_transpose_map_async(const int32_t *fine_coords, int64_t n, const int32_t *parent,
                                int fine_stride, int32_t *up_map, void *stream)
{
    if (n < 0 || fine_stride < 1 || (n > 0 && (!fine_coords || !parent || !up_map))) return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    hipLaunchKernelGGL(transpose_map_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const int4 *>(fine_coords), (int)n, parent,
                       fine_stride, up_map);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
