// Distance field of a sparse TSDF scene on gfx950: the exact squared Euclidean distance from every cell of a box to the nearest
// surface sample of the scene, and which row that sample is (DESIGN.md §5b "distance field"; the caller is
// eprecon_amd/distance_field.py).  The reference has no such product: the rule is this project's.
//
//   inside  a row with tsdf <= 0; a coordinate that is no row is outside (it reads 1, as in tsdf_raycast.hip); of rows that
//           repeat a coordinate the first counts.
//   site    a (first) row with a 6-neighbour coordinate whose inside-state differs from its own.
//   answer  dist2(x) = min over the sites s inside the box of |x - s|^2, site(x) = the smallest row among those that attain it;
//           beyond radius^2: dist2 = INT_MAX, site = -1.  state(x) = 0 no row, 1 an outside row, 2 an inside row.
//
// Everything is an integer.  The working volume holds 64-bit keys (d2 << 32) | row, INT_MAX in both halves where nothing is
// known, and the minimum over the packed key IS the rule: smallest d2 first, smallest row among equals.  Launches, whatever the
// rows look like:
//
//   clear   the row table, the status word, the working volume (far) and `state` (0); with m == 0 also the outputs, and
//           nothing follows.
//   insert  one launch over the rows: row key -> smallest row (hashgrid.hpp).
//   seed    one launch over the rows: a first row looks its six neighbours up, writes its state and, when it is a site inside
//           the box, the key (0 << 32) | row into its cell.  Only the first row of a coordinate writes: plain stores.
//   z, y, x three band-minimum passes, out[i] = min over |i - j| <= R of (in[j].d2 + (i - j)^2, in[j].row).  A constant added to
//           a whole line keeps the order of its keys, so the minimum over the packed key composes across the passes into the
//           lexicographic minimum over the box-shaped neighbourhood, which contains every site within R.  Each lane scans
//           outward from its own cell, k = 0, 1, ..., and stops once k^2 > best.d2 (not at >=: a tie may still bring a smaller
//           row), so a cell near the surface costs a handful of reads whatever R is.
//             z   the scanned axis is the contiguous one: a wave owns 64 cells of one line, stages them with their halo
//                 (clipped to the line: at most 1024 keys) in its own stretch of LDS by coalesced reads, and scans there;
//                 consecutive lanes read consecutive 8-byte words at every step, which is conflict-free.
//             y,x the lanes run along the contiguous axis (z; in the x pass along the whole y-z plane), so every step of the
//                 scan is one contiguous 512-byte read per wave.  The x pass splits the key into dist2 and site and applies
//                 the R^2 cut.
//
// No atomics outside insert (and the status word), no workgroup waits on another, no scratch.  The outputs are a function of
// the rows and the box alone: bit-identical from run to run.
#include "hashgrid.hpp"

namespace {
using namespace ep;

constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / kWave;
constexpr int kMaxExtent = 1 << 10;           // per axis: d2 <= 3 * 1023^2 stays far from 2^31
constexpr int kStatusKeyRange = 1;            // a row (or a neighbour the seed would look up) outside the key range
constexpr int kStatusTableFull = 2;           // a probe sequence wrapped
constexpr int32_t kFar = 0x7fffffff;
constexpr unsigned long long kFarKey = 0x7fffffff7fffffffull;

struct Box {
    int lo[3], n[3];        // n: the extents X, Y, Z
};

struct Layout {
    uint32_t capacity;
    size_t table, vol_a, vol_b, total;
};

bool box_ok(const int32_t lo[3], const int32_t hi[3])
{
    if (!lo || !hi) return false;
    for (int k = 0; k < 3; ++k)
        if (hi[k] <= lo[k] || (int64_t)hi[k] - lo[k] > kMaxExtent) return false;
    return true;
}

Layout layout_for(int64_t m, int64_t cells)
{
    Layout L;
    L.capacity = hash_capacity_for(m > 0 ? m : 0);
    L.table = 0;
    L.vol_a = align_up(table_bytes(L.capacity), 256);
    L.vol_b = L.vol_a + align_up((size_t)cells * 8, 256);
    L.total = L.vol_b + align_up((size_t)cells * 8, 256);
    return L;
}

__global__ __launch_bounds__(kBlock) void df_clear_kernel(HashTable rows, unsigned long long *__restrict__ vol, uint8_t *__restrict__ state,
                                                          int32_t *__restrict__ dist2, int32_t *__restrict__ site, int64_t cells,
                                                          int outputs, int32_t *status)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i <= (int64_t)rows.mask) {
        rows.keys[i] = kEmptyKey;
        rows.vals[i] = kFar;
    }
    if (i < cells) {
        state[i] = 0;
        if (outputs) {
            dist2[i] = kFar;
            site[i] = -1;
        } else {
            vol[i] = kFarKey;
        }
    }
    if (i == 0) *status = 0;
}

__device__ __forceinline__ bool row_in_range(int x, int y, int z)
{
    // the seed looks c - 1 .. c + 1 up: all of them must be keys
    return key_in_range(0, x - 1, y - 1, z - 1) && key_in_range(0, x + 1, y + 1, z + 1);
}

__global__ __launch_bounds__(kBlock) void df_insert_kernel(HashTable rows, const int32_t *__restrict__ coords, int32_t m, int32_t *status)
{
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int x = coords[3 * (size_t)i], y = coords[3 * (size_t)i + 1], z = coords[3 * (size_t)i + 2];
    if (!row_in_range(x, y, z)) atomicOr(status, kStatusKeyRange);
    else if (!hash_insert(rows, pack_key(0, x, y, z), i)) atomicOr(status, kStatusTableFull);
}

__device__ __forceinline__ bool inside_at(const HashTable &rows, const float *__restrict__ tsdf, int x, int y, int z)
{
    const int r = hash_lookup(rows, pack_key(0, x, y, z));
    return r >= 0 && tsdf[r] <= 0.0f;
}

__global__ __launch_bounds__(kBlock) void df_seed_kernel(HashTable rows, const int32_t *__restrict__ coords, const float *__restrict__ tsdf,
                                                         int32_t m, Box box, unsigned long long *__restrict__ vol,
                                                         uint8_t *__restrict__ state)
{
    const int32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= m) return;
    const int x = coords[3 * (size_t)i], y = coords[3 * (size_t)i + 1], z = coords[3 * (size_t)i + 2];
    const int cx = x - box.lo[0], cy = y - box.lo[1], cz = z - box.lo[2];
    if (cx < 0 || cx >= box.n[0] || cy < 0 || cy >= box.n[1] || cz < 0 || cz >= box.n[2]) return;    // only sites inside the box count
    if (!row_in_range(x, y, z)) return;
    if (hash_lookup(rows, pack_key(0, x, y, z)) != i) return;       // a later row of a repeated coordinate
    const bool in = tsdf[i] <= 0.0f;
    const bool differs = inside_at(rows, tsdf, x - 1, y, z) != in || inside_at(rows, tsdf, x + 1, y, z) != in ||
                         inside_at(rows, tsdf, x, y - 1, z) != in || inside_at(rows, tsdf, x, y + 1, z) != in ||
                         inside_at(rows, tsdf, x, y, z - 1) != in || inside_at(rows, tsdf, x, y, z + 1) != in;
    const size_t cell = ((size_t)cx * box.n[1] + cy) * box.n[2] + cz;
    state[cell] = in ? 2 : 1;
    if (differs) vol[cell] = (unsigned long long)(uint32_t)i;
}

__device__ __forceinline__ unsigned long long shifted(unsigned long long key, int k)
{
    return key + ((unsigned long long)(uint32_t)(k * k) << 32);
}

// the z pass: lines of nz keys, contiguous; a wave owns the cells [z0, z0 + 64) of one line and the window of the line within
// `reach` of them, staged in its `window` keys of LDS (window >= min(nz, 64 + 2 reach))
__global__ __launch_bounds__(kBlock) void df_pass_z_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out,
                                                           int64_t lines, int nz, int reach, int window)
{
    extern __shared__ __align__(16) unsigned long long staged[];
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x / kWave;
    const int chunks = (nz + kWave - 1) / kWave;
    const int64_t wave = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * kWavesPerBlock + wid;
    const bool live = wave < lines * chunks;
    const int64_t line = live ? wave / chunks : 0;
    const int z0 = live ? (int)(wave - line * chunks) * kWave : 0;
    const int wlo = z0 - reach > 0 ? z0 - reach : 0, whi = z0 + kWave + reach < nz ? z0 + kWave + reach : nz;
    unsigned long long *mine = staged + (size_t)wid * window;
    bool any = false;
    if (live) {
        const unsigned long long *src = in + line * nz;
        for (int j = wlo + lane; j < whi; j += kWave) {
            const unsigned long long key = src[j];
            mine[j - wlo] = key;
            any = any || key != kFarKey;
        }
    }
    __syncthreads();
    const bool some = __any(any);           // (every lane of the wave is still here: a lane past the line's end staged too)
    const int i = z0 + lane;
    if (!live || i >= nz) return;
    unsigned long long best = kFarKey;
    if (some) {
        best = mine[i - wlo];
        for (int k = 1; k <= reach && (unsigned long long)(uint32_t)(k * k) <= (best >> 32); ++k) {
            if (i - k >= wlo) {
                const unsigned long long key = mine[i - k - wlo];
                if (key != kFarKey && shifted(key, k) < best) best = shifted(key, k);
            }
            if (i + k < whi) {
                const unsigned long long key = mine[i + k - wlo];
                if (key != kFarKey && shifted(key, k) < best) best = shifted(key, k);
            }
        }
    }
    out[line * nz + i] = best;
}

// the y and x passes on the volume seen as [outer][n][len]: the scanned axis has stride `len`, the lanes run along `len`.  A
// wave owns 64 consecutive lane cells of one (outer, i); the four waves of a block own four consecutive i of the same lane
// cells, so that the lines they read overlap, and an XCD gets one contiguous range of blocks (xcd_remap: its L2 sees the
// overlap of neighbouring blocks too).  kLast: split the key and apply the cut.
template <bool kLast>
__global__ __launch_bounds__(kBlock) void df_pass_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out,
                                                         int32_t *__restrict__ dist2, int32_t *__restrict__ site, int64_t outer, int n,
                                                         int64_t len, int reach, long long cut)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t chunks = (len + kWave - 1) / kWave;
    const int64_t wave = (int64_t)xcd_remap(blockIdx.x, gridDim.x) * kWavesPerBlock + threadIdx.x / kWave;
    if (wave >= outer * chunks * n) return;
    const int i = (int)(wave % n);
    const int64_t rest = wave / n, chunk = rest % chunks, o = rest / chunks;
    const int64_t l = chunk * kWave + lane;
    if (l >= len) return;
    const unsigned long long *src = in + o * n * len + l;
    unsigned long long best = src[(int64_t)i * len];
    for (int k = 1; k <= reach && (unsigned long long)(uint32_t)(k * k) <= (best >> 32); ++k) {
        if (i - k >= 0) {
            const unsigned long long key = src[(int64_t)(i - k) * len];
            if (key != kFarKey && shifted(key, k) < best) best = shifted(key, k);
        }
        if (i + k < n) {
            const unsigned long long key = src[(int64_t)(i + k) * len];
            if (key != kFarKey && shifted(key, k) < best) best = shifted(key, k);
        }
    }
    const int64_t at = (o * n + i) * len + l;
    if (kLast) {
        const bool far = best == kFarKey || (long long)(best >> 32) > cut;
        dist2[at] = far ? kFar : (int32_t)(best >> 32);
        site[at] = far ? -1 : (int32_t)(uint32_t)best;
    } else {
        out[at] = best;
    }
}

}  // namespace

extern "C" {

size_t eprecon_distance_field_workspace_bytes(int64_t m, const int32_t lo[3], const int32_t hi[3])
{
    if (m < 0 || !box_ok(lo, hi)) return 0;
    return layout_for(m, (int64_t)(hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])).total;
}

int eprecon_distance_field_async(const int32_t *coords, const float *tsdf, int64_t m, const int32_t lo[3], const int32_t hi[3],
                                 int radius, int32_t *dist2, int32_t *site, uint8_t *state, int32_t *status, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (m < 0 || m > 0x07ffffffll || !box_ok(lo, hi) || radius < 0 || !dist2 || !site || !state || !status || !workspace ||
        (m > 0 && (!coords || !tsdf)))
        return EPRECON_ERR_ARG;
    Box box;
    for (int k = 0; k < 3; ++k) {
        box.lo[k] = lo[k];
        box.n[k] = hi[k] - lo[k];
    }
    const int64_t cells = (int64_t)box.n[0] * box.n[1] * box.n[2];
    const Layout L = layout_for(m, cells);
    if (workspace_bytes < L.total) return EPRECON_ERR_ARG;
    char *w = reinterpret_cast<char *>(workspace);
    const HashTable rows = make_table(w + L.table, L.capacity);
    unsigned long long *vol_a = reinterpret_cast<unsigned long long *>(w + L.vol_a);
    unsigned long long *vol_b = reinterpret_cast<unsigned long long *>(w + L.vol_b);
    hipStream_t st = (hipStream_t)stream;

    const int64_t span = cells > (int64_t)L.capacity ? cells : (int64_t)L.capacity;
    hipLaunchKernelGGL(df_clear_kernel, dim3((unsigned)ceil_div(span, kBlock)), dim3(kBlock), 0, st, rows, vol_a, state, dist2, site,
                       cells, m == 0 ? 1 : 0, status);
    EP_LAUNCH_CHECK();
    if (m == 0) return EPRECON_OK;
    const dim3 row_blocks((unsigned)ceil_div(m, kBlock));
    hipLaunchKernelGGL(df_insert_kernel, row_blocks, dim3(kBlock), 0, st, rows, coords, (int32_t)m, status);
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(df_seed_kernel, row_blocks, dim3(kBlock), 0, st, rows, coords, tsdf, (int32_t)m, box, vol_a, state);
    EP_LAUNCH_CHECK();

    const int nx = box.n[0], ny = box.n[1], nz = box.n[2];
    const long long cut = (long long)radius * radius;     // (radius < 2^31: no overflow in 64 bits)
    {
        const int reach = radius < nz - 1 ? radius : nz - 1;
        const int window = nz < kWave + 2 * reach ? nz : kWave + 2 * reach;
        const int64_t waves = (int64_t)nx * ny * ceil_div(nz, kWave);
        hipLaunchKernelGGL(df_pass_z_kernel, dim3((unsigned)ceil_div(waves, kWavesPerBlock)), dim3(kBlock),
                           (size_t)kWavesPerBlock * window * 8, st, vol_a, vol_b, (int64_t)nx * ny, nz, reach, window);
        EP_LAUNCH_CHECK();
    }
    {
        const int64_t waves = (int64_t)nx * ceil_div(nz, kWave) * ny;
        hipLaunchKernelGGL(df_pass_kernel<false>, dim3((unsigned)ceil_div(waves, kWavesPerBlock)), dim3(kBlock), 0, st, vol_b, vol_a,
                           (int32_t *)nullptr, (int32_t *)nullptr, (int64_t)nx, ny, (int64_t)nz, radius < ny - 1 ? radius : ny - 1, cut);
        EP_LAUNCH_CHECK();
    }
    {
        const int64_t plane = (int64_t)ny * nz, waves = ceil_div(plane, kWave) * nx;
        hipLaunchKernelGGL(df_pass_kernel<true>, dim3((unsigned)ceil_div(waves, kWavesPerBlock)), dim3(kBlock), 0, st, vol_a,
                           (unsigned long long *)nullptr, dist2, site, (int64_t)1, nx, plane, radius < nx - 1 ? radius : nx - 1, cut);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

}  // extern "C"
