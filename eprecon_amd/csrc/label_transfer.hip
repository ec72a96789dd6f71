// Panoptic export (tools/generate_semantic_instance.py of the reference): every mesh vertex takes the labels of the nearest
// labelled voxel.  The sites are cells of a dense volume that is already on the device, so there is no cloud, no sort and no
// float copy of the sites: one 64-bit occupancy word per 4x4x4 brick, and a search over shells of bricks whose site
// coordinates are recomputed in fp64 from the cell index exactly as numpy computes `idx * voxel_size + origin`.
//
// Exactness: the winner is the minimum of (d2, linear index) over ALL sites.  Every pruning bound (a brick's box, the
// unvisited slabs) is evaluated with the same rounded operations as d2 itself on per-axis offsets that are no larger than any
// site's inside the box; rounded multiplication and addition are monotonic, so a bound never exceeds the d2 of a site it
// covers, and both comparisons are strict.  The thread form and the wave form therefore agree bit for bit.
#include <algorithm>

#include "common.hpp"

namespace {

using namespace ep;

constexpr int kMaxMap = 256;

// the search itself is plain C++ (host and device): a host program can walk it against a brute force without a GPU
#define LT_HD __host__ __device__ __forceinline__

struct LtMap {
    int32_t v[kMaxMap];
    int n;
};

struct LtGrid {
    double o[3], vs;      // fl64(origin_f32), voxel size
    int dims[3], nb[3];   // cells, bricks
};

LT_HD double lt_site(const LtGrid &G, int i, int a) { return (double)i * G.vs + G.o[a]; }

// (the library is built with -ffp-contract=off: every product and sum below is rounded on its own)
LT_HD double lt_d2(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

// distance of q to the interval [site(i0), site(i1)] on axis a
LT_HD double lt_gap(const LtGrid &G, double q, int i0, int i1, int a)
{
    const double lo = lt_site(G, i0, a), hi = lt_site(G, i1, a);
    return q < lo ? lo - q : (q > hi ? q - hi : 0.0);
}

LT_HD int lt_cell(const LtGrid &G, double q, int a)
{
    const double f = floor((q - G.o[a]) / G.vs);
    return (int)fmin(fmax(f, 0.0), (double)(G.dims[a] - 1));
}

// ---------------------------------------------------------------------------------------------------- brick masks

__global__ __launch_bounds__(256) void lt_brick_mask_kernel(LtMap M, LtGrid G, const int32_t *semantic, int64_t n_bricks,
                                                            unsigned long long *masks, int32_t *status)
{
    __shared__ int32_t s_map[kMaxMap];
    s_map[threadIdx.x] = (int)threadIdx.x < M.n ? M.v[threadIdx.x] : 0;
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t brick = (int64_t)blockIdx.x * 4 + threadIdx.x / kWave;
    if (brick >= n_bricks) return;
    const int bz = (int)(brick % G.nb[2]), by = (int)(brick / G.nb[2] % G.nb[1]), bx = (int)(brick / G.nb[2] / G.nb[1]);
    const int x = 4 * bx + (lane >> 4), y = 4 * by + ((lane >> 2) & 3), z = 4 * bz + (lane & 3);
    bool site = false, bad = false;
    if (x < G.dims[0] && y < G.dims[1] && z < G.dims[2]) {
        const int32_t s = semantic[((int64_t)x * G.dims[1] + y) * G.dims[2] + z];
        bad = s < 0 || s >= M.n;
        site = !bad && s_map[s] != 0;
    }
    const unsigned long long word = __ballot(site), any_bad = __ballot(bad);
    if (lane == 0) {
        masks[brick] = word;
        if (word) atomicAdd(&status[1], __popcll(word));
        if (any_bad) atomicOr(&status[0], 1);
    }
}

// ---------------------------------------------------------------------------------------------------------- query

struct LtQuery {
    double q[3];
    int b[3];      // brick of the clamped cell
    int rmax;
};

LT_HD LtQuery lt_query_of(const LtGrid &G, const float *p)
{
    LtQuery Q;
    int rmax = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Q.q[a] = (double)p[a];
        Q.b[a] = lt_cell(G, Q.q[a], a) >> 2;
        rmax = max(rmax, max(Q.b[a], G.nb[a] - 1 - Q.b[a]));
    }
    Q.rmax = rmax;
    return Q;
}

// Shell r of bricks around Q.b, clipped to the grid, as six disjoint rectangles: the two x faces over the whole clipped
// (y, z) range, the two y faces over the inner x range, the two z faces over the inner x and y ranges.
struct LtShell {
    int lo[3], n_full[3];     // clipped [b - r, b + r]
    int ilo[3], n_in[3];      // clipped [b - r + 1, b + r - 1]
    int n[6], total;
};

LT_HD LtShell lt_shell_of(const LtGrid &G, const LtQuery &Q, int r)
{
    LtShell S;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        S.lo[a] = max(Q.b[a] - r, 0);
        S.n_full[a] = min(Q.b[a] + r, G.nb[a] - 1) - S.lo[a] + 1;
        S.ilo[a] = max(Q.b[a] - r + 1, 0);
        S.n_in[a] = max(min(Q.b[a] + r - 1, G.nb[a] - 1) - S.ilo[a] + 1, 0);
    }
    const int area[3] = {S.n_full[1] * S.n_full[2], S.n_in[0] * S.n_full[2], S.n_in[0] * S.n_in[1]};
    S.total = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        S.n[2 * a] = Q.b[a] - r >= 0 ? area[a] : 0;
        S.n[2 * a + 1] = (r > 0 && Q.b[a] + r < G.nb[a]) ? area[a] : 0;
        S.total += S.n[2 * a] + S.n[2 * a + 1];
    }
    return S;
}

// brick number t (0 <= t < S.total) of the shell
LT_HD void lt_shell_brick(const LtShell &S, const LtQuery &Q, int r, int t, int &bx, int &by, int &bz)
{
    int f = 5;
#pragma unroll
    for (int k = 4; k >= 0; --k) {      // the face t falls in: the first k with t < n[0] + ... + n[k]
        int before = 0;
#pragma unroll
        for (int j = 0; j <= k; ++j) before += S.n[j];
        if (t < before) f = k;
    }
    int base = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) base += j < f ? S.n[j] : 0;
    t -= base;
    const int a = f >> 1, fixed = (f & 1) ? r : -r;
    if (a == 0) {
        const int u = t / S.n_full[2];
        bx = Q.b[0] + fixed, by = S.lo[1] + u, bz = S.lo[2] + (t - u * S.n_full[2]);
    } else if (a == 1) {
        const int u = t / S.n_full[2];
        bx = S.ilo[0] + u, by = Q.b[1] + fixed, bz = S.lo[2] + (t - u * S.n_full[2]);
    } else {
        const int u = t / S.n_in[1];
        bx = S.ilo[0] + u, by = S.ilo[1] + (t - u * S.n_in[1]), bz = Q.b[2] + fixed;
    }
}

LT_HD void lt_visit(const LtGrid &G, const LtQuery &Q, const unsigned long long *masks, int bx, int by, int bz,
                                         double &best, int &bi)
{
    unsigned long long word = masks[((int64_t)bx * G.nb[1] + by) * G.nb[2] + bz];
    if (!word) return;
    const int x0 = 4 * bx, y0 = 4 * by, z0 = 4 * bz;
    // (strict: a brick whose bound EQUALS the best may hold an equally near site of a smaller index)
    const double lb = lt_d2(lt_gap(G, Q.q[0], x0, min(x0 + 3, G.dims[0] - 1), 0), lt_gap(G, Q.q[1], y0, min(y0 + 3, G.dims[1] - 1), 1),
                            lt_gap(G, Q.q[2], z0, min(z0 + 3, G.dims[2] - 1), 2));
    if (lb > best) return;
    while (word) {
        const int l = __builtin_ctzll(word);
        word &= word - 1;
        const int x = x0 + (l >> 4), y = y0 + ((l >> 2) & 3), z = z0 + (l & 3);
        const double d2 = lt_d2(Q.q[0] - lt_site(G, x, 0), Q.q[1] - lt_site(G, y, 1), Q.q[2] - lt_site(G, z, 2));
        const int lin = (x * G.dims[1] + y) * G.dims[2] + z;
        if (d2 < best || (d2 == best && lin < bi)) {
            best = d2;
            bi = lin;
        }
    }
}

// After shells 0..r: every unvisited site lies outside the visited cube of bricks on some axis, i.e. in one of (up to) six
// slabs of cells; true when none of them can hold a site as near as `best` (strict: an equal distance is still visited) or
// when there is no slab left.  The same rule as nn_query_kernel (mesh_eval.hip), with the slabs' exact site coordinates in
// place of cell walls, so it also carries the whole distance of a vertex outside the volume and needs no slack.
LT_HD bool lt_done(const LtGrid &G, const LtQuery &Q, int r, double best)
{
    double full[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) full[a] = lt_gap(G, Q.q[a], 0, G.dims[a] - 1, a);
    double lb = INFINITY;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int side = 0; side < 2; ++side) {
            const int k0 = side ? 4 * (Q.b[a] + r + 1) : 0, k1 = side ? G.dims[a] : 4 * (Q.b[a] - r);    // cells [k0, k1)
            if (k0 >= k1) continue;
            const double e = lt_gap(G, Q.q[a], k0, k1 - 1, a);
            lb = fmin(lb, a == 0 ? lt_d2(e, full[1], full[2]) : (a == 1 ? lt_d2(full[0], e, full[2]) : lt_d2(full[0], full[1], e)));
        }
    return lb == INFINITY || best < lb;
}

struct LtOut {
    const int32_t *semantic, *instance;
    int32_t *idx, *sem, *ins;
    float *dist;
};

__device__ __forceinline__ void lt_store(const LtMap &M, const LtOut &O, int64_t i, double best, int bi)
{
    const bool hit = bi != 0x7fffffff;
    O.idx[i] = hit ? bi : -1;
    O.dist[i] = (float)sqrt(best);
    int sem = 0, ins = 0;
    if (hit) {
        const int32_t s = O.semantic[bi];
        sem = (s >= 0 && s < M.n) ? M.v[s] : 0;
        ins = O.instance[bi];
    }
    O.sem[i] = sem;
    O.ins[i] = ins;
}

__global__ __launch_bounds__(256) void lt_query_kernel(LtMap M, LtGrid G, const unsigned long long *masks, const float *query,
                                                       int64_t n_query, int near_shells, LtOut O, int32_t *queue_count,
                                                       int32_t *queue)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_query) return;
    const LtQuery Q = lt_query_of(G, query + 3 * i);
    double best = INFINITY;
    int bi = 0x7fffffff;
    bool done = false;
    const int r_end = min(Q.rmax, near_shells);
    for (int r = 0; r <= r_end && !done; ++r) {
        const LtShell S = lt_shell_of(G, Q, r);
        for (int t = 0; t < S.total; ++t) {
            int bx, by, bz;
            lt_shell_brick(S, Q, r, t, bx, by, bz);
            lt_visit(G, Q, masks, bx, by, bz, best, bi);
        }
        done = lt_done(G, Q, r, best);
    }
    if (done) lt_store(M, O, i, best, bi);
    else queue[atomicAdd(queue_count, 1)] = (int32_t)i;     // (at most n_query entries: the queue cannot overflow)
}

// (d2, index) minimum over the wave; every lane returns it
__device__ __forceinline__ void lt_wave_min(double &best, int &bi)
{
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const double ob = __shfl_xor(best, s);
        const int oi = __shfl_xor(bi, s);
        if (ob < best || (ob == best && oi < bi)) {
            best = ob;
            bi = oi;
        }
    }
}

__global__ __launch_bounds__(256) void lt_query_wave_kernel(LtMap M, LtGrid G, const unsigned long long *masks, const float *query,
                                                            LtOut O, const int32_t *queue_count, const int32_t *queue)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int count = *queue_count;       // (the live count: the launch covers the capacity, no host read in between)
    for (int w = blockIdx.x * 4 + threadIdx.x / kWave; w < count; w += gridDim.x * 4) {
        const int64_t i = queue[w];
        const LtQuery Q = lt_query_of(G, query + 3 * i);
        double best = INFINITY;
        int bi = 0x7fffffff;
        for (int r = 0; r <= Q.rmax; ++r) {
            const LtShell S = lt_shell_of(G, Q, r);
            for (int t = lane; t < S.total; t += kWave) {
                int bx, by, bz;
                lt_shell_brick(S, Q, r, t, bx, by, bz);
                lt_visit(G, Q, masks, bx, by, bz, best, bi);
            }
            lt_wave_min(best, bi);
            if (lt_done(G, Q, r, best)) break;
        }
        if (lane == 0) lt_store(M, O, i, best, bi);
    }
}

// ----------------------------------------------------------------------------------------------------------- vote

// One atomic pair per distinct (instance, class) of a wave, not per vertex: neighbouring vertices of a mesh mostly share both, and a
// few hundred table entries under 10^5 single adds serialise.  The wave's lowest lane of an entry carries its smallest vertex index.
__global__ __launch_bounds__(256) void lt_vote_kernel(const int32_t *mapped_sem, const int32_t *rank, int64_t n, int n_inst,
                                                      int n_class, int32_t *count, int32_t *first)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    int e = -1;
    if (i < n) {
        const int32_t c = mapped_sem[i], k = rank[i];
        if (c >= 0 && c < n_class && k >= 0 && k < n_inst) e = k * n_class + c;      // (n_inst * n_class fits: the host checked)
    }
    unsigned long long left = __ballot(e >= 0);
    while (left) {
        const int leader = __builtin_ctzll(left);
        const unsigned long long same = __ballot(e == __shfl(e, leader));
        if (lane == leader) {
            atomicAdd(&count[e], __popcll(same));
            atomicMin(&first[e], (int32_t)i);
        }
        left &= ~same;
    }
}

__global__ __launch_bounds__(256) void lt_vote_final_kernel(const int32_t *count, const int32_t *first, int n_inst, int n_class,
                                                            int32_t *class_out, int32_t *count_out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_inst) return;
    int best_c = 0, best_n = 0, best_first = 0x7fffffff, total = 0;
    for (int c = 0; c < n_class; ++c) {
        const int m = count[(int64_t)k * n_class + c], f = first[(int64_t)k * n_class + c];
        total += m;
        if (m > best_n || (m == best_n && m > 0 && f < best_first)) {
            best_c = c;
            best_n = m;
            best_first = f;
        }
    }
    class_out[k] = best_c;
    count_out[k] = total;
}

bool lt_dims_ok(const int32_t *dims)
{
    return dims && dims[0] >= 1 && dims[1] >= 1 && dims[2] >= 1 && (int64_t)dims[0] * dims[1] * dims[2] <= 0x7fffffffll;
}

void lt_grid(const int32_t *dims, const float *origin, double vs, LtGrid &G)
{
    G.vs = vs;
    for (int a = 0; a < 3; ++a) {
        G.o[a] = origin ? (double)origin[a] : 0.0;
        G.dims[a] = dims[a];
        G.nb[a] = (dims[a] + 3) / 4;
    }
}

void lt_map(const int32_t *mapping, int n_map, LtMap &M)
{
    M.n = n_map;
    for (int k = 0; k < kMaxMap; ++k) M.v[k] = k < n_map ? mapping[k] : 0;
}

}  // namespace

extern "C" {

size_t eprecon_label_transfer_workspace_bytes(const int32_t *dims_host, int64_t n_query)
{
    if (!lt_dims_ok(dims_host) || n_query < 0 || n_query > 0x7fffffffll) return 0;
    return 256 + align_up((size_t)n_query * 4, 256);
}

int eprecon_label_bricks_async(const int32_t *semantic, const int32_t *dims_host, const int32_t *mapping_host, int n_map,
                               uint64_t *masks_out, int32_t *status_out, void *stream)
{
    if (!semantic || !dims_host || !mapping_host || n_map < 1 || n_map > kMaxMap || !masks_out || !status_out ||
        dims_host[0] < 1 || dims_host[1] < 1 || dims_host[2] < 1)
        return EPRECON_ERR_ARG;
    if (!lt_dims_ok(dims_host)) return EPRECON_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    LtGrid G;
    LtMap M;
    lt_grid(dims_host, nullptr, 1.0, G);
    lt_map(mapping_host, n_map, M);
    const int64_t n_bricks = (int64_t)G.nb[0] * G.nb[1] * G.nb[2];
    EP_HIP_CHECK(hipMemsetAsync(status_out, 0, 2 * sizeof(int32_t), st));
    hipLaunchKernelGGL(lt_brick_mask_kernel, dim3((unsigned)ceil_div(n_bricks, 4)), dim3(256), 0, st, M, G, semantic, n_bricks,
                       reinterpret_cast<unsigned long long *>(masks_out), status_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_label_transfer_async(const uint64_t *masks, const int32_t *semantic, const int32_t *instance,
                                 const int32_t *dims_host, const float *origin_host, double voxel_size,
                                 const int32_t *mapping_host, int n_map, const float *query, int64_t n_query, int near_shells,
                                 int32_t *idx_out, float *dist_out, int32_t *sem_out, int32_t *ins_out, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (!masks || !semantic || !instance || !dims_host || !origin_host || !(voxel_size > 0.0) || !mapping_host || n_map < 1 ||
        n_map > kMaxMap || n_query < 0 || dims_host[0] < 1 || dims_host[1] < 1 || dims_host[2] < 1)
        return EPRECON_ERR_ARG;
    if (!lt_dims_ok(dims_host) || n_query > 0x7fffffffll) return EPRECON_ERR_UNSUPPORTED;
    if (n_query == 0) return EPRECON_OK;
    if (!query || !idx_out || !dist_out || !sem_out || !ins_out || !workspace) return EPRECON_ERR_ARG;
    if (workspace_bytes < eprecon_label_transfer_workspace_bytes(dims_host, n_query)) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    LtGrid G;
    LtMap M;
    lt_grid(dims_host, origin_host, voxel_size, G);
    lt_map(mapping_host, n_map, M);
    int32_t *queue_count = reinterpret_cast<int32_t *>(workspace), *queue = queue_count + 64;
    const LtOut O{semantic, instance, idx_out, sem_out, ins_out, dist_out};
    const auto *words = reinterpret_cast<const unsigned long long *>(masks);
    EP_HIP_CHECK(hipMemsetAsync(queue_count, 0, sizeof(int32_t), st));
    hipLaunchKernelGGL(lt_query_kernel, dim3((unsigned)ceil_div(n_query, 256)), dim3(256), 0, st, M, G, words, query, n_query,
                       near_shells < 0 ? -1 : near_shells, O, queue_count, queue);
    EP_LAUNCH_CHECK();
    if (near_shells <= (1 << 30)) {
        // one wave per queued vertex, four per workgroup; the grid covers the capacity up to a cap the waves stride over
        const int64_t blocks = std::min<int64_t>(ceil_div(n_query, 4), 8192);
        hipLaunchKernelGGL(lt_query_wave_kernel, dim3((unsigned)blocks), dim3(256), 0, st, M, G, words, query, O,
                           (const int32_t *)queue_count, (const int32_t *)queue);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

int eprecon_instance_vote_async(const int32_t *mapped_sem, const int32_t *rank, int64_t n, int n_inst, int n_class,
                                int32_t *class_out, int32_t *count_out, void *workspace, size_t workspace_bytes, void *stream)
{
    if (n < 0 || n_inst < 1 || n_class < 1 || !class_out || !count_out || !workspace ||
        (n > 0 && (!mapped_sem || !rank)))
        return EPRECON_ERR_ARG;
    // (the `first` table is cleared to the pattern 0x7f7f7f7f; an entry is one int)
    if (n > 0x7f7f7f7fll || (int64_t)n_inst * n_class > 0x7fffffffll) return EPRECON_ERR_UNSUPPORTED;
    const size_t table = align_up((size_t)n_inst * n_class * 4, 128);
    if (workspace_bytes < 2 * table) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int32_t *count = reinterpret_cast<int32_t *>(workspace);
    int32_t *first = reinterpret_cast<int32_t *>(reinterpret_cast<char *>(workspace) + table);
    EP_HIP_CHECK(hipMemsetAsync(count, 0, table, st));
    EP_HIP_CHECK(hipMemsetAsync(first, 0x7f, table, st));
    if (n > 0) {
        hipLaunchKernelGGL(lt_vote_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, mapped_sem, rank, n, n_inst, n_class,
                           count, first);
        EP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(lt_vote_final_kernel, dim3((unsigned)ceil_div(n_inst, 256)), dim3(256), 0, st, (const int32_t *)count,
                       (const int32_t *)first, n_inst, n_class, class_out, count_out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
