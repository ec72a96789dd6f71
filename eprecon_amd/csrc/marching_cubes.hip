// Iso-surface extraction (marching cubes) of the dense scene TSDF on gfx950 — SURVEY.md 8f row 1, the scene output path.
//
// Replaces the mesh extraction of the reference's SaveScene (utils.py:225-229,232-241: skimage.measure.marching_cubes
// on the host copy of outputs['scene_tsdf'], level 0), so that the dense scene volume no longer has to travel to the
// host (utils.py:291,345-348) before it becomes a mesh.  skimage is an un-vendored dependency (its default method is
// Lewiner's table set, which cannot be read here): this is the classic marching-cubes construction — one vertex per
// sign-changing grid edge at the linear zero crossing, faces from a 256-case table — with the table GENERATED (below)
// from one rule, not transcribed.  Vertex positions are those any marching-cubes variant produces; the triangulation
// inside ambiguous cells may differ from skimage's ("parity unpinned" for the face list; the mesh is pinned by its
// own properties: watertight, vertices on the level set, tests/test_marching_cubes.py).
//
// Table rule: corner i of a cell = (i & 1, (i >> 1) & 1, i >> 2); edge e = axis * 4 + (b + 2 c) joins the two corners
// that differ along `axis` with the other two coordinates (b, c).  A corner is "inside" when value < level.  On every
// cube face the cut edges are joined by segments — two cut edges: one segment; four (diagonal corners inside): each
// INSIDE corner is cut off by its own segment, a choice that depends on that face's signs only, so the two cells
// sharing the face agree and the surface has no cracks.  The segments close into loops; every loop is fanned from its
// first edge.  At most 5 triangles per cell (checked when the table is built).
//
// Pipeline: mc_count (per grid point: cut edges it owns along +x, +y, +z; per cell: triangle count) -> two scans ->
// mc_emit (vertices with gradient normals and optional label lookups; faces through the owning grid point of each
// edge, oriented so that the face normal agrees with the field gradient).  Output order is raster order: deterministic.
// The winding of a face whose normal is perpendicular to the cell gradient within 2^-20 s (s: the magnitudes that enter
// (u x w) . g, tests/mesh_ref.py) is unspecified; every other face is checked against the float64 witness there.
#include <math.h>
#include <string.h>

#include <mutex>

#include "scan.hpp"

namespace {
using namespace ep;

int8_t g_table_host[256][16];
int8_t *g_table_by_device[64] = {nullptr};   // one upload per device, under g_table_mutex (see upload_table)
std::mutex g_table_mutex;
bool g_table_built = false;

inline int edge_id(int axis, int b, int c) { return axis * 4 + b + 2 * c; }

// the two corners of edge e
inline void edge_corners(int e, int &c0, int &c1)
{
    const int axis = e >> 2, b = e & 1, c = (e >> 1) & 1;
    int p[3];
    const int o1 = (axis + 1) % 3, o2 = (axis + 2) % 3;
    // (b, c) are the coordinates along the two other axes in ascending axis order
    const int lo = o1 < o2 ? o1 : o2, hi = o1 < o2 ? o2 : o1;
    p[lo] = b; p[hi] = c;
    p[axis] = 0;
    c0 = p[0] + 2 * p[1] + 4 * p[2];
    p[axis] = 1;
    c1 = p[0] + 2 * p[1] + 4 * p[2];
}

void build_table()
{
    if (g_table_built) return;
    for (int cs = 0; cs < 256; ++cs) {
        int nbr[12][2], deg[12];
        for (int e = 0; e < 12; ++e) deg[e] = 0;
        auto link = [&](int a, int b) { nbr[a][deg[a]++] = b; nbr[b][deg[b]++] = a; };
        // six faces: fixed axis f, side s; the face's corners in cyclic order (u, w) = (0,0),(1,0),(1,1),(0,1)
        for (int f = 0; f < 3; ++f)
            for (int s = 0; s < 2; ++s) {
                const int u = (f + 1) % 3, w = (f + 2) % 3;
                int corner[4], fedge[4];
                const int cu[4] = {0, 1, 1, 0}, cw[4] = {0, 0, 1, 1};
                for (int k = 0; k < 4; ++k) {
                    int p[3];
                    p[f] = s; p[u] = cu[k]; p[w] = cw[k];
                    corner[k] = p[0] + 2 * p[1] + 4 * p[2];
                }
                for (int k = 0; k < 4; ++k) {  // edge between corner k and k + 1
                    const int a = corner[k], b = corner[(k + 1) & 3];
                    const int diff = a ^ b, axis = diff == 1 ? 0 : (diff == 2 ? 1 : 2);
                    const int base = a & ~diff;
                    const int p[3] = {base & 1, (base >> 1) & 1, base >> 2};
                    const int o1 = (axis + 1) % 3, o2 = (axis + 2) % 3;
                    const int lo = o1 < o2 ? o1 : o2, hi = o1 < o2 ? o2 : o1;
                    fedge[k] = edge_id(axis, p[lo], p[hi]);
                }
                bool in[4], cut[4];
                int ncut = 0;
                for (int k = 0; k < 4; ++k) in[k] = (cs >> corner[k]) & 1;
                for (int k = 0; k < 4; ++k) {
                    cut[k] = in[k] != in[(k + 1) & 3];
                    ncut += cut[k];
                }
                if (ncut == 2) {
                    int a = -1, b = -1;
                    for (int k = 0; k < 4; ++k)
                        if (cut[k]) (a < 0 ? a : b) = fedge[k];
                    link(a, b);
                } else if (ncut == 4) {
                    // every inside corner k is cut off: join its two incident edges (k - 1, k)
                    for (int k = 0; k < 4; ++k)
                        if (in[k]) link(fedge[(k + 3) & 3], fedge[k]);
                }
            }
        int n = 0;
        bool used[12] = {false};
        int8_t *row = g_table_host[cs];
        for (int e0 = 0; e0 < 12; ++e0) {
            if (used[e0] || deg[e0] == 0) continue;
            int loop[12], len = 0, prev = -1, cur = e0;
            while (true) {
                loop[len++] = cur;
                used[cur] = true;
                const int nx = nbr[cur][0] != prev ? nbr[cur][0] : nbr[cur][1];
                prev = cur;
                cur = nx;
                if (cur == e0 || len >= 12) break;
            }
            for (int k = 1; k + 1 < len; ++k) {
                if (n + 3 > 15) break;
                row[n++] = (int8_t)loop[0]; row[n++] = (int8_t)loop[k]; row[n++] = (int8_t)loop[k + 1];
            }
        }
        for (; n < 16; ++n) row[n] = -1;
    }
    g_table_built = true;
}

struct McParams {
    const float *vol;
    int Dx, Dy, Dz;
    float level;
    const float *weight;     // MASKED instantiations only: cubes with a corner of weight 0 emit nothing
};

__device__ __forceinline__ float at(const McParams &p, int x, int y, int z) { return p.vol[((size_t)x * p.Dy + y) * p.Dz + z]; }

// MASKED (open3d's ExtractTriangleMesh rule): a cell takes part only when all eight corners have weight > 0; a cut edge
// carries a vertex only when one of the (up to four) cells around it takes part.  The unmasked instantiations compile to
// the code they always were (every `if constexpr (MASKED)` branch vanishes).
__device__ __forceinline__ bool cell_live(const McParams &p, int x, int y, int z)
{
    if (x < 0 || y < 0 || z < 0 || x + 1 >= p.Dx || y + 1 >= p.Dy || z + 1 >= p.Dz) return false;
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 8; ++k)
        ok = ok && p.weight[((size_t)(x + (k & 1)) * p.Dy + (y + ((k >> 1) & 1))) * p.Dz + (z + (k >> 2))] > 0.0f;
    return ok;
}

__device__ __forceinline__ bool edge_live(const McParams &p, int x, int y, int z, int axis)
{
    const int o1 = (axis + 1) % 3, o2 = (axis + 2) % 3;
    const int lo = o1 < o2 ? o1 : o2, hi = o1 < o2 ? o2 : o1;
    for (int k = 0; k < 4; ++k) {
        int q[3] = {x, y, z};
        q[lo] -= k & 1; q[hi] -= k >> 1;
        if (cell_live(p, q[0], q[1], q[2])) return true;
    }
    return false;
}

// edge (x,y,z)+axis is cut (and, when MASKED, live); the neighbour along axis must be inside the grid
template <bool MASKED>
__device__ __forceinline__ bool edge_cut(const McParams &p, int x, int y, int z, int axis, bool in0)
{
    const bool cut = (at(p, x + (axis == 0), y + (axis == 1), z + (axis == 2)) < p.level) != in0;
    if constexpr (MASKED) return cut && edge_live(p, x, y, z, axis);
    return cut;
}

// per grid point: number of sign-changing edges it owns (+x, +y, +z); per cell (same index, x < Dx-1 ...): triangles
template <bool MASKED>
__global__ __launch_bounds__(256) void mc_count_kernel(McParams p, const int8_t *table, int32_t *nvert, int32_t *ntri)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = p.Dx * p.Dy * p.Dz;
    if (i >= n) return;
    const int z = i % p.Dz, y = (i / p.Dz) % p.Dy, x = i / (p.Dz * p.Dy);
    const bool in0 = at(p, x, y, z) < p.level;
    int c = 0;
    if (x + 1 < p.Dx) c += edge_cut<MASKED>(p, x, y, z, 0, in0);
    if (y + 1 < p.Dy) c += edge_cut<MASKED>(p, x, y, z, 1, in0);
    if (z + 1 < p.Dz) c += edge_cut<MASKED>(p, x, y, z, 2, in0);
    nvert[i] = c;
    int t = 0;
    if (x + 1 < p.Dx && y + 1 < p.Dy && z + 1 < p.Dz && (!MASKED || cell_live(p, x, y, z))) {
        int cs = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) cs |= (at(p, x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2)) < p.level ? 1 : 0) << k;
        const int8_t *row = table + cs * 16;
        while (t < 5 && row[3 * t] >= 0) ++t;
    }
    ntri[i] = t;
}

__device__ __forceinline__ float3 gradient(const McParams &p, int x, int y, int z)
{
    const int xm = max(x - 1, 0), xp = min(x + 1, p.Dx - 1), ym = max(y - 1, 0), yp = min(y + 1, p.Dy - 1),
              zm = max(z - 1, 0), zp = min(z + 1, p.Dz - 1);
    return make_float3((at(p, xp, y, z) - at(p, xm, y, z)) / (float)max(xp - xm, 1),
                       (at(p, x, yp, z) - at(p, x, ym, z)) / (float)max(yp - ym, 1),
                       (at(p, x, y, zp) - at(p, x, y, zm)) / (float)max(zp - zm, 1));
}

// vertices: one per cut edge, owned by the edge's lower grid point; order (point raster, axis x < y < z)
template <bool MASKED>
__global__ __launch_bounds__(256) void mc_vertex_kernel(McParams p, const int32_t *voff, float *verts, float *normals,
                                                        const int32_t *label_a, const int32_t *label_b, int32_t *out_a,
                                                        int32_t *out_b)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = p.Dx * p.Dy * p.Dz;
    if (i >= n) return;
    const int z = i % p.Dz, y = (i / p.Dz) % p.Dy, x = i / (p.Dz * p.Dy);
    const float v0 = at(p, x, y, z);
    const bool in0 = v0 < p.level;
    int o = voff[i];
    const float3 g0 = gradient(p, x, y, z);
#pragma unroll
    for (int axis = 0; axis < 3; ++axis) {
        const int x1 = x + (axis == 0), y1 = y + (axis == 1), z1 = z + (axis == 2);
        if (x1 >= p.Dx || y1 >= p.Dy || z1 >= p.Dz) continue;
        const float v1 = at(p, x1, y1, z1);
        if ((v1 < p.level) == in0) continue;
        if constexpr (MASKED) {
            if (!edge_live(p, x, y, z, axis)) continue;
        }
        const float t = __fdiv_rn(p.level - v0, v1 - v0);   // linear zero crossing on the edge
        const float px = (float)x + (axis == 0 ? t : 0.0f), py = (float)y + (axis == 1 ? t : 0.0f),
                    pz = (float)z + (axis == 2 ? t : 0.0f);
        verts[3 * (size_t)o + 0] = px; verts[3 * (size_t)o + 1] = py; verts[3 * (size_t)o + 2] = pz;
        if (normals) {
            const float3 g1 = gradient(p, x1, y1, z1);
            float nx = g0.x + t * (g1.x - g0.x), ny = g0.y + t * (g1.y - g0.y), nz = g0.z + t * (g1.z - g0.z);
            const float len = sqrtf(nx * nx + ny * ny + nz * nz);
            if (len > 0.0f) { nx /= len; ny /= len; nz /= len; }
            normals[3 * (size_t)o + 0] = nx; normals[3 * (size_t)o + 1] = ny; normals[3 * (size_t)o + 2] = nz;
        }
        if (label_a || label_b) {
            // utils.py:236-239: labels of the nearest voxel, np.round (half to even) and clip into the volume
            const int rx = min(max((int)rintf(px), 0), p.Dx - 1), ry = min(max((int)rintf(py), 0), p.Dy - 1),
                      rz = min(max((int)rintf(pz), 0), p.Dz - 1);
            const size_t c = ((size_t)rx * p.Dy + ry) * p.Dz + rz;
            if (label_a) out_a[o] = label_a[c];
            if (label_b) out_b[o] = label_b[c];
        }
        ++o;
    }
}

template <bool MASKED>
__device__ __forceinline__ int edge_vertex(const McParams &p, const int32_t *voff, int x, int y, int z, int e)
{
    // edge e = axis * 4 + (b + 2 c): owner grid point = cell origin + (b, c) along the other two axes (ascending)
    const int axis = e >> 2, b = e & 1, c = (e >> 1) & 1;
    int q[3] = {x, y, z};
    const int o1 = (axis + 1) % 3, o2 = (axis + 2) % 3;
    const int lo = o1 < o2 ? o1 : o2, hi = o1 < o2 ? o2 : o1;
    q[lo] += b; q[hi] += c;
    const int i = (q[0] * p.Dy + q[1]) * p.Dz + q[2];
    // rank of `axis` among the owner's cut edges
    const bool in0 = at(p, q[0], q[1], q[2]) < p.level;
    int r = 0;
    if (axis > 0 && q[0] + 1 < p.Dx) r += edge_cut<MASKED>(p, q[0], q[1], q[2], 0, in0);
    if (axis > 1 && q[1] + 1 < p.Dy) r += edge_cut<MASKED>(p, q[0], q[1], q[2], 1, in0);
    return voff[i] + r;
}

template <bool MASKED>
__global__ __launch_bounds__(256) void mc_face_kernel(McParams p, const int8_t *table, const int32_t *voff, const int32_t *toff,
                                                      const float *verts, int32_t *faces)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = p.Dx * p.Dy * p.Dz;
    if (i >= n) return;
    const int z = i % p.Dz, y = (i / p.Dz) % p.Dy, x = i / (p.Dz * p.Dy);
    if (x + 1 >= p.Dx || y + 1 >= p.Dy || z + 1 >= p.Dz) return;
    if constexpr (MASKED) {
        if (!cell_live(p, x, y, z)) return;
    }
    int cs = 0;
    float val[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        val[k] = at(p, x + (k & 1), y + ((k >> 1) & 1), z + (k >> 2));
        cs |= (val[k] < p.level ? 1 : 0) << k;
    }
    const int8_t *row = table + cs * 16;
    if (row[0] < 0) return;
    // field gradient of the cell (trilinear, at the centre): faces are wound so that their normal follows it
    const float gx = 0.25f * ((val[1] + val[3] + val[5] + val[7]) - (val[0] + val[2] + val[4] + val[6]));
    const float gy = 0.25f * ((val[2] + val[3] + val[6] + val[7]) - (val[0] + val[1] + val[4] + val[5]));
    const float gz = 0.25f * ((val[4] + val[5] + val[6] + val[7]) - (val[0] + val[1] + val[2] + val[3]));
    int o = toff[i];
    for (int t = 0; t < 5 && row[3 * t] >= 0; ++t, ++o) {
        int a = edge_vertex<MASKED>(p, voff, x, y, z, row[3 * t]), b = edge_vertex<MASKED>(p, voff, x, y, z, row[3 * t + 1]),
            c = edge_vertex<MASKED>(p, voff, x, y, z, row[3 * t + 2]);
        const float ax = verts[3 * (size_t)a], ay = verts[3 * (size_t)a + 1], az = verts[3 * (size_t)a + 2];
        const float ux = verts[3 * (size_t)b] - ax, uy = verts[3 * (size_t)b + 1] - ay, uz = verts[3 * (size_t)b + 2] - az;
        const float wx = verts[3 * (size_t)c] - ax, wy = verts[3 * (size_t)c + 1] - ay, wz = verts[3 * (size_t)c + 2] - az;
        const float nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        if (nx * gx + ny * gy + nz * gz < 0.0f) {
            const int s = b; b = c; c = s;
        }
        faces[3 * (size_t)o] = a; faces[3 * (size_t)o + 1] = b; faces[3 * (size_t)o + 2] = c;
    }
}

// the case table on the CURRENT device (built / uploaded once per device; callers may be on different threads)
int upload_table(const int8_t **table_out)
{
    int device = 0;
    EP_HIP_CHECK(hipGetDevice(&device));
    if (device < 0 || device >= 64) return EPRECON_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lock(g_table_mutex);
    build_table();
    int8_t *&dev = g_table_by_device[device];
    if (!dev) {
        EP_HIP_CHECK(hipMalloc(&dev, sizeof(g_table_host)));
        EP_HIP_CHECK(hipMemcpy(dev, g_table_host, sizeof(g_table_host), hipMemcpyHostToDevice));
    }
    *table_out = dev;
    return EPRECON_OK;
}

}  // namespace

extern "C" {

// the generated 256 x 16 case table (edge triples, -1 terminated): for tests / the oracle cross-check
int eprecon_marching_cubes_table(int8_t *out_host)
{
    if (!out_host) return EPRECON_ERR_ARG;
    std::lock_guard<std::mutex> lock(g_table_mutex);
    build_table();
    memcpy(out_host, g_table_host, sizeof(g_table_host));
    return EPRECON_OK;
}

size_t eprecon_marching_cubes_workspace_bytes(int dx, int dy, int dz)
{
    const size_t n = (size_t)dx * dy * dz;
    return 4 * align_up(n * 4, 256) + 2 * scan_scratch_bytes((int64_t)n) + 256;
}

}  // extern "C"

namespace {

template <bool MASKED>
int mc_count(const float *volume, const float *weight, int dx, int dy, int dz, float level, int64_t *counts_host,
             void *workspace, size_t workspace_bytes, void *stream)
{
    if (!volume || (MASKED && !weight) || dx < 2 || dy < 2 || dz < 2 || !counts_host || !workspace) return EPRECON_ERR_ARG;
    const int64_t n = (int64_t)dx * dy * dz;
    if (n > 0x7fffffff / 4) return EPRECON_ERR_UNSUPPORTED;
    if (workspace_bytes < eprecon_marching_cubes_workspace_bytes(dx, dy, dz)) return EPRECON_ERR_WORKSPACE;
    const int8_t *table = nullptr;
    int rc = upload_table(&table);
    if (rc != EPRECON_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    const size_t seg = align_up((size_t)n * 4, 256), sseg = scan_scratch_bytes(n);
    int32_t *nvert = reinterpret_cast<int32_t *>(ws), *ntri = reinterpret_cast<int32_t *>(ws + seg);
    int32_t *voff = reinterpret_cast<int32_t *>(ws + 2 * seg), *toff = reinterpret_cast<int32_t *>(ws + 3 * seg);
    int32_t *s1 = reinterpret_cast<int32_t *>(ws + 4 * seg), *s2 = reinterpret_cast<int32_t *>(ws + 4 * seg + sseg);
    int32_t *totals = reinterpret_cast<int32_t *>(ws + 4 * seg + 2 * sseg);
    McParams p{volume, dx, dy, dz, level, weight};
    hipLaunchKernelGGL(mc_count_kernel<MASKED>, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, p, table, nvert,
                       ntri);
    EP_LAUNCH_CHECK();
    rc = ep::exclusive_scan_i32(nvert, (int)n, voff, s1, totals, st);
    if (rc == EPRECON_OK) rc = ep::exclusive_scan_i32(ntri, (int)n, toff, s2, totals + 1, st);
    if (rc != EPRECON_OK) return rc;
    int32_t host[2];
    EP_HIP_CHECK(hipMemcpyAsync(host, totals, sizeof(host), hipMemcpyDeviceToHost, st));
    EP_HIP_CHECK(hipStreamSynchronize(st));
    counts_host[0] = host[0];
    counts_host[1] = host[1];
    return EPRECON_OK;
}

template <bool MASKED>
int mc_emit(const float *volume, const float *weight, int dx, int dy, int dz, float level, float *verts, float *normals,
            int32_t *faces, const int32_t *label_a, const int32_t *label_b, int32_t *vert_label_a, int32_t *vert_label_b,
            const void *workspace, void *stream)
{
    if (!volume || (MASKED && !weight) || !verts || !faces || !workspace || (label_a && !vert_label_a) ||
        (label_b && !vert_label_b))
        return EPRECON_ERR_ARG;
    const int64_t n = (int64_t)dx * dy * dz;
    const int8_t *table = nullptr;
    const int trc = upload_table(&table);
    if (trc != EPRECON_OK) return trc;
    hipStream_t st = (hipStream_t)stream;
    const char *ws = reinterpret_cast<const char *>(workspace);
    const size_t seg = align_up((size_t)n * 4, 256);
    const int32_t *voff = reinterpret_cast<const int32_t *>(ws + 2 * seg), *toff = reinterpret_cast<const int32_t *>(ws + 3 * seg);
    McParams p{volume, dx, dy, dz, level, weight};
    const dim3 grid((unsigned)ceil_div(n, 256)), blk(256);
    hipLaunchKernelGGL(mc_vertex_kernel<MASKED>, grid, blk, 0, st, p, voff, verts, normals, label_a, label_b, vert_label_a,
                       vert_label_b);
    EP_LAUNCH_CHECK();
    hipLaunchKernelGGL(mc_face_kernel<MASKED>, grid, blk, 0, st, p, table, voff, toff, (const float *)verts, faces);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // namespace

extern "C" {

// phase 1 (blocking): counts_host[0] = vertices, [1] = triangles; the workspace keeps the scanned offsets for phase 2
int eprecon_marching_cubes_count(const float *volume, int dx, int dy, int dz, float level, int64_t *counts_host,
                                 void *workspace, size_t workspace_bytes, void *stream)
{
    return mc_count<false>(volume, nullptr, dx, dy, dz, level, counts_host, workspace, workspace_bytes, stream);
}

// phase 2: verts f32[nv,3] (voxel coordinates, like skimage), normals f32[nv,3] or NULL, faces int32[nt,3];
// optional per-vertex labels of the nearest voxel from two int32 volumes (semantic / instance, utils.py:236-239)
int eprecon_marching_cubes_emit_async(const float *volume, int dx, int dy, int dz, float level, float *verts, float *normals,
                                      int32_t *faces, const int32_t *label_a, const int32_t *label_b, int32_t *vert_label_a,
                                      int32_t *vert_label_b, const void *workspace, void *stream)
{
    return mc_emit<false>(volume, nullptr, dx, dy, dz, level, verts, normals, faces, label_a, label_b, vert_label_a,
                          vert_label_b, workspace, stream);
}

// the same two phases restricted to the cells whose eight corners all have weight > 0 (the trimmed surface of the scene
// evaluation: open3d's ExtractTriangleMesh rule); weight f32[dx,dy,dz] like the volume
int eprecon_marching_cubes_count_masked(const float *volume, const float *weight, int dx, int dy, int dz, float level,
                                        int64_t *counts_host, void *workspace, size_t workspace_bytes, void *stream)
{
    return mc_count<true>(volume, weight, dx, dy, dz, level, counts_host, workspace, workspace_bytes, stream);
}

int eprecon_marching_cubes_emit_masked_async(const float *volume, const float *weight, int dx, int dy, int dz, float level,
                                             float *verts, float *normals, int32_t *faces, const int32_t *label_a,
                                             const int32_t *label_b, int32_t *vert_label_a, int32_t *vert_label_b,
                                             const void *workspace, void *stream)
{
    return mc_emit<true>(volume, weight, dx, dy, dz, level, verts, normals, faces, label_a, label_b, vert_label_a,
                         vert_label_b, workspace, stream);
}

}  // extern "C"
