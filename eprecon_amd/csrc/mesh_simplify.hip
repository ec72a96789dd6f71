// Mesh simplification by quadric vertex clustering (eprecon_amd/simplify.py): the three launches of the
// rule that look at every vertex, every face and every cluster.
//
//   sm_keys_kernel      one lane per vertex: its cell floor((double(v) - origin) / cell) per axis in fp64 (the library is built
//                       with -ffp-contract=off, so this is the expression as numpy rounds it), the range check and the packed
//                       key (cx + 2^20) << 42 | (cy + 2^20) << 21 | (cz + 2^20), which orders like (cx, cy, cz).  No fp64 copy
//                       of the vertices exists anywhere.
//   sm_faces_kernel     one lane per face: the cluster triple (-1 three times for a face with an index outside [0, N)), the
//                       key of the unordered triple (a, b, c sorted, 21 bits each; -1 for a face with two equal clusters) and
//                       the marks of the clusters a face with three different clusters refers to.  A dropped duplicate has the
//                       triple of the face that survives it, so these marks are the marks of the surviving faces.
//   sm_quadrics_kernel  one lane per cluster, over the two CSR lists of eprecon_segment_lists_async (the corner entries 3f + c
//                       and the member vertices of the cluster, each ascending): the mean, the area-weighted plane quadrics,
//                       the normal sum and the colour sums, the 3x3 solve, the clip of the segment mean -> minimiser to the
//                       cell's box, the outputs.  Every fp64 sum runs in list order in one lane: no float atomics, the same
//                       bits on every run.
//
// House rules (components.hip, segment_stats.hip): every loop is bounded by a count the host passed, every index read from
// memory is checked against its range before it is used as one, the status word collects what the wrapper turns into an
// exception (1 a face index outside [0, N), 2 a vertex that is not finite, 4 a cell outside +-2^20), no barrier is used and
// so no exit precedes one.
#include <algorithm>

#include "common.hpp"

namespace {

using namespace ep;

constexpr int kCellBits = 21;
constexpr long long kCellBias = 1ll << (kCellBits - 1);      // cells in [-2^20, 2^20)
constexpr long long kCellMask = (1ll << kCellBits) - 1;
constexpr int kMaxClusters = 1 << kCellBits;                 // three cluster ids in one 63-bit face key
constexpr int64_t kMaxVertices = 0x7fffffff;
constexpr int64_t kMaxCorners = 0x7fffffff;                  // 3 M < 2^31

struct Frame {
    double ox, oy, oz, cell;
};

__global__ __launch_bounds__(256) void sm_keys_kernel(const float *verts, int64_t n, Frame fr, long long *key, int32_t *status)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = (double)verts[3 * i], y = (double)verts[3 * i + 1], z = (double)verts[3 * i + 2];
    int flags = 0;
    long long k = -1;
    if (!(fabs(x) <= 3.5e38 && fabs(y) <= 3.5e38 && fabs(z) <= 3.5e38)) {      // (an infinity or a NaN fails the comparison)
        flags = 2;
    } else {
        const double qx = floor((x - fr.ox) / fr.cell), qy = floor((y - fr.oy) / fr.cell), qz = floor((z - fr.oz) / fr.cell);
        const double lo = -(double)kCellBias, hi = (double)kCellBias;
        if (qx >= lo && qx < hi && qy >= lo && qy < hi && qz >= lo && qz < hi)
            k = (((long long)qx + kCellBias) << (2 * kCellBits)) | (((long long)qy + kCellBias) << kCellBits) | ((long long)qz + kCellBias);
        else
            flags = 4;
    }
    key[i] = k;
    if (flags) atomicOr(&status[0], flags);
}

__global__ __launch_bounds__(256) void sm_faces_kernel(const int32_t *faces, int64_t m, const int32_t *cluster, int64_t n, int n_clusters,
                                                       int32_t *tri, long long *face_key, uint8_t *referenced, int32_t *status)
{
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= m) return;
    const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    int a = -1, b = -1, c = -1;
    long long k = -1;
    bool bad = ia < 0 || ia >= n || ib < 0 || ib >= n || ic < 0 || ic >= n;
    if (!bad) {
        a = cluster[ia], b = cluster[ib], c = cluster[ic];
        bad = a < 0 || a >= n_clusters || b < 0 || b >= n_clusters || c < 0 || c >= n_clusters;      // (the caller's ids)
        if (bad) a = b = c = -1;
    }
    if (bad) {
        atomicOr(&status[0], 1);
    } else if (a != b && b != c && a != c) {
        const int lo = min(a, min(b, c)), hi = max(a, max(b, c)), mid = a + b + c - lo - hi;      // (ids below 2^21: no overflow)
        k = ((long long)lo << (2 * kCellBits)) | ((long long)mid << kCellBits) | (long long)hi;
        referenced[a] = 1, referenced[b] = 1, referenced[c] = 1;      // (every writer stores the same byte)
    }
    tri[3 * f] = a, tri[3 * f + 1] = b, tri[3 * f + 2] = c;
    face_key[f] = k;
}

__device__ __forceinline__ double cell_centre(long long q, double origin, double cell) { return origin + ((double)q + 0.5) * cell; }

// (A + lambda I) x = r for the symmetric positive definite matrix a = (xx, xy, xz, yy, yz, zz), by Cholesky; -> false when a
// pivot is not positive (a NaN, or lambda = 0 on a singular A): the caller keeps the mean
__device__ __forceinline__ bool solve_spd3(const double a[6], const double r[3], double x[3])
{
    if (!(a[0] > 0.0)) return false;
    const double l00 = sqrt(a[0]);
    const double l10 = a[1] / l00, l20 = a[2] / l00;
    const double d1 = a[3] - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1);
    const double l21 = (a[4] - l20 * l10) / l11;
    const double d2 = a[5] - l20 * l20 - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    const double y0 = r[0] / l00;
    const double y1 = (r[1] - l10 * y0) / l11;
    const double y2 = (r[2] - l20 * y0 - l21 * y1) / l22;
    x[2] = y2 / l22;
    x[1] = (y1 - l21 * x[2]) / l11;
    x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
    return true;
}

__global__ __launch_bounds__(64) void sm_quadrics_kernel(const float *verts, int64_t n, const int32_t *faces, int64_t m, const uint8_t *colors,
                                                         const long long *key, const int32_t *corner_offsets,
                                                         const int32_t *corner_order, const int32_t *member_offsets,
                                                         const int32_t *member_order, int n_clusters, Frame fr, double regularize,
                                                         double *pos, float *normal, uint8_t *rgb)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n_clusters) return;
    const int64_t corners = 3 * m;
    // the lists of this cluster, clamped to the arrays they index: a loop below runs at most n (members) or 3 m (corners) times
    const int64_t m0 = std::max<int64_t>(member_offsets[k], 0), m1 = std::min<int64_t>(member_offsets[k + 1], n);
    const int64_t c0 = std::max<int64_t>(corner_offsets[k], 0), c1 = std::min<int64_t>(corner_offsets[k + 1], corners);
    const double half = 0.5 * fr.cell;
    double cx = 0.0, cy = 0.0, cz = 0.0;      // the cell's centre, from the key of the first member
    double sx = 0.0, sy = 0.0, sz = 0.0;
    long long count = 0, sr = 0, sg = 0, sb = 0;
    bool framed = false;
    for (int64_t e = m0; e < m1; ++e) {
        const int v = member_order[e];
        if (v < 0 || v >= n) continue;
        if (!framed) {
            const long long q = key[v];
            if (q < 0) continue;      // (a vertex the key kernel refused: the wrapper has raised already)
            cx = cell_centre(((q >> (2 * kCellBits)) & kCellMask) - kCellBias, fr.ox, fr.cell);
            cy = cell_centre(((q >> kCellBits) & kCellMask) - kCellBias, fr.oy, fr.cell);
            cz = cell_centre((q & kCellMask) - kCellBias, fr.oz, fr.cell);
            framed = true;
        }
        sx += (double)verts[3 * (int64_t)v] - cx;
        sy += (double)verts[3 * (int64_t)v + 1] - cy;
        sz += (double)verts[3 * (int64_t)v + 2] - cz;
        ++count;
        if (colors) sr += colors[3 * (int64_t)v], sg += colors[3 * (int64_t)v + 1], sb += colors[3 * (int64_t)v + 2];
    }
    double mean[3] = {0.0, 0.0, 0.0};
    if (count > 0) mean[0] = sx / (double)count, mean[1] = sy / (double)count, mean[2] = sz / (double)count;

    double a[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, ns[3] = {0.0, 0.0, 0.0};
    for (int64_t e = c0; e < c1; ++e) {
        const int entry = corner_order[e];
        if (entry < 0 || entry >= corners) continue;
        const int64_t f = entry / 3;
        const int ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
        if (ia < 0 || ia >= n || ib < 0 || ib >= n || ic < 0 || ic >= n) continue;
        // the normal from the vertices as they are (differences of float32 values: the same bits whatever the cell), the plane's
        // offset from the corner relative to the centre
        const double pax = (double)verts[3 * (int64_t)ia], pay = (double)verts[3 * (int64_t)ia + 1], paz = (double)verts[3 * (int64_t)ia + 2];
        const double e1x = (double)verts[3 * (int64_t)ib] - pax, e1y = (double)verts[3 * (int64_t)ib + 1] - pay, e1z = (double)verts[3 * (int64_t)ib + 2] - paz;
        const double e2x = (double)verts[3 * (int64_t)ic] - pax, e2y = (double)verts[3 * (int64_t)ic + 1] - pay, e2z = (double)verts[3 * (int64_t)ic + 2] - paz;
        const double ax = pax - cx, ay = pay - cy, az = paz - cz;
        const double nx = e1y * e2z - e1z * e2y, ny = e1z * e2x - e1x * e2z, nz = e1x * e2y - e1y * e2x;
        const double len = sqrt(nx * nx + ny * ny + nz * nz);
        if (!(len > 0.0)) continue;      // (a zero-area face, or one with a vertex that is not finite)
        const double ux = nx / len, uy = ny / len, uz = nz / len, w = 0.5 * len;
        const double d = -(ux * ax + uy * ay + uz * az);
        a[0] += w * ux * ux, a[1] += w * ux * uy, a[2] += w * ux * uz;
        a[3] += w * uy * uy, a[4] += w * uy * uz, a[5] += w * uz * uz;
        const double wd = -w * d;
        b[0] += wd * ux, b[1] += wd * uy, b[2] += wd * uz;
        ns[0] += nx, ns[1] += ny, ns[2] += nz;
    }

    // the minimiser of the regularised quadric, then the largest step from the mean towards it that stays in the box
    double x[3] = {mean[0], mean[1], mean[2]};
    const double trace = a[0] + a[3] + a[5];
    if (trace > 0.0) {
        const double lambda = regularize * trace / 3.0;
        const double al[6] = {a[0] + lambda, a[1], a[2], a[3] + lambda, a[4], a[5] + lambda};
        const double r[3] = {b[0] + lambda * mean[0], b[1] + lambda * mean[1], b[2] + lambda * mean[2]};
        double s[3];
        if (solve_spd3(al, r, s)) x[0] = s[0], x[1] = s[1], x[2] = s[2];
    }
    double t = 1.0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        const double dir = x[ax] - mean[ax];
        if (dir > 0.0) t = fmin(t, (half - mean[ax]) / dir);
        else if (dir < 0.0) t = fmin(t, (-half - mean[ax]) / dir);
    }
    t = fmax(t, 0.0);
    const double centre[3] = {cx, cy, cz};
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        double p = mean[ax] + t * (x[ax] - mean[ax]);
        p = fmin(fmax(p, -half), half);      // (the rounding of the step; a no-op in exact arithmetic)
        pos[3 * (int64_t)k + ax] = centre[ax] + p;
    }
    const double nl = sqrt(ns[0] * ns[0] + ns[1] * ns[1] + ns[2] * ns[2]);
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) normal[3 * (int64_t)k + ax] = nl > 0.0 ? (float)(ns[ax] / nl) : 0.0f;
    if (rgb) {
        const long long den = 2 * std::max<long long>(count, 1);
        rgb[3 * (int64_t)k] = (uint8_t)((2 * sr + count) / den);
        rgb[3 * (int64_t)k + 1] = (uint8_t)((2 * sg + count) / den);
        rgb[3 * (int64_t)k + 2] = (uint8_t)((2 * sb + count) / den);
    }
}

bool frame_of(const double *origin_host, double cell, Frame &fr)
{
    if (!origin_host || !(cell > 0.0) || !(cell < 1e300)) return false;
    for (int a = 0; a < 3; ++a)
        if (!(fabs(origin_host[a]) < 1e300)) return false;
    fr = Frame{origin_host[0], origin_host[1], origin_host[2], cell};
    return true;
}

}  // namespace

extern "C" {

int32_t eprecon_simplify_max_clusters(void) { return kMaxClusters; }

int eprecon_simplify_keys_async(const float *verts, int64_t n, const double *origin_host, double cell, int64_t *key, int32_t *status,
                                void *stream)
{
    Frame fr;
    if (n < 0 || !status || !frame_of(origin_host, cell, fr) || (n > 0 && (!verts || !key))) return EPRECON_ERR_ARG;
    if (n > kMaxVertices) return EPRECON_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    EP_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    if (n == 0) return EPRECON_OK;
    hipLaunchKernelGGL(sm_keys_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, verts, n, fr, reinterpret_cast<long long *>(key),
                       status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_simplify_faces_async(const int32_t *faces, int64_t m, const int32_t *cluster, int64_t n, int32_t n_clusters, int32_t *tri,
                                 int64_t *face_key, uint8_t *referenced, int32_t *status, void *stream)
{
    if (m < 0 || n < 0 || n_clusters < 0 || !status || (m > 0 && (!faces || !tri || !face_key)) || (n > 0 && !cluster) ||
        (n_clusters > 0 && !referenced))
        return EPRECON_ERR_ARG;
    if (n > kMaxVertices || 3 * m > kMaxCorners || n_clusters > kMaxClusters) return EPRECON_ERR_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    EP_HIP_CHECK(hipMemsetAsync(status, 0, sizeof(int32_t), st));
    if (n_clusters > 0) EP_HIP_CHECK(hipMemsetAsync(referenced, 0, (size_t)n_clusters, st));
    if (m == 0) return EPRECON_OK;
    hipLaunchKernelGGL(sm_faces_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, faces, m, cluster, n, (int)n_clusters, tri,
                       reinterpret_cast<long long *>(face_key), referenced, status);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

int eprecon_simplify_quadrics_async(const float *verts, int64_t n, const int32_t *faces, int64_t m, const uint8_t *colors,
                                    const int64_t *key, const int32_t *corner_offsets, const int32_t *corner_order,
                                    const int32_t *member_offsets, const int32_t *member_order, int32_t n_clusters,
                                    const double *origin_host, double cell, double regularize, double *pos, float *normal, uint8_t *rgb,
                                    void *stream)
{
    Frame fr;
    if (n < 0 || m < 0 || n_clusters < 0 || !frame_of(origin_host, cell, fr) || !(regularize > 0.0) || !(regularize < 1e300) ||
        (colors && !rgb))
        return EPRECON_ERR_ARG;
    if (n > kMaxVertices || 3 * m > kMaxCorners || n_clusters > kMaxClusters) return EPRECON_ERR_UNSUPPORTED;
    if (n_clusters == 0) return EPRECON_OK;
    if (n == 0 || !verts || !key || !corner_offsets || !member_offsets || !member_order || !pos || !normal || (m > 0 && (!faces || !corner_order)))
        return EPRECON_ERR_ARG;
    hipLaunchKernelGGL(sm_quadrics_kernel, dim3((unsigned)ceil_div(n_clusters, 64)), dim3(64), 0, (hipStream_t)stream, verts, n, faces, m,
                       colors, reinterpret_cast<const long long *>(key), corner_offsets, corner_order, member_offsets, member_order,
                       (int)n_clusters, fr, regularize, pos, normal, colors ? rgb : (uint8_t *)nullptr);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
