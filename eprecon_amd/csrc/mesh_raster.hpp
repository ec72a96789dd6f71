// Triangle rasteriser shared by the depth render (mesh_eval.hip) and the visibility buffer (mesh_render.hip); its point and
// triangle expressions (point_camera, project_point, tri_camera, tri_planes) also serve vertex colouring (mesh_colorize.hip).
//
// One thread per (triangle, view) in a 2D grid (y = view) transforms its triangle into the camera (fp64), culls it, and
// sizes its pixel box.  A box of at most kSmallBox pixels is walked by that thread; a larger one goes to a queue that a
// second launch walks with a whole wave per entry (64 lanes stride the box), so that the few triangles near the camera do
// not serialise one thread over thousands of pixels.  Coverage is decided per pixel in camera space by the signs of the
// ray's triple products with the three edge planes through the camera centre — exact for triangles that cross the near
// plane or lie partly behind the camera, with no clipping of the triangle; only its pixel box is taken from the part in
// front of z = znear (a box of the whole image for every triangle that crosses the camera plane made those few hundred
// triangles per view the largest cost of a room scene).  The depth is the ray / plane intersection.
//
// What a covered pixel does with its depth is the including unit's: `raster_tri` and `raster_queue` hand every hit
// (view, triangle, row, column, fp32 depth bits) to a sink; the unit's __global__ kernels call them.
#pragma once

#include <math.h>

#include "common.hpp"

namespace ep_raster {
using namespace ep;

constexpr int kSmallBox = 64;          // pixel boxes up to this size stay with their (triangle, view) thread
constexpr unsigned kInfBits = 0x7F800000u;

struct RenderParams {
    const float *verts;
    const int32_t *faces;
    const double *cams;      // K[9], K^-1[9], per view w2c[12]
    int64_t n_verts, n_faces;
    int n_views, height, width;
    float pixel_center, znear, zfar;
    int cull_back;
    unsigned *zbuf;          // [V,H,W] fp32 bits (depth render)
    unsigned *queue_count;
    unsigned long long *queue;
    int64_t queue_capacity;
};

struct TriSetup {
    double e0[3], e1[3], e2[3];   // edge-plane normals a x b, b x c, c x a
    double n[3], nd;              // plane normal (b-a) x (c-a) and n . a
    int c_lo, c_hi, r_lo, r_hi;   // pixel box (inclusive)
};

__device__ __forceinline__ void cross3(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ double dot3(const double *a, const double *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ int clamp_pix(double v, int hi) { return (int)fmin(fmax(v, -1.0), (double)hi + 1.0); }

// the f32 world point p, widened, in the camera frame of the world->camera 3x4 M
__device__ __forceinline__ void point_camera(const double *M, const float *p, double q[3])
{
    const double x = p[0], y = p[1], z = p[2];
#pragma unroll
    for (int r = 0; r < 3; ++r) q[r] = ((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3];
}

// image point of the camera-frame point q under K (last row 0 0 1): the homogeneous coordinates times 1 / z
__device__ __forceinline__ void project_point(const double *K, const double *q, double &px, double &py)
{
    const double iz = 1.0 / q[2];
    px = ((K[0] * q[0] + K[1] * q[1]) + K[2] * q[2]) * iz;
    py = ((K[3] * q[0] + K[4] * q[1]) + K[5] * q[2]) * iz;
}

// corners of triangle `tri` in the camera frame of `view`; false: a vertex index out of range (the face is never drawn)
__device__ __forceinline__ bool tri_camera(const RenderParams &P, int view, int64_t tri, int32_t id[3], double v[3][3])
{
    id[0] = P.faces[3 * tri];
    id[1] = P.faces[3 * tri + 1];
    id[2] = P.faces[3 * tri + 2];
    if (id[0] < 0 || id[1] < 0 || id[2] < 0 || id[0] >= P.n_verts || id[1] >= P.n_verts || id[2] >= P.n_verts) return false;
    const double *M = P.cams + 18 + 12 * (size_t)view;
#pragma unroll
    for (int k = 0; k < 3; ++k) point_camera(M, P.verts + 3 * (size_t)id[k], v[k]);
    return true;
}

// plane and edge planes of a camera-frame triangle
__device__ __forceinline__ void tri_planes(const double v[3][3], TriSetup &T)
{
    const double u[3] = {v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2]};
    const double w[3] = {v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2]};
    cross3(u, w, T.n);
    T.nd = dot3(T.n, v[0]);
    cross3(v[0], v[1], T.e0);
    cross3(v[1], v[2], T.e1);
    cross3(v[2], v[0], T.e2);
}

// ray through pixel (r, c) in the camera frame (z component 1 for K with last row 0 0 1)
__device__ __forceinline__ void pixel_ray(const RenderParams &P, int r, int c, double d[3])
{
    const double *Ki = P.cams + 9;
    const double pu = (double)c + (double)P.pixel_center, pv = (double)r + (double)P.pixel_center;
    d[0] = (Ki[0] * pu + Ki[1] * pv) + Ki[2];
    d[1] = (Ki[3] * pu + Ki[4] * pv) + Ki[5];
    d[2] = (Ki[6] * pu + Ki[7] * pv) + Ki[8];
}

// false: the triangle draws nothing in this view
static __device__ bool tri_setup(const RenderParams &P, int view, int64_t tri, TriSetup &T)
{
    int32_t id[3];
    double v[3][3];
    if (!tri_camera(P, view, tri, id, v)) return false;
    const double *K = P.cams;
    const double zmin = fmin(v[0][2], fmin(v[1][2], v[2][2])), zmax = fmax(v[0][2], fmax(v[1][2], v[2][2]));
    if (zmax < (double)P.znear || zmin > (double)P.zfar) return false;
    tri_planes(v, T);
    if (T.nd == 0.0) return false;                     // degenerate, or its plane passes through the camera
    if (P.cull_back && !(T.nd < 0.0)) return false;    // back face
    // pixel box: the projection of the part of the triangle with z >= znear (the corners in front, plus the points where
    // the edges cross z = znear), one pixel of slack — only the box is clipped, the exact per-pixel test decides coverage
    const double pc = (double)P.pixel_center, zn = (double)P.znear;
    double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300;
    auto add = [&](const double *q) {
        double px, py;
        project_point(K, q, px, py);
        umin = fmin(umin, px); umax = fmax(umax, px); vmin = fmin(vmin, py); vmax = fmax(vmax, py);
    };
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double *a = v[k], *b = v[(k + 1) % 3];
        if (a[2] >= zn) add(a);
        if ((a[2] < zn) != (b[2] < zn)) {
            const double t = (zn - a[2]) / (b[2] - a[2]);
            const double q[3] = {a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), zn};
            add(q);
        }
    }
    T.c_lo = max(clamp_pix(ceil(umin - pc) - 1.0, P.width), 0);
    T.c_hi = min(clamp_pix(floor(umax - pc) + 1.0, P.width), P.width - 1);
    T.r_lo = max(clamp_pix(ceil(vmin - pc) - 1.0, P.height), 0);
    T.r_hi = min(clamp_pix(floor(vmax - pc) + 1.0, P.height), P.height - 1);
    return T.c_lo <= T.c_hi && T.r_lo <= T.r_hi;
}

// coverage and depth of pixel (r, c): true when the ray hits the triangle inside [znear, zfar]; bits = its fp32 depth
__device__ __forceinline__ bool cover_depth(const RenderParams &P, const TriSetup &T, int r, int c, unsigned &bits)
{
    double d[3];
    pixel_ray(P, r, c, d);
    const double s0 = dot3(T.e0, d), s1 = dot3(T.e1, d), s2 = dot3(T.e2, d);
    const bool covered = (s0 >= 0.0 && s1 >= 0.0 && s2 >= 0.0) || (s0 <= 0.0 && s1 <= 0.0 && s2 <= 0.0);
    if (!covered) return false;
    const double den = dot3(T.n, d);
    if (den == 0.0) return false;
    const double z = T.nd / den * d[2];
    if (!(z >= (double)P.znear && z <= (double)P.zfar)) return false;
    bits = __float_as_uint((float)z);
    return true;
}

// body of the one-thread-per-(triangle, view) launch (256 threads, grid y = view): sink(view, tri, r, c, bits) per hit
template <class Sink>
__device__ __forceinline__ void raster_tri(const RenderParams &P, const Sink &sink)
{
    const int64_t tri = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int view = blockIdx.y;
    if (tri >= P.n_faces) return;
    TriSetup T;
    if (!tri_setup(P, view, tri, T)) return;
    const int bw = T.c_hi - T.c_lo + 1, area = bw * (T.r_hi - T.r_lo + 1);
    if (area > kSmallBox) {
        const unsigned slot = atomicAdd(P.queue_count, 1u);
        if ((int64_t)slot < P.queue_capacity) {
            P.queue[slot] = ((unsigned long long)view << 32) | (unsigned long long)tri;
            return;
        }
        // (queue full: this thread walks the box itself — slower, same result)
    }
    for (int k = 0; k < area; ++k) {
        const int r = T.r_lo + k / bw, c = T.c_lo + k % bw;
        unsigned bits;
        if (cover_depth(P, T, r, c, bits)) sink(view, tri, r, c, bits);
    }
}

// body of the queue launch (256 threads): one wave per queued (view, triangle), its 64 lanes stride the pixel box
template <class Sink>
__device__ __forceinline__ void raster_queue(const RenderParams &P, const Sink &sink)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_waves = (int64_t)gridDim.x * (256 / kWave);
    const int64_t count = min((int64_t)*P.queue_count, P.queue_capacity);
    for (int64_t e = (int64_t)blockIdx.x * (256 / kWave) + threadIdx.x / kWave; e < count; e += n_waves) {
        const unsigned long long q = P.queue[e];
        const int view = (int)(q >> 32);
        const int64_t tri = (int64_t)(q & 0xffffffffull);
        TriSetup T;
        if (!tri_setup(P, view, tri, T)) continue;    // (wave-uniform: every lane set up the same triangle)
        const int bw = T.c_hi - T.c_lo + 1, area = bw * (T.r_hi - T.r_lo + 1);
        for (int k = lane; k < area; k += kWave) {
            const int r = T.r_lo + k / bw, c = T.c_lo + k % bw;
            unsigned bits;
            if (cover_depth(P, T, r, c, bits)) sink(view, tri, r, c, bits);
        }
    }
}

inline size_t raster_workspace_bytes(int64_t queue_capacity)
{
    return 256 + align_up((size_t)(queue_capacity > 0 ? queue_capacity : 0) * 8, 256);
}

// argument rules both entries share
inline bool raster_args_ok(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *cams,
                           int n_views, int height, int width, float znear, float zfar, int64_t queue_capacity)
{
    return cams && n_views >= 1 && n_views <= 65535 && height >= 1 && width >= 1 && n_faces >= 0 && n_verts >= 0 &&
           n_faces <= 0x7fffffffll && queue_capacity >= 0 && znear > 0.0f && zfar >= znear && (n_faces == 0 || (verts && faces));
}

}  // namespace ep_raster
