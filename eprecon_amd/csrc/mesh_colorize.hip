// Vertex colours from the video on gfx950: the pixels of posed colour frames carried onto the vertices of a mesh — the
// reference has only a commented-out colour path in its ground-truth fusion; driven by eprecon_amd/colorize.py.
//
//   colorize_accumulate   acc f64[N,4] += (w r, w g, w b, w), seen int32[N] += 1 per (vertex, view) pair that is kept
//   colorize_finish       rgb u8[N,3] = min(255, floor(acc_c / acc_w + 0.5)) where seen >= min_views, else the fallback
//
// The rule (fp64 throughout, sums associated as in mesh_raster.hpp), per vertex i and view v:
//   1. q = w2c_v p_i (point_camera), z = q.z; kept only if znear <= z <= zfar.
//   2. Occlusion against the mesh's own visibility buffer u64[V,Hd,Wd] (render_visibility) with intrinsics K_vis:
//      (u_d, v_d) = project_point(K_vis, q), cd = floor(u_d - pixel_center + 0.5), rd likewise, both inside the buffer; the
//      word there is a hit (upper word < 0x7F800000, the face index a drawable face: resolve's tests) and, with D its fp32
//      depth, z <= D + tolerance.
//   3. Facing from the face that won that pixel, rebuilt in the camera frame (tri_camera, tri_planes): n its plane normal,
//      cos = |n.q| / (|n| |q|); kept only if |n| > 0 and cos >= min_cos.  No per-vertex normal is read.
//   4. (u_c, v_c) = project_point(K_color, q), x = u_c - pixel_center, y = v_c - pixel_center; kept only if
//      0 <= x <= Wc-1 and 0 <= y <= Hc-1.  x0 = min(floor(x), Wc-2), fx = x - x0, the same for y; per channel
//      top = (1-fx) c00 + fx c01, bottom = (1-fx) c10 + fx c11, value = (1-fy) top + fy bottom.
//   5. w = cos / z^2; acc += (w value_r, w value_g, w value_b, w); seen += 1.
//
// One thread per vertex loops the views of the call in ascending order with the running sums in registers: acc and seen are
// read once before the first view and written once after the last, so the sums are one sequential chain per vertex — no
// atomics, bit-identical run to run and however the views are split into calls.  The camera block of the launch (K_color,
// K_vis, the w2c of its views) is staged in LDS.  A wave none of whose vertices lands inside the visibility buffer of a view
// skips that view with one uniform branch.  The frame reads are scattered 2 x 2 x 3-byte gathers.
#include "mesh_raster.hpp"

namespace {
using namespace ep;
using namespace ep_raster;

constexpr int kBlock = 256;
constexpr int kMaxViews = 64;    // views per launch: (18 + 12 * 64) doubles of LDS; an entry call of more views launches again

struct ColorParams {
    const uint8_t *frames;              // [V,hc,wc,3] of this launch's views
    const unsigned long long *vis;      // [V,hd,wd] of this launch's views
    int view0;                          // first view of this launch in the call's camera block
    int hc, wc, hd, wd;
    double tolerance, min_cos;
    double *acc;                        // [N,4]
    int32_t *seen;                      // [N]
};

__global__ __launch_bounds__(kBlock) void colorize_accumulate_kernel(RenderParams P, ColorParams C)
{
    // K_color[9], K_vis[9], then the w2c[12] of views view0 .. view0 + n_views - 1: tri_camera's layout (K, K^-1, views)
    __shared__ double cams[18 + 12 * kMaxViews];
    for (int k = threadIdx.x; k < 18 + 12 * P.n_views; k += kBlock)
        cams[k] = P.cams[k < 18 ? k : k + 12 * C.view0];
    __syncthreads();
    P.cams = cams;

    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool live = i < P.n_verts;
    const int64_t row = live ? i : 0;                  // (n_verts >= 1: the entry launches nothing for an empty mesh)
    const float *p = P.verts + 3 * (size_t)row;
    double sum[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) sum[k] = C.acc[4 * (size_t)row + k];
    int count = C.seen[row];

    const double pc = (double)P.pixel_center, znear = (double)P.znear, zfar = (double)P.zfar;
    for (int view = 0; view < P.n_views; ++view) {
        double q[3];
        point_camera(cams + 18 + 12 * view, p, q);
        double ud, vd;
        project_point(cams + 9, q, ud, vd);
        const double cd = floor(ud - pc + 0.5), rd = floor(vd - pc + 0.5);
        const bool inside = live && q[2] >= znear && q[2] <= zfar && cd >= 0.0 && cd <= (double)(C.wd - 1) && rd >= 0.0 &&
                            rd <= (double)(C.hd - 1);
        if (__ballot(inside) == 0ull) continue;        // wave-uniform: nothing of this wave lands in the view
        if (!inside) continue;
        const unsigned long long key = C.vis[((size_t)view * C.hd + (size_t)(int)rd) * C.wd + (size_t)(int)cd];
        const unsigned bits = (unsigned)(key >> 32);
        const int64_t tri = (int64_t)(key & 0xffffffffull);
        int32_t id[3];
        double tv[3][3];
        // (a word that names no drawable face is "no hit", as in resolve: it must not index past the mesh)
        if (!(bits < kInfBits && tri < P.n_faces && tri_camera(P, view, tri, id, tv))) continue;
        if (!(q[2] <= (double)__uint_as_float(bits) + C.tolerance)) continue;
        TriSetup T;
        tri_planes(tv, T);
        const double nlen = sqrt(dot3(T.n, T.n));
        const double cosine = fabs(dot3(T.n, q)) / (nlen * sqrt(dot3(q, q)));
        if (!(nlen > 0.0 && cosine >= C.min_cos)) continue;
        double uc, vc;
        project_point(cams, q, uc, vc);
        const double x = uc - pc, y = vc - pc;
        if (!(x >= 0.0 && x <= (double)(C.wc - 1) && y >= 0.0 && y <= (double)(C.hc - 1))) continue;
        const double x0 = fmin(floor(x), (double)(C.wc - 2)), y0 = fmin(floor(y), (double)(C.hc - 2));
        const double fx = x - x0, fy = y - y0;
        const uint8_t *top = C.frames + (((size_t)view * C.hc + (size_t)(int)y0) * C.wc + (size_t)(int)x0) * 3;
        const uint8_t *bottom = top + (size_t)C.wc * 3;
        const double w = cosine / (q[2] * q[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = (1.0 - fx) * (double)top[k] + fx * (double)top[3 + k];
            const double b = (1.0 - fx) * (double)bottom[k] + fx * (double)bottom[3 + k];
            sum[k] += w * ((1.0 - fy) * a + fy * b);
        }
        sum[3] += w;
        ++count;
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < 4; ++k) C.acc[4 * (size_t)i + k] = sum[k];
    C.seen[i] = count;
}

struct FinishParams {
    const double *acc;
    const int32_t *seen;
    int64_t n;
    int min_views;
    uint8_t fallback[3];
    uint8_t *rgb;
};

__global__ __launch_bounds__(kBlock) void colorize_finish_kernel(FinishParams F)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= F.n) return;
    const double w = F.acc[4 * (size_t)i + 3];
    const bool coloured = F.seen[i] >= F.min_views && w > 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        F.rgb[3 * (size_t)i + k] = coloured ? (uint8_t)fmin(255.0, floor(F.acc[4 * (size_t)i + k] / w + 0.5)) : F.fallback[k];
}

}  // namespace

extern "C" {

int eprecon_colorize_accumulate_async(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *cams,
                                      int n_views, const uint8_t *frames, int hc, int wc, const uint64_t *vis, int hd, int wd,
                                      float pixel_center, float znear, float zfar, double tolerance, double min_cos, double *acc,
                                      int32_t *seen, void *stream)
{
    if (n_verts < 0 || n_faces < 0 || n_views < 0 || n_verts > 0x7fffffffll || n_faces > 0x7fffffffll || hc < 2 || wc < 2 ||
        hd < 1 || wd < 1 || !(znear > 0.0f) || !(zfar >= znear) || !(tolerance >= 0.0) || !(min_cos >= 0.0 && min_cos <= 1.0))
        return EPRECON_ERR_ARG;
    if (n_verts == 0 || n_views == 0) return EPRECON_OK;
    if (!verts || !cams || !frames || !vis || !acc || !seen || (n_faces > 0 && !faces)) return EPRECON_ERR_ARG;
    const unsigned long long *words = reinterpret_cast<const unsigned long long *>(vis);
    for (int v0 = 0; v0 < n_views; v0 += kMaxViews) {
        const int nv = n_views - v0 < kMaxViews ? n_views - v0 : kMaxViews;
        RenderParams P{verts, faces, cams, n_verts, n_faces, nv, hd, wd, pixel_center, znear, zfar, 0,
                       nullptr, nullptr, nullptr, 0};
        ColorParams C{frames + (size_t)v0 * hc * wc * 3, words + (size_t)v0 * hd * wd, v0, hc, wc, hd, wd, tolerance, min_cos,
                      acc, seen};
        hipLaunchKernelGGL(colorize_accumulate_kernel, dim3((unsigned)ceil_div(n_verts, kBlock)), dim3(kBlock), 0,
                           (hipStream_t)stream, P, C);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

int eprecon_colorize_finish_async(const double *acc, const int32_t *seen, int64_t n, int min_views, int fallback_red,
                                  int fallback_green, int fallback_blue, uint8_t *rgb_out, void *stream)
{
    if (n < 0 || n > 0x7fffffffll || fallback_red < 0 || fallback_red > 255 || fallback_green < 0 || fallback_green > 255 ||
        fallback_blue < 0 || fallback_blue > 255)
        return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    if (!acc || !seen || !rgb_out) return EPRECON_ERR_ARG;
    FinishParams F{acc, seen, n, min_views, {(uint8_t)fallback_red, (uint8_t)fallback_green, (uint8_t)fallback_blue}, rgb_out};
    hipLaunchKernelGGL(colorize_finish_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, F);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
