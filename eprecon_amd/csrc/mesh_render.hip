// View rendering on gfx950: which triangle every pixel of every camera sees, and what hangs on that (labels, shading) —
// the reference's tools/render.py and VIS_INCREMENTAL open a pyrender window; driven by eprecon_amd/render.py.
//
//   render_visibility   u64[V,H,W]: (fp32 depth bits << 32) | face index of the nearest triangle; all-ones where none
//   render_resolve      depth, face, nearest corner, per-vertex labels at that corner and flat shading per pixel
//
// Visibility walks (triangle, view) pairs exactly as the depth render does (mesh_raster.hpp: the same setup, coverage and
// depth expressions, the same queue for large pixel boxes); a hit lowers the pixel's word with one 64-bit atomicMin
// (global_atomic_umin_x2 on gfx950, no compare-and-swap loop).  A min: bit-identical run to run; its upper half is the
// depth render's z-buffer bit for bit; at equal depth bits the smallest face index wins.
//
// Resolve is one thread per pixel: it rebuilds the winning triangle in the camera frame with the rasteriser's own fp64
// expressions and weighs the corners by the three triple products the coverage test used,
//   w_a : w_b : w_c = d.(b x c) : d.(c x a) : d.(a x b)      (perspective-correct barycentric weights of the ray d)
// The pixel takes the id of the corner with the largest |w| (the earlier slot of the face on ties): ids are never
// interpolated.  Flat shading: I = ambient + (1 - ambient) |n^ . d^| with the unit face normal and the
// unit pixel ray in fp64, channel = min(255, floor(c I + 0.5)) with c the uint8 colour of that corner's vertex.
#include "mesh_raster.hpp"

namespace {
using namespace ep;
using namespace ep_raster;

struct VisSink {
    unsigned long long *vis;
    int height, width;
    __device__ __forceinline__ void operator()(int view, int64_t tri, int r, int c, unsigned bits) const
    {
        unsigned long long *dst = vis + ((size_t)view * height + r) * width + c;
        const unsigned long long key = ((unsigned long long)bits << 32) | (unsigned long long)tri;
        if (key < *dst) atomicMin(dst, key);
    }
};

__global__ __launch_bounds__(256) void visibility_tri_kernel(RenderParams P, unsigned long long *vis)
{
    raster_tri(P, VisSink{vis, P.height, P.width});
}

__global__ __launch_bounds__(256) void visibility_queue_kernel(RenderParams P, unsigned long long *vis)
{
    raster_queue(P, VisSink{vis, P.height, P.width});
}

struct ResolveParams {
    const unsigned long long *vis;
    float *depth;
    int32_t *face, *corner;
    const int32_t *labels[2];
    int32_t background[2];
    int32_t *label_out[2];
    const uint8_t *colors;     // [n_verts,3] or null (kDefaultColor)
    double ambient;
    uint8_t background_rgb[3];
    uint8_t *rgb;              // [V,H,W,3]
};

constexpr double kDefaultColor = 153.0;    // the reference's baseColorFactor 0.6

__device__ __forceinline__ uint8_t shade_channel(double c, double intensity)
{
    return (uint8_t)fmin(255.0, floor(c * intensity + 0.5));
}

__global__ __launch_bounds__(256) void resolve_kernel(RenderParams P, ResolveParams R)
{
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per_view = (int64_t)P.height * P.width;
    if (pix >= per_view * P.n_views) return;
    const unsigned long long key = R.vis[pix];
    const unsigned bits = (unsigned)(key >> 32);
    const int64_t tri = (int64_t)(key & 0xffffffffull);
    const int view = (int)(pix / per_view);
    const int rem = (int)(pix % per_view), r = rem / P.width, c = rem % P.width;
    int32_t id[3];
    double v[3][3];
    // (a word that names no drawable face is "no hit": a buffer this mesh did not produce must not index past it)
    const bool hit = bits < kInfBits && tri < P.n_faces && tri_camera(P, view, tri, id, v);
    int32_t best = -1;
    double intensity = 1.0;
    if (hit) {
        TriSetup T;
        tri_planes(v, T);
        double d[3];
        pixel_ray(P, r, c, d);
        const double wa = fabs(dot3(T.e1, d)), wb = fabs(dot3(T.e2, d)), wc = fabs(dot3(T.e0, d));
        int slot = 0;
        double wmax = wa;
        if (wb > wmax) {
            slot = 1;
            wmax = wb;
        }
        if (wc > wmax) slot = 2;
        best = slot == 0 ? id[0] : (slot == 1 ? id[1] : id[2]);
        if (R.rgb) {
            const double cosine = fabs(dot3(T.n, d)) / (sqrt(dot3(T.n, T.n)) * sqrt(dot3(d, d)));
            intensity = R.ambient + (1.0 - R.ambient) * cosine;
        }
    }
    if (R.depth) R.depth[pix] = hit ? __uint_as_float(bits) : 0.0f;
    if (R.face) R.face[pix] = hit ? (int32_t)tri : -1;
    if (R.corner) R.corner[pix] = best;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (R.label_out[k]) R.label_out[k][pix] = hit ? R.labels[k][best] : R.background[k];
    if (R.rgb) {
        uint8_t *o = R.rgb + 3 * (size_t)pix;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double col = R.colors && hit ? (double)R.colors[3 * (size_t)best + k] : kDefaultColor;
            o[k] = hit ? shade_channel(col, intensity) : R.background_rgb[k];
        }
    }
}

}  // namespace

extern "C" {

size_t eprecon_render_visibility_workspace_bytes(int64_t queue_capacity) { return raster_workspace_bytes(queue_capacity); }

int eprecon_render_visibility_async(const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces, const double *cams,
                                    int n_views, int height, int width, float pixel_center, float znear, float zfar,
                                    int cull_back, uint64_t *vis_out, int64_t queue_capacity, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (!vis_out || !workspace ||
        !raster_args_ok(verts, n_verts, faces, n_faces, cams, n_views, height, width, znear, zfar, queue_capacity))
        return EPRECON_ERR_ARG;
    if (workspace_bytes < raster_workspace_bytes(queue_capacity)) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    RenderParams P{verts, faces, cams, n_verts, n_faces, n_views, height, width, pixel_center, znear, zfar, cull_back,
                   nullptr, reinterpret_cast<unsigned *>(ws), reinterpret_cast<unsigned long long *>(ws + 256), queue_capacity};
    unsigned long long *vis = reinterpret_cast<unsigned long long *>(vis_out);
    const int64_t n_pix = (int64_t)n_views * height * width;
    EP_HIP_CHECK(hipMemsetAsync(P.queue_count, 0, sizeof(unsigned), st));
    EP_HIP_CHECK(hipMemsetAsync(vis, 0xFF, (size_t)n_pix * sizeof(unsigned long long), st));
    if (n_faces > 0) {
        hipLaunchKernelGGL(visibility_tri_kernel, dim3((unsigned)ceil_div(n_faces, 256), (unsigned)n_views), dim3(256), 0, st, P,
                           vis);
        EP_LAUNCH_CHECK();
        hipLaunchKernelGGL(visibility_queue_kernel, dim3(2048), dim3(256), 0, st, P, vis);
        EP_LAUNCH_CHECK();
    }
    return EPRECON_OK;
}

int eprecon_render_resolve_async(const uint64_t *vis, const float *verts, int64_t n_verts, const int32_t *faces, int64_t n_faces,
                                 const double *cams, int n_views, int height, int width, float pixel_center, float *depth_out,
                                 int32_t *face_out, int32_t *corner_out, const int32_t *labels_a, int32_t background_a,
                                 int32_t *label_a_out, const int32_t *labels_b, int32_t background_b, int32_t *label_b_out,
                                 const uint8_t *colors, double ambient, int bg_red, int bg_green, int bg_blue,
                                 uint8_t *rgb_out, void *stream)
{
    if (!vis || !cams || n_views < 1 || height < 1 || width < 1 || n_faces < 0 || n_verts < 0 || n_faces > 0x7fffffffll ||
        (n_faces > 0 && (!verts || !faces)) || (label_a_out && !labels_a && n_faces > 0) ||
        (label_b_out && !labels_b && n_faces > 0) || !(ambient >= 0.0 && ambient <= 1.0) || bg_red < 0 ||
        bg_red > 255 || bg_green < 0 || bg_green > 255 || bg_blue < 0 || bg_blue > 255)
        return EPRECON_ERR_ARG;
    const int64_t n_pix = (int64_t)n_views * height * width;
    if (n_pix > 0x7fffffffll * 256) return EPRECON_ERR_UNSUPPORTED;
    RenderParams P{verts, faces, cams, n_verts, n_faces, n_views, height, width, pixel_center, 0.0f, 0.0f, 0,
                   nullptr, nullptr, nullptr, 0};
    ResolveParams R{reinterpret_cast<const unsigned long long *>(vis), depth_out, face_out, corner_out, {labels_a, labels_b},
                    {background_a, background_b}, {label_a_out, label_b_out}, colors, ambient,
                    {(uint8_t)bg_red, (uint8_t)bg_green, (uint8_t)bg_blue}, rgb_out};
    hipLaunchKernelGGL(resolve_kernel, dim3((unsigned)ceil_div(n_pix, 256)), dim3(256), 0, (hipStream_t)stream, P, R);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

}  // extern "C"
