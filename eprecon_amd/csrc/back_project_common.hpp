// Device helpers of the back-projection that more than one translation unit needs: the contract's projection and voxel centre
// (back_project.hip, back_project_backward.hip), the bilinear taps and their channel vectors (the scalar gather and its transpose),
// and the 64-pixel NCHW -> channels-last tile (back_project.hip, views_to_rows.hip).  Everything is inlined into its caller.
#pragma once

#include "common.hpp"

namespace ep {

struct Proj {
    float gx, gy, pz;
    bool vis;
};

// P: rows 0..2 of a 4x4 row-major projection (12 floats).  k-ordered fma chain == torch CPU bmm
// == fp32 MFMA accumulation order (see the oracle header for the evidence).
__device__ __forceinline__ Proj project(const float *P, float X, float Y, float Z, float wm1,
                                        float hm1)
{
    const float px = __fmaf_rn(P[3], 1.0f, __fmaf_rn(P[2], Z, __fmaf_rn(P[1], Y, __fmul_rn(P[0], X))));
    const float py = __fmaf_rn(P[7], 1.0f, __fmaf_rn(P[6], Z, __fmaf_rn(P[5], Y, __fmul_rn(P[4], X))));
    const float pz = __fmaf_rn(P[11], 1.0f, __fmaf_rn(P[10], Z, __fmaf_rn(P[9], Y, __fmul_rn(P[8], X))));
    const float u = __fdiv_rn(px, pz);
    const float v = __fdiv_rn(py, pz);
    Proj r;
    r.gx = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, u), wm1), 1.0f);
    r.gy = __fsub_rn(__fdiv_rn(__fmul_rn(2.0f, v), hm1), 1.0f);
    r.pz = pz;
    r.vis = (fabsf(r.gx) <= 1.0f) && (fabsf(r.gy) <= 1.0f) && (pz > 0.0f);
    return r;
}

__device__ __forceinline__ void voxel_centre(const int4 c, const float *origin, float vs, float &X,
                                             float &Y, float &Z)
{
    // float(c) * voxel_size + origin: separate multiply and add (models/occupancy_initialization.py:213)
    X = __fadd_rn(__fmul_rn((float)c.y, vs), origin[3 * c.x + 0]);
    Y = __fadd_rn(__fmul_rn((float)c.z, vs), origin[3 * c.x + 1]);
    Z = __fadd_rn(__fmul_rn((float)c.w, vs), origin[3 * c.x + 2]);
}

__device__ __forceinline__ void stage_matrices(float *sP, const float *krcam, int nmat, int tid,
                                               int nthreads)
{
    for (int i = tid; i < nmat * 12; i += nthreads) {
        const int m = i / 12, e = i - m * 12;
        sP[i] = krcam[m * 16 + e];
    }
}

struct Taps {
    int o00, o10, o01, o11;  // element offsets of the four taps inside one NHWC map (channel 0)
    float w00, w10, w01, w11;
};

__device__ __forceinline__ Taps make_taps(float ix, float iy, int W, int H, int C)
{
    const float x0f = floorf(ix), y0f = floorf(iy);
    int x0 = (int)x0f, y0 = (int)y0f;
    float wx1 = ix - x0f, wx0 = (x0f + 1.0f) - ix;
    float wy1 = iy - y0f, wy0 = (y0f + 1.0f) - iy;
    int x1 = x0 + 1, y1 = y0 + 1;
    // zero padding: a visible voxel has ix in [0, W-1], so only the +1 taps can leave the image,
    // and then only with weight exactly 0
    if (x1 >= W) { x1 = W - 1; wx1 = 0.0f; }
    if (y1 >= H) { y1 = H - 1; wy1 = 0.0f; }
    Taps t;
    t.o00 = (y0 * W + x0) * C;
    t.o10 = (y0 * W + x1) * C;
    t.o01 = (y1 * W + x0) * C;
    t.o11 = (y1 * W + x1) * C;
    t.w00 = wx0 * wy0;
    t.w10 = wx1 * wy0;
    t.w01 = wx0 * wy1;
    t.w11 = wx1 * wy1;
    return t;
}

template <int VEC>
struct Chan;
template <>
struct Chan<4> {
    float4 v;
    __device__ __forceinline__ static Chan zero() { return Chan{make_float4(0.f, 0.f, 0.f, 0.f)}; }
    __device__ __forceinline__ static Chan sample(const float *m, const Taps &t)
    {
        const float4 a = *reinterpret_cast<const float4 *>(m + t.o00);
        const float4 b = *reinterpret_cast<const float4 *>(m + t.o10);
        const float4 c = *reinterpret_cast<const float4 *>(m + t.o01);
        const float4 d = *reinterpret_cast<const float4 *>(m + t.o11);
        Chan r;
        r.v.x = fmaf(d.x, t.w11, fmaf(c.x, t.w01, fmaf(b.x, t.w10, a.x * t.w00)));
        r.v.y = fmaf(d.y, t.w11, fmaf(c.y, t.w01, fmaf(b.y, t.w10, a.y * t.w00)));
        r.v.z = fmaf(d.z, t.w11, fmaf(c.z, t.w01, fmaf(b.z, t.w10, a.z * t.w00)));
        r.v.w = fmaf(d.w, t.w11, fmaf(c.w, t.w01, fmaf(b.w, t.w10, a.w * t.w00)));
        return r;
    }
    __device__ __forceinline__ void add(const Chan &o) { v.x += o.v.x; v.y += o.v.y; v.z += o.v.z; v.w += o.v.w; }
    __device__ __forceinline__ void add_sqdiff(const Chan &f, const Chan &mean)
    {
        const float dx = f.v.x - mean.v.x, dy = f.v.y - mean.v.y, dz = f.v.z - mean.v.z, dw = f.v.w - mean.v.w;
        v.x = fmaf(dx, dx, v.x); v.y = fmaf(dy, dy, v.y); v.z = fmaf(dz, dz, v.z); v.w = fmaf(dw, dw, v.w);
    }
    __device__ __forceinline__ Chan div(float d) const
    {
        return Chan{make_float4(__fdiv_rn(v.x, d), __fdiv_rn(v.y, d), __fdiv_rn(v.z, d), __fdiv_rn(v.w, d))};
    }
    __device__ __forceinline__ void store(float *dst, bool aligned16) const
    {
        if (aligned16) {
            *reinterpret_cast<float4 *>(dst) = v;
        } else {
            dst[0] = v.x; dst[1] = v.y; dst[2] = v.z; dst[3] = v.w;
        }
    }
};
template <>
struct Chan<1> {
    float v;
    __device__ __forceinline__ static Chan zero() { return Chan{0.f}; }
    __device__ __forceinline__ static Chan sample(const float *m, const Taps &t)
    {
        return Chan{fmaf(m[t.o11], t.w11, fmaf(m[t.o01], t.w01, fmaf(m[t.o10], t.w10, m[t.o00] * t.w00)))};
    }
    __device__ __forceinline__ void add(const Chan &o) { v += o.v; }
    __device__ __forceinline__ void add_sqdiff(const Chan &f, const Chan &mean)
    {
        const float d = f.v - mean.v;
        v = fmaf(d, d, v);
    }
    __device__ __forceinline__ Chan div(float d) const { return Chan{__fdiv_rn(v, d)}; }
    __device__ __forceinline__ void store(float *dst, bool) const { dst[0] = v; }
};

// ---------------------------------------------------------------------------------------------
// NCHW -> NHWC through an LDS tile: reads coalesced along H*W, writes coalesced along (pixel, C)
// ---------------------------------------------------------------------------------------------
constexpr int kTrPix = 64;
// One 64-pixel tile of one map.  VEC4 (hw % 4 == 0, Cs % 4 == 0, 16-byte aligned bases): 16 bytes per lane on both sides -- four
// pixels of one channel in, four channels of one pixel out; otherwise 4 bytes per lane.  A copy either way: the same bits.
template <bool VEC4>
__device__ __forceinline__ void relayout_body(char *smem, const float *__restrict__ in, float *__restrict__ out, int C, int hw,
                                              int Cs, int map, int p0)
{
    float *tile = reinterpret_cast<float *>(smem);  // [C][kTrPix + 1]
    const int npix = min(kTrPix, hw - p0);
    const float *src = in + (size_t)map * C * hw;
    float *dst = out + (size_t)map * hw * Cs + (size_t)p0 * Cs;
    if constexpr (VEC4) {
        constexpr int G = kTrPix / 4;
        for (int e = threadIdx.x; e < C * G; e += 256) {
            const int c = e / G, px = (e - c * G) * 4;
            if (px < npix) {   // (npix is a multiple of 4 here: px + 3 < npix)
                const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)c * hw + p0 + px);
                float *t = tile + c * (kTrPix + 1) + px;
                t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
            }
        }
        __syncthreads();
        const int Q = Cs / 4;
        for (int e = threadIdx.x; e < npix * Q; e += 256) {  // pad channels (Cs > C) are written as zeros
            const int px = e / Q, c = (e - px * Q) * 4;
            const float *t = tile + c * (kTrPix + 1) + px;
            float4 v;
            v.x = c + 0 < C ? t[0 * (kTrPix + 1)] : 0.0f;
            v.y = c + 1 < C ? t[1 * (kTrPix + 1)] : 0.0f;
            v.z = c + 2 < C ? t[2 * (kTrPix + 1)] : 0.0f;
            v.w = c + 3 < C ? t[3 * (kTrPix + 1)] : 0.0f;
            reinterpret_cast<float4 *>(dst)[e] = v;
        }
    } else {
        for (int e = threadIdx.x; e < C * kTrPix; e += 256) {
            const int c = e / kTrPix, px = e - c * kTrPix;
            if (px < npix) tile[c * (kTrPix + 1) + px] = src[(size_t)c * hw + p0 + px];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < npix * Cs; e += 256) {  // pad channels (Cs > C) are written as zeros
            const int px = e / Cs, c = e - px * Cs;
            dst[e] = c < C ? tile[c * (kTrPix + 1) + px] : 0.0f;
        }
    }
}

inline bool relayout_vec4(const void *in, const void *out, int hw, int Cs)
{
    return hw % 4 == 0 && Cs % 4 == 0 && (((uintptr_t)in | (uintptr_t)out) & 15) == 0;
}

}  // namespace ep
