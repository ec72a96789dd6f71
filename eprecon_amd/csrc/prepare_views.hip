// View preparation on gfx950: a fragment's decoded colour frames -> the f32[V,3,h,w] tensor the network takes, and its depth
// frames -> metres.
//
// Replaces, per fragment, the host loop of                                   datasets/transforms.py ResizeImage + ToTensor
//   V x { centre the frame on a 4:3 canvas, PIL resize(BILINEAR), float copy, transpose }  and  datasets/scannet.py:57-63.
// PIL's 8-bit resampling is integer arithmetic once its coefficient tables are known (include/eprecon_hip.h states it), so
// the result here is PIL's bit for bit; the tables are built on the host in float64 (eprecon_amd/transforms.py).
//
// prepare_views_kernel: a workgroup of 256 owns a 64 x 16 tile of output pixels of one view.
//   1. horizontal pass: for every source row of the tile's vertical window (rows r0 .. r1 of the padded frame, from table_y)
//      the tile's 64 output columns x 3 channels, straight from global memory (a wave reads ~64 * scale * 3 consecutive
//      bytes of one row) into LDS as bytes, planar [row][channel][64].  Thread t keeps column t % 64 throughout, so its
//      taps and coefficients sit in registers.  Rows outside the frame are the canvas's black rows: 0, never read.
//   2. vertical pass from LDS: thread t, column t % 64, output rows t / 64 + 4 j; three coalesced float stores, one per
//      channel plane.
// At the production ratio 2.025 the window is 35 rows, 6.7 KB of LDS.  The traffic it must move is one read of the frames
// and one write of the output; what it waits on is the issue of the horizontal pass's byte loads (DESIGN.md 7ad has the
// figures).  Every table entry is range-checked where it is used: a tap outside the frame or the window is skipped.
#include "common.hpp"

namespace {
using namespace ep;

constexpr int kTileW = EPRECON_VIEWS_TILE_W, kTileH = EPRECON_VIEWS_TILE_H, kMaxK = EPRECON_VIEWS_MAX_KSIZE;
constexpr int kBlock = 256, kRowStep = kBlock / kTileW;
constexpr int kPrecision = 22;
static_assert(kBlock % kTileW == 0 && kTileH % kRowStep == 0, "a thread keeps its column; the rows divide among the threads");

struct PrepareViewsArgs {
    const uint8_t *frames;
    const int32_t *table_x, *table_y;
    float *out;
    int height, width, pad_top, ksize_x, ksize_y, lds_rows, out_h, out_w;
};

__device__ __forceinline__ int clip8(int acc)
{
    const int v = acc >> kPrecision;      // arithmetic shift
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(kBlock) void prepare_views_kernel(PrepareViewsArgs a)
{
    extern __shared__ uint8_t hbuf[];     // [rows][3][kTileW]
    const int tid = threadIdx.x, col = tid % kTileW, sub = tid / kTileW;
    const int view = blockIdx.z, oy0 = blockIdx.y * kTileH, ox = blockIdx.x * kTileW + col;
    const int oy_end = min(oy0 + kTileH, a.out_h);
    const int stride_x = 2 + a.ksize_x, stride_y = 2 + a.ksize_y;
    const int r0 = a.table_y[(size_t)oy0 * stride_y];
    const int32_t *last = a.table_y + (size_t)(oy_end - 1) * stride_y;
    const int rows = max(0, min(last[0] + last[1] - r0, a.lds_rows));

    // ---- horizontal pass: this thread's column, its taps in registers
    int xmin = 0, n = 0, k[kMaxK];
    if (ox < a.out_w) {
        const int32_t *t = a.table_x + (size_t)ox * stride_x;
        xmin = t[0];
        n = min(t[1], a.ksize_x);
#pragma unroll
        for (int x = 0; x < kMaxK; ++x) k[x] = x < n ? t[2 + x] : 0;
    }
    const uint8_t *frame = a.frames + (size_t)view * a.height * a.width * 3;
    for (int i = sub; i < rows * 3; i += kRowStep) {       // i = local row * 3 + channel
        const int lr = i / 3, ch = i - lr * 3;
        const int sr = r0 + lr - a.pad_top;
        int acc = 1 << (kPrecision - 1);
        if (sr >= 0 && sr < a.height) {
            const uint8_t *p = frame + (size_t)sr * a.width * 3 + ch;
#pragma unroll
            for (int x = 0; x < kMaxK; ++x) {
                const int sx = xmin + x;
                if (x < n && sx >= 0 && sx < a.width) acc += (int)p[(size_t)sx * 3] * k[x];
            }
        }
        hbuf[i * kTileW + col] = (uint8_t)clip8(acc);
    }
    __syncthreads();

    // ---- vertical pass
    if (ox >= a.out_w) return;
    const size_t plane = (size_t)a.out_h * a.out_w;
    for (int oy = oy0 + sub; oy < oy_end; oy += kRowStep) {
        const int32_t *t = a.table_y + (size_t)oy * stride_y;
        const int first = t[0] - r0, ny = min(t[1], a.ksize_y);
        int acc[3] = {1 << (kPrecision - 1), 1 << (kPrecision - 1), 1 << (kPrecision - 1)};
#pragma unroll
        for (int y = 0; y < kMaxK; ++y) {
            const int lr = first + y;
            if (y < ny && lr >= 0 && lr < rows) {
                const int ky = t[2 + y];
                const uint8_t *p = hbuf + (size_t)lr * 3 * kTileW + col;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] += (int)p[ch * kTileW] * ky;
            }
        }
        float *o = a.out + (size_t)view * 3 * plane + (size_t)oy * a.out_w + ox;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[ch * plane] = (float)clip8(acc[ch]);
    }
}

__global__ __launch_bounds__(kBlock) void depth_to_metres_kernel(const uint16_t *depth_mm, int64_t n, float max_depth, float *out)
{
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float d = __fdiv_rn((float)depth_mm[i], 1000.0f);
    out[i] = d > max_depth ? 0.0f : d;
}

}  // namespace

extern "C" int eprecon_prepare_views_async(const uint8_t *frames, int n_views, int height, int width, int pad_top, int pad_bottom,
                                           const int32_t *table_x, int ksize_x, const int32_t *table_y, int ksize_y, int lds_rows,
                                           int out_h, int out_w, float *out, void *stream)
{
    if (!frames || !table_x || !table_y || !out || n_views <= 0 || height <= 0 || width <= 0 || out_h <= 0 || out_w <= 0 ||
        pad_top < 0 || pad_bottom < 0 || ksize_x < 1 || ksize_x > kMaxK || ksize_y < 1 || ksize_y > kMaxK || lds_rows < 1)
        return EPRECON_ERR_ARG;
    const size_t lds = (size_t)lds_rows * 3 * kTileW;
    if (lds > dynamic_lds_limit() || n_views > 65535 || ceil_div(out_h, kTileH) > 65535 ||
        (int64_t)n_views * height * width * 3 > 0x7fffffff || (int64_t)n_views * 3 * out_h * out_w > 0x7fffffff)
        return EPRECON_ERR_UNSUPPORTED;
    PrepareViewsArgs a{frames, table_x, table_y, out, height, width, pad_top, ksize_x, ksize_y, lds_rows, out_h, out_w};
    const dim3 grid((unsigned)ceil_div(out_w, kTileW), (unsigned)ceil_div(out_h, kTileH), (unsigned)n_views);
    hipLaunchKernelGGL(prepare_views_kernel, grid, dim3(kBlock), lds, (hipStream_t)stream, a);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" int eprecon_depth_to_metres_async(const uint16_t *depth_mm, int64_t n, float max_depth, float *out, void *stream)
{
    if (!depth_mm || !out || n < 0) return EPRECON_ERR_ARG;
    if (n == 0) return EPRECON_OK;
    if (ceil_div(n, kBlock) > 0x7fffffff) return EPRECON_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(depth_to_metres_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, (hipStream_t)stream,
                       depth_mm, n, max_depth, out);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
