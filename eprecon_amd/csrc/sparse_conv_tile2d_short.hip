// Dense 2D 3x3 'same' convolution on v_mfma_f32_16x16x4_f32 for SHORT pixel lists: the 10,800-pixel 1/16 level of the 2D fusion
// stack (9 x 30 x 40, C = 80 / 40), where conv2d_tile16_kernel (sparse_conv_tile2d.hip) has too few tiles to fill the chip and
// the split-K kernel it replaces goes through the pixel map (an index load, then a dependent gather, per tap).
//   - a workgroup owns ONE 16-pixel segment of one image row (810 workgroups at 9 x 30 x 40) and stages its 3 x 18 halo in LDS,
//     all C_in channels at once (18 KB at C_in = 80), the producer's pending BatchNorm (+ ReLU) applied on the way in, zeros
//     outside the image
//   - the reduction over the nine offsets is split across the three waves: wave w takes the offsets of halo row w (dy = w: three
//     offsets x all channel chunks); the partial accumulators of waves 1 and 2 are added to wave 0's in LDS in that fixed order
//   - why three waves: 810 tiles x 3 = 2,430 waves for the 1,024 SIMDs (2.4 per SIMD) with no imbalance between the waves of a
//     workgroup; the longest per-wave MFMA chain (80 -> 80: 3 offsets x 20 k-steps x 5 column tiles = 300 MFMAs of 32 cycles) is
//     about 4 us, and the SIMDs' MFMA pipes, not the chains, bound the layer (9.5 us of padded MFMA work at 80 -> 80)
//   - A operands: one ds_read_b128 per (offset, chunk) (a last chunk of <= 8 channels: ds_read_b64 and two MFMAs, the wq16 tail8
//     layout); B operands: the wq16 packing, one 1 KB buffer load per (offset, chunk, column tile), two steps ahead
//   - epilogue: tile16_epilogue (conv_common.hpp) on wave 0, one BatchNorm summary row per workgroup
// Summation order: four channels per MFMA as the other kernels; per wave (dx, chunk) in order, then dy = 0 + 1 + 2.  Bit-identical
// run to run; equal to the split-K kernel within fp32 round-off.
#include <stdint.h>
#include <stdlib.h>

#include "common.hpp"
#include "conv_common.hpp"

namespace epconv {
namespace {
using namespace ep;

constexpr int kSW = 16;                  // pixels of a tile (one 16-row MFMA tile)
constexpr int kSWaves = 3;               // one per halo row
constexpr int kSHaloW = kSW + 2;         // 18
constexpr int kSHalo = kSWaves * kSHaloW;  // 54 pixels
constexpr int kSThreads = kSWaves * 64;

template <int CT, int KCH, bool TAIL8, bool BN>
__global__ __launch_bounds__(kSThreads) void conv2d_tile_short_kernel(ConvParams p, int tiles_x)
{
    constexpr int P = 16 * KCH + 4;                       // LDS pixel pitch in floats (conflict-free ds_read_b128 at 52 / 84)
    constexpr int kRed = (kSWaves - 1) * CT * 256;        // partial accumulators of waves 1, 2
    constexpr int kStat = kSWaves * 3 * 16 * CT;          // the epilogue's summary scratch (after the partials)
    constexpr int kLds = kSHalo * P > kRed + kStat ? kSHalo * P : kRed + kStat;
    __shared__ __attribute__((aligned(16))) float sX[kLds];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, q = lane >> 4;
    const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);   // (gridDim.x = maps * H * tiles_x)
    const int H = p.img_h, W = p.img_w;
    const int irow = tile / tiles_x, tx = tile - irow * tiles_x;   // irow = map * H + y
    const int map = irow / H, y0 = irow - map * H, x0 = tx * kSW;
    const size_t map_row0 = (size_t)map * H * W;

    // ---- halo staging: element i -> (halo pixel i / G, 4-channel group i % G); loads at clamped addresses first, then the
    // fix-ups and the LDS stores
    constexpr int G = 4 * KCH;
    constexpr int kIt = (kSHalo * G + kSThreads - 1) / kSThreads;
    {
        float4 hv[kIt], sc[kIt], sh[kIt];
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int i = tid + it * kSThreads;
            const int px = min(i / G, kSHalo - 1);
            const int c = min(4 * (i % G), p.Cin - 4);
            const int hy = px / kSHaloW, hx = px - hy * kSHaloW;
            const int y = min(max(y0 - 1 + hy, 0), H - 1), x = min(max(x0 - 1 + hx, 0), W - 1);
            hv[it] = *reinterpret_cast<const float4 *>(p.x + (map_row0 + (size_t)y * W + x) * p.ld_x + c);
            if (BN) {   // (in_scale / in_shift may be slices of a concat buffer's vectors: no alignment assumed)
                sc[it] = make_float4(p.in_scale[c], p.in_scale[c + 1], p.in_scale[c + 2], p.in_scale[c + 3]);
                sh[it] = make_float4(p.in_shift[c], p.in_shift[c + 1], p.in_shift[c + 2], p.in_shift[c + 3]);
            }
        }
#pragma unroll
        for (int it = 0; it < kIt; ++it) {
            const int i = tid + it * kSThreads;
            if (i >= kSHalo * G) break;
            const int px = i / G, c = 4 * (i % G);
            const int hy = px / kSHaloW, hx = px - hy * kSHaloW;
            const int y = y0 - 1 + hy, x = x0 - 1 + hx;
            float4 v = hv[it];
            if (BN) {
                v.x = fmaf(v.x, sc[it].x, sh[it].x); v.y = fmaf(v.y, sc[it].y, sh[it].y);
                v.z = fmaf(v.z, sc[it].z, sh[it].z); v.w = fmaf(v.w, sc[it].w, sh[it].w);
                if (p.in_relu) {
                    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
                }
            }
            if (!(c < p.Cin && y >= 0 && y < H && x >= 0 && x < W)) v = make_float4(0.f, 0.f, 0.f, 0.f);   // zero padding
            *reinterpret_cast<float4 *>(sX + px * P + c) = v;
        }
    }
    __syncthreads();

    // ---- this wave's share of the reduction: offsets k = 3 wave + dx, dx = 0..2, every chunk; step s = dx * KCH + chunk
    f32x4 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    constexpr unsigned kStepBytes = CT * 1024u, kOffBytes = KCH * kStepBytes;
    constexpr int NS = 3 * KCH;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq16), 0, (int)(9 * kOffBytes), 0x00020000);
    const unsigned wlane = (unsigned)lane * 16u;
    const unsigned wbase = (unsigned)(3 * wave) * kOffBytes;
    // this lane's A row: pixel l16 of the tile; offset (wave, dx) reads halo pixel (wave, l16 + dx)
    const float *xa = sX + (wave * kSHaloW + l16) * P;
    constexpr int kAheadB = 2;
    float4 bq[kAheadB + 1][CT];
    float4 aq[2];
    auto load_b = [&](int s, float4(&dst)[CT]) {
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)t * 1024u,
                                                                  wbase + (unsigned)(s / KCH) * kOffBytes + (unsigned)(s % KCH) * kStepBytes, 0);
            dst[t] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
        }
    };
    auto load_a = [&](int s) {
        const bool tail = TAIL8 && s % KCH == KCH - 1;
        const float *src = xa + (s / KCH) * P + 16 * (s % KCH) + (tail ? 2 * q : 4 * q);
        if (tail) {
            const float2 v = *reinterpret_cast<const float2 *>(src);
            return make_float4(v.x, v.y, 0.0f, 0.0f);
        }
        return *reinterpret_cast<const float4 *>(src);
    };
#pragma unroll
    for (int s = 0; s < kAheadB; ++s) load_b(s, bq[s]);
    aq[0] = load_a(0);
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const bool tail = TAIL8 && s % KCH == KCH - 1;   // (compile time after unrolling)
        if (s + kAheadB < NS) load_b(s + kAheadB, bq[(s + kAheadB) % (kAheadB + 1)]);
        if (s + 1 < NS) aq[(s + 1) & 1] = load_a(s + 1);
        const float4 av = aq[s & 1];
        const float4(&bk)[CT] = bq[s % (kAheadB + 1)];
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bk[t].x, acc[t], 0, 0, 0);
#pragma unroll
        for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bk[t].y, acc[t], 0, 0, 0);
        if (!tail) {
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bk[t].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bk[t].w, acc[t], 0, 0, 0);
        }
        // this step's loads (B two steps ahead, the next step's A) spread among its MFMAs
#pragma unroll
        for (int sg = 0; sg < CT; ++sg) {
            __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            if (tail) __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
            else __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
        }
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_barrier(0);
    }

    // ---- cross-wave reduction in LDS (fixed order: dy = 0, then 1, then 2), the epilogue on wave 0
    __syncthreads();   // every wave is done with the halo: the partials overlay it
    f32x4 *red = reinterpret_cast<f32x4 *>(sX);
    if (wave > 0) {
#pragma unroll
        for (int t = 0; t < CT; ++t) red[((wave - 1) * CT + t) * 64 + lane] = acc[t];
    }
    __syncthreads();
    int orow[4];   // output rows of this lane's accumulator rows 4 q + j: pixel (y0, x0 + 4 q + j); waves 1, 2 hold none
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int x = x0 + 4 * q + j;
        orow[j] = (wave == 0 && x < W) ? (int)(map_row0 + (size_t)y0 * W + x) : -1;
    }
    if (wave == 0) {
#pragma unroll
        for (int w = 0; w < kSWaves - 1; ++w)
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] += red[(w * CT + t) * 64 + lane];
    }
    tile16_epilogue<CT, true, kSWaves>(p, acc, orow, sX + kRed, tile);
}

int tiles_x_of(const ConvParams &p) { return (p.img_w + kSW - 1) / kSW; }

template <int CT, int KCH, bool TAIL8, bool BN>
int launch_ts(const ConvParams &p, hipStream_t st)
{
    const int tx = tiles_x_of(p);
    hipLaunchKernelGGL((conv2d_tile_short_kernel<CT, KCH, TAIL8, BN>), dim3((unsigned)((int64_t)tx * p.img_h * p.img_maps)), dim3(kSThreads),
                       0, st, p, tx);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
template <int CT, int KCH, bool TAIL8>
int launch_ts_bn(const ConvParams &p, hipStream_t st)
{
    return p.in_scale ? launch_ts<CT, KCH, TAIL8, true>(p, st) : launch_ts<CT, KCH, TAIL8, false>(p, st);
}
template <int CT, int KCH>
int launch_ts_tail(const ConvParams &p, hipStream_t st)
{
    // (pack_weights16_body's rule: a last chunk of <= 8 channels is laid out for two MFMAs)
    return p.Cin - 16 * (KCH - 1) <= 8 ? launch_ts_bn<CT, KCH, true>(p, st) : launch_ts_bn<CT, KCH, false>(p, st);
}
template <int CT>
int launch_ts_kch(const ConvParams &p, hipStream_t st)
{
    return (p.Cin + 15) / 16 == 3 ? launch_ts_tail<CT, 3>(p, st) : launch_ts_tail<CT, 5>(p, st);
}
}  // namespace

bool tile2d_short_list(const ConvParams &p) { return p.K == 9 && p.img_maps > 0 && p.n_out < kT2ShortMaxRows; }

// EPRECON_CONV_TILE2D_SHORT=0: the short-list 3x3 layers on the kernels of the previous rule (read per launch: tests flip it).
// Takes K = 9 image layers below kT2ShortMaxRows rows with 33..48 or 65..80 channels in and out (the 1/16 level: 80 -> 80, 80 -> 40,
// 40 -> 40).  Declines like tile2d16_ok: an input whose pending BatchNorm is an accumulator block (in_acc), LayerNorm /
// accumulate, unaligned inputs or weights.
bool tile2d_short_ok(const ConvParams &p)
{
    if (switch_off("EPRECON_CONV_TILE2D_SHORT")) return false;
    if (!tile2d_short_list(p) || p.img_h <= 0 || p.img_w <= 0 || (int64_t)p.img_maps * p.img_h * p.img_w != p.n_out) return false;
    if (p.ln || p.accumulate || p.in_acc) return false;
    const int ct = (p.Cout + 15) / 16, kch = (p.Cin + 15) / 16;
    if ((ct != 3 && ct != 5) || (kch != 3 && kch != 5)) return false;
    if (p.Cin % 4 != 0 || p.ld_x % 4 != 0 || (reinterpret_cast<uintptr_t>(p.x) & 15) != 0) return false;
    if (!p.wq16 || (reinterpret_cast<uintptr_t>(p.wq16) & 15) != 0) return false;
    // every pixel row of the images must be readable (n_in >= n_out)
    if (p.x_bytes < ((int64_t)(p.n_out - 1) * p.ld_x + p.Cin) * 4) return false;
    return true;
}

int64_t tile2d_short_partial_rows(const ConvParams &p) { return (int64_t)tiles_x_of(p) * p.img_h * p.img_maps; }

int launch_tile2d_short(const ConvParams &p, hipStream_t st)
{
    return (p.Cout + 15) / 16 == 3 ? launch_ts_kch<3>(p, st) : launch_ts_kch<5>(p, st);
}

}  // namespace epconv
