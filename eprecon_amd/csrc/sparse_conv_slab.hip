// The gather kernels with 128-row workgroups on the kernel map (dispatcher: sparse_conv.hip, select_conv):
//   spconv_mfma_kernel       wide layers: 32-channel weight slabs double-buffered in LDS, one barrier per slab (here);
//   spconv_resident_kernel   C_in <= 64 (and, walked in slabs of <= 64 channels, the wide inputs of the 3D kernel maps): the
//                            weights of a group of offsets resident per barrier, rows gathered in software-pipelined batches
//                            (sparse_conv_resident_impl.hpp, instantiated by sparse_conv_resident_nt{1,2}.hip).
// and the image-tile kernel of the dense 2D 3x3 layers with C_in <= 40:
//   conv2d_tile_kernel       halo tile + all nine weight matrices in LDS, no kernel map, no global access in the MFMA loop.
// The two stage their weights with the same stage_weights<32> and share this unit for that reason: compiled apart, the optimiser
// sees each without the other's calls of it and allocates the NT = 1 instantiations of both differently (four VGPRs either way
// on spconv_mfma_kernel<1, *>; profiles/r10/README.md).
#include "common.hpp"
#include "conv_common.hpp"
#include "conv_gather.hpp"

namespace {
using namespace ep;
using namespace epconv;

template <int NT, bool VEC4>
__global__ __launch_bounds__(256) void spconv_mfma_kernel(ConvParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TN = 32 * NT;
    float *sW = reinterpret_cast<float *>(smem);                     // [2][kSlabC][TN]
    int *sNbr = reinterpret_cast<int *>(sW + 2 * kSlabC * TN);       // [K][128]
    int *sActive = sNbr + p.K * kRowsPerBlock;                       // [K] live-row flags
    const int cinA = (p.Cin + 3) & ~3;
    float *sAff = reinterpret_cast<float *>(sActive + ((p.K + 3) & ~3));  // [2][cinA] input scale / shift

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int row0 = blockIdx.x * kRowsPerBlock;
    const int col0 = blockIdx.y * TN;  // short lists: the output columns are split over blockIdx.y

    // neighbour tile + live-offset flags
    for (int k = tid; k < p.K; k += 256) sActive[k] = 0;
    stage_in_affine<256>(p, sAff, cinA, tid);
    __syncthreads();
    for (int e = tid; e < p.K * kRowsPerBlock; e += 256) {
        const int k = e / kRowsPerBlock, r = e - k * kRowsPerBlock;
        const int row = row0 + r;
        int j = -1;
        if (row < p.n_out) j = p.nbr ? p.nbr[(size_t)k * p.n_out + row] : row;
        sNbr[e] = j;
        if (j >= 0) sActive[k] = 1;  // benign race: every writer stores 1
    }
    __syncthreads();

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int nslab = (p.Cin + kSlabC - 1) / kSlabC;
    // stage counter over (live k, slab); the double buffer flips per staged slab
    int buf = 0;
    bool have_prev = false;
    for (int k = 0; k < p.K; ++k) {
        if (!sActive[k]) continue;  // block-uniform
        const int j = sNbr[k * kRowsPerBlock + wave * kRowsPerWave + r32];
        const float *xrow = p.x + (size_t)(j >= 0 ? j : 0) * p.ld_x;
        const float *wk = p.w + (size_t)k * p.Cin * p.Cout + col0;
        for (int sl = 0; sl < nslab; ++sl) {
            const int c0 = sl * kSlabC;
            // ---- stage W[k][c0 : c0+32][0 : TN] into sW[buf] (zero padded) ----
            float *dstW = sW + buf * kSlabC * TN;
            stage_weights<TN>(dstW, wk, c0, p.Cin, p.Cout, p.Cout - col0, kSlabC, tid);
            // ---- gather this lane's A values: 4 chunks of 8 channels, 4 floats each ----
            float a[4][4];
#pragma unroll
            for (int ch = 0; ch < 4; ++ch) {
                const int c = c0 + ch * 8 + 4 * half;
                if (VEC4) {
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (j >= 0 && c < p.Cin) v = *reinterpret_cast<const float4 *>(xrow + c);
                    if (p.Cin & 3) {  // ragged channel count: whatever follows the row's last channel is not input
                        if (c + 1 >= p.Cin) v.y = 0.0f;
                        if (c + 2 >= p.Cin) v.z = 0.0f;
                        if (c + 3 >= p.Cin) v.w = 0.0f;
                    }
                    a[ch][0] = v.x; a[ch][1] = v.y; a[ch][2] = v.z; a[ch][3] = v.w;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) a[ch][s] = (j >= 0 && c + s < p.Cin) ? xrow[c + s] : 0.0f;
                }
            }
            __syncthreads();  // sW[buf] complete; the other buffer is free again after this barrier
            (void)have_prev;
            const float *srcW = sW + buf * kSlabC * TN;
            const int nch = min(4, (p.Cin - c0 + 7) / 8);
            if (p.in_scale) {
                // BatchNorm (+ReLU) of the producer applied to the gathered values; padding stays 0
#pragma unroll
                for (int ch = 0; ch < 4; ++ch) {
                    const int c = c0 + ch * 8 + 4 * half;
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const bool ok = j >= 0 && c + s < p.Cin;
                        float v = fmaf(a[ch][s], sAff[min(c + s, cinA - 1)], sAff[cinA + min(c + s, cinA - 1)]);
                        if (p.in_relu) v = fmaxf(v, 0.0f);
                        a[ch][s] = ok ? v : 0.0f;
                    }
                }
            }
            for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float *brow = srcW + (ch * 8 + 4 * half + s) * TN + r32;
#pragma unroll
                    for (int t = 0; t < NT; ++t)
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[ch][s], brow[t * 32], acc[t], 0, 0, 0);
                }
            }
            buf ^= 1;
            have_prev = true;
        }
    }

    conv_epilogue<NT>(p, acc, LinearRows{row0 + wave * kRowsPerWave, p.n_out}, col0, r32, half, wave, sW, (int)blockIdx.x, (int)gridDim.y);
}

template <int NT>
int launch_conv(const ConvParams &p, bool vec4, hipStream_t st)
{
    const dim3 grid((unsigned)ceil_div(p.n_out, kRowsPerBlock), (unsigned)ceil_div(p.Cout, 32 * NT));
    const size_t lds = (size_t)2 * kSlabC * 32 * NT * sizeof(float) +
                       (size_t)p.K * kRowsPerBlock * sizeof(int) + (size_t)((p.K + 3) & ~3) * sizeof(int) +
                       (size_t)2 * ((p.Cin + 3) & ~3) * sizeof(float) + 16;
    if (vec4)
        hipLaunchKernelGGL((spconv_mfma_kernel<NT, true>), grid, dim3(256), lds, st, p);
    else
        hipLaunchKernelGGL((spconv_mfma_kernel<NT, false>), grid, dim3(256), lds, st, p);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// ---------------------------------------------------------------------------------------------
// Dense 2D 3x3 'same' convolution, narrow layers (9 * cin_pad * 32 NT floats of weights fit LDS):
// implicit GEMM on an image tile.  A workgroup owns 8 rows x 16 pixels of one map; the 10 x 18 halo
// tile of the input is staged ONCE in LDS with coalesced 16-byte loads (the producer's pending
// BatchNorm + ReLU applied on the way in, zero padding outside the image), together with all nine
// weight matrices; the nine offsets then read their A operands from LDS (one ds_read_b128 per chunk),
// so the inner loop has no global memory access at all.  The gather form of the same layer re-reads
// every input row nine times through L1/L2 and pays a memory latency per batch of offsets:
// 53 us for 24->24 on 172,800 pixels (1.8 GFLOP).  Epilogue: the shared one (bias, ReLU, residual,
// BatchNorm summaries).
//   wave w -> tile rows 2w, 2w+1 (32 pixels); MFMA row r32 -> pixel (2w + r32 / 16, r32 % 16)
// ---------------------------------------------------------------------------------------------
constexpr int kTileH = 8, kTileW = 16;
constexpr int kHaloH = kTileH + 2, kHaloW = kTileW + 2;

template <int NT, int NCH>
__global__ __launch_bounds__(256) void conv2d_tile_kernel(ConvParams p, int tiles_x, int tiles_y)
{
    constexpr int cin_pad = NCH * 8;
    constexpr int P = cin_pad + 4;  // LDS pixel pitch in floats: 16 consecutive pixels hit 16 distinct bank quads
    constexpr int TN = 32 * NT;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sW = reinterpret_cast<float *>(smem);               // [9][cin_pad][TN], zero padded
    float *sX = sW + 9 * cin_pad * TN;                         // [kHaloH][kHaloW][P]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x, map = blockIdx.y;
    const int col0 = blockIdx.z * TN;
    const int x0 = tx * kTileW, y0 = ty * kTileH;
    const size_t map_row0 = (size_t)map * p.img_h * p.img_w;

    // (BatchNorm form (c): the input's pending BatchNorm comes as an accumulator block -> its affine form in LDS first)
    __shared__ __attribute__((aligned(16))) float sInAff[2 * cin_pad];
    if (p.in_acc) {
        stage_in_affine<256>(p, sInAff, cin_pad, tid);
        __syncthreads();
    }
    // ---- stage the weights of all nine offsets and the halo tile; one barrier ----
    if (cin_pad == p.Cin) {
        stage_weights<TN>(sW, p.w + col0, 0, 9 * p.Cin, p.Cout, p.Cout - col0, 9 * cin_pad, tid);
    } else {  // rows of an offset are not contiguous in the padded layout
        for (int k = 0; k < 9; ++k)
            stage_weights<TN>(sW + k * cin_pad * TN, p.w + col0, k * p.Cin, (k + 1) * p.Cin, p.Cout, p.Cout - col0, cin_pad, tid);
    }
    constexpr int C4 = cin_pad / 4;
    constexpr int kHaloItems = kHaloH * kHaloW * C4;
    constexpr int kHaloIter = (kHaloItems + 255) / 256;
    float4 hv[kHaloIter];
#pragma unroll
    for (int it = 0; it < kHaloIter; ++it) {  // all loads first (clamped addresses), then the fix-ups and LDS stores
        const int e = min(tid + it * 256, kHaloItems - 1);
        const int px = e / C4, c4 = e - px * C4;
        const int hy = px / kHaloW, hx = px - hy * kHaloW;
        const int y = min(max(y0 - 1 + hy, 0), p.img_h - 1), x = min(max(x0 - 1 + hx, 0), p.img_w - 1);
        hv[it] = *reinterpret_cast<const float4 *>(p.x + (map_row0 + (size_t)y * p.img_w + x) * p.ld_x + min(c4 * 4, p.Cin - 4));
    }
#pragma unroll
    for (int it = 0; it < kHaloIter; ++it) {
        const int e = tid + it * 256;
        if (e >= kHaloItems) break;
        const int px = e / C4, c4 = e - px * C4;
        const int hy = px / kHaloW, hx = px - hy * kHaloW;
        const int y = y0 - 1 + hy, x = x0 - 1 + hx;
        const int c = c4 * 4;
        float4 v = hv[it];
        if (p.in_scale) {
            float4 sc, sh;
            if (p.in_acc) {
                sc = *reinterpret_cast<const float4 *>(sInAff + min(c, cin_pad - 4));
                sh = *reinterpret_cast<const float4 *>(sInAff + cin_pad + min(c, cin_pad - 4));
            } else {
                sc = *reinterpret_cast<const float4 *>(p.in_scale + min(c, p.Cin - 4));
                sh = *reinterpret_cast<const float4 *>(p.in_shift + min(c, p.Cin - 4));
            }
            v.x = fmaf(v.x, sc.x, sh.x); v.y = fmaf(v.y, sc.y, sh.y);
            v.z = fmaf(v.z, sc.z, sh.z); v.w = fmaf(v.w, sc.w, sh.w);
            if (p.in_relu) {
                v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
            }
        }
        if (!(y >= 0 && y < p.img_h && x >= 0 && x < p.img_w && c < p.Cin)) v = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(sX + px * P + c) = v;
    }
    __syncthreads();

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int ry = 2 * wave + (r32 >> 4), rx = r32 & 15;  // this lane's pixel inside the tile
    const float *xa = sX + (ry * kHaloW + rx) * P + 4 * half;
    const float *wb = sW + r32 + 4 * half * TN;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const float *xk = xa + ((k / 3) * kHaloW + (k % 3)) * P;
        const float *wk = wb + k * cin_pad * TN;
        float4 av[NCH];
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) av[ch] = *reinterpret_cast<const float4 *>(xk + ch * 8);
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
            float b[4][NT];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int t = 0; t < NT; ++t) b[q][t] = wk[(ch * 8 + q) * TN + t * 32];
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].x, b[0][t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].y, b[1][t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].z, b[2][t], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[ch].w, b[3][t], acc[t], 0, 0, 0);
            }
        }
    }
    const int wy0 = y0 + 2 * wave;
    const ImageRows rm{(int)(map_row0 + (size_t)wy0 * p.img_w + x0), wy0, x0, p.img_h, p.img_w};
    const int partial_row = ((int)blockIdx.y * tiles_y + ty) * tiles_x + tx;
    conv_epilogue<NT>(p, acc, rm, col0, r32, half, wave, sW, partial_row, (int)gridDim.z);
}

size_t conv2d_tile_lds(int nt, int nch) { return ((size_t)9 * nch * 8 * 32 * nt + (size_t)kHaloH * kHaloW * (nch * 8 + 4)) * sizeof(float); }

template <int NCH>
int launch_conv2d_tile(const ConvParams &p, hipStream_t st)
{
    const int tiles_x = (p.img_w + kTileW - 1) / kTileW, tiles_y = (p.img_h + kTileH - 1) / kTileH;
    const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)p.img_maps, (unsigned)ceil_div(p.Cout, 32));
    const size_t lds = max(conv2d_tile_lds(1, NCH), (size_t)3 * 256 * sizeof(float));
    if (lds > 64 * 1024) {  // above the default dynamic-LDS limit: opt in once per instantiation
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv2d_tile_kernel<1, NCH>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024);
        if (attr != hipSuccess) return EPRECON_ERR_HIP_BASE - (int)attr;
    }
    hipLaunchKernelGGL((conv2d_tile_kernel<1, NCH>), grid, dim3(256), lds, st, p, tiles_x, tiles_y);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

// short lists: 32-column blocks over blockIdx.y instead of all (<= 128) output columns per workgroup (10,800 pixels of the
// 1/16 maps are 85 row tiles for 256 CUs; the gathered rows are re-read from L2 by each column block)
bool column_split(const ConvParams &p)
{
    return (int)ceil_div(p.n_out, kRowsPerBlock) < 256 && (p.Cout + 31) / 32 > 1 && !p.ln;
}
int cin_pad8(const ConvParams &p) { return (p.Cin + 7) / 8 * 8; }
}  // namespace

namespace epconv {
// eligibility of the tile kernel; on success *blocks = workgroups per column block (= BatchNorm summary rows)
bool conv2d_tile_ok(const ConvParams &p, int *nt_out, int *nch_out, int64_t *blocks)
{
    if (p.K != 9 || p.img_h <= 0 || p.img_w <= 0 || p.img_maps <= 0 || p.ln || p.accumulate)
        return false;
    if ((int64_t)p.img_maps * p.img_h * p.img_w != p.n_out) return false;
    if (p.Cin % 4 != 0 || p.ld_x % 4 != 0 || (reinterpret_cast<uintptr_t>(p.x) & 15) != 0) return false;
    if (p.in_scale && ((reinterpret_cast<uintptr_t>(p.in_scale) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.in_shift) & 15) != 0))
        return false;
    const int nch = (p.Cin + 7) / 8;
    if (nch > 5) return false;
    const int nt = 1;  // 32-column blocks over blockIdx.z keep the nine weight matrices within LDS
    if (conv2d_tile_lds(nt, nch) > 96 * 1024) return false;
    const int tiles = ((p.img_h + kTileH - 1) / kTileH) * ((p.img_w + kTileW - 1) / kTileW);
    if ((int64_t)tiles * p.img_maps < 256) return false;  // short lists: the column-split gather form fills the chip better
    *nt_out = nt; *nch_out = nch; *blocks = (int64_t)tiles * p.img_maps;
    return true;
}

int launch_resident_nt1(const ConvParams &p, bool vec4, int cin_pad, hipStream_t st);
int launch_resident_nt2(const ConvParams &p, bool vec4, int cin_pad, hipStream_t st);

// narrow layers: the weights of a group of offsets resident in LDS
bool resident_narrow_ok(const ConvParams &p) { return cin_pad8(p) <= 64 && (p.Cout <= 64 || column_split(p)); }

int launch_resident_narrow(const ConvParams &p, hipStream_t st)
{
    return ((p.Cout + 31) / 32 == 1 || column_split(p)) ? launch_resident_nt1(p, gather_vec4(p), cin_pad8(p), st)
                                                        : launch_resident_nt2(p, gather_vec4(p), cin_pad8(p), st);
}

// wide inputs (C_in > 64) on the same pipelined kernel, walked in slabs of <= 64 channels.  Columns: 64 per workgroup
// when the row tiles alone fill the chip, else 32.
// (3D kernel maps only: the dense 2D layers, K = 1 / 9 on 10,800..43,200 pixel rows, measured faster on the slab kernel)
bool resident_wide_ok(const ConvParams &p)
{
    return cin_pad8(p) > 64 && gather_vec4(p) && (p.K == 27 || p.K == 8) && !(p.ln && (p.Cout + 31) / 32 > 2);
}

int launch_resident_wide(const ConvParams &p, hipStream_t st)
{
    const int nblk = (int)ceil_div(p.n_out, kRowsPerBlock), nt_full = (p.Cout + 31) / 32;
    const bool two = nt_full >= 2 && (p.ln || (int64_t)nblk * ((nt_full + 1) / 2) >= 256);
    return two ? launch_resident_nt2(p, gather_vec4(p), cin_pad8(p), st) : launch_resident_nt1(p, gather_vec4(p), cin_pad8(p), st);
}

int launch_mfma(const ConvParams &p, hipStream_t st)
{
    const bool vec4 = gather_vec4(p);
    const int nt_full = (p.Cout + 31) / 32;
    if (nt_full == 1 || column_split(p)) return launch_conv<1>(p, vec4, st);
    if (nt_full == 2) return launch_conv<2>(p, vec4, st);
    if (nt_full == 3) return launch_conv<3>(p, vec4, st);
    return launch_conv<4>(p, vec4, st);  // Cout > 128: 128-column blocks over blockIdx.y
}

int launch_image_tile(const ConvParams &p, hipStream_t st)
{
    switch ((p.Cin + 7) / 8) {
        case 1: return launch_conv2d_tile<1>(p, st);
        case 2: return launch_conv2d_tile<2>(p, st);
        case 3: return launch_conv2d_tile<3>(p, st);
        case 4: return launch_conv2d_tile<4>(p, st);
        default: return launch_conv2d_tile<5>(p, st);
    }
}

}  // namespace epconv
