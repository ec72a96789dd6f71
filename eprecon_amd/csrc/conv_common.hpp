// Shared between the translation units of the convolution family (the dispatcher sparse_conv.hip and one sparse_conv_*.hip per
// kernel family): the launch parameters, the BatchNorm summary helpers, the epilogue of the 16-row tile kernels, and at the end
// each family's contract with the dispatcher: its eligibility rule, the BatchNorm summary rows (or the rows of a summary block)
// of its launch, and its launcher, which picks the template instantiation.
#pragma once
#include "common.hpp"

namespace epconv {

struct ConvParams {
    const float *x;      // [n_in, ld_x] (+ x_col0 folded into the pointer)
    const int32_t *nbr;  // [K][n_out] or nullptr (K must be 1: identity map)
    const float *w;      // [K][Cin][Cout]
    const float *bias;   // [Cout] or nullptr
    float *out;          // [n_out, ld_out]
    int n_out, K, Cin, Cout, ld_x, ld_out;
    int64_t x_bytes;     // bytes addressable from x (buffer-load gathers: rows past it read as zeros)
    int relu;            // fused ReLU epilogue
    int accumulate;      // out += result instead of out = result
    const float *res;    // optional [n_out, ld_res]: added after the ReLU (x + ReLU(conv(x)) blocks)
    int ld_res;
    float *bn_partial;   // optional [3][Cout][bn_ld]: per-workgroup (count, mean, M2) of the stored values, channel-major
    int bn_ld;           // ... its row stride (>= the summary rows the launch writes; see bn_partial_store)
    // BatchNorm of the INPUT applied while gathering: a = [relu](x * in_scale[c] + in_shift[c]) (nullptr: a = x)
    const float *in_scale, *in_shift;
    int in_relu;
    // the same for the residual operand (columns of the output)
    const float *res_scale, *res_shift;
    int res_relu;
    // LayerNorm over the Cout channels of every output row, after bias / ReLU / residual (needs all
    // columns in one workgroup): out = [relu]( LN(v) * ln_gamma + ln_beta )
    int ln;
    const float *ln_gamma, *ln_beta;
    float ln_eps;
    int ln_post_relu;
    // dense 2D 'same' 3x3 convolution over [maps][img_h][img_w] pixel rows (K == 9): lets narrow layers run
    // on conv2d_tile_kernel, which needs no kernel map
    int img_h, img_w, img_maps;
    // the caller sizes bn_partial with eprecon_conv_desc_partial_rows (descriptor entry point), so kernels whose
    // workgroups do not cover 128 rows may be chosen
    int flex_partial;
    // dense-grid form of the 3x3x3 stride-1 convolution (conv3d_tile_kernel): vox_rank int32[gx][gy][gz] (z fastest) holds
    // the row of the voxel in a grid cell or -1; wq = the weights in MFMA operand order (pack_weights_kernel)
    const int32_t *vox_rank;
    int gx, gy, gz;
    const float *wq;    // ... in 32x32x2 operand order (pack_weights_kernel): B operands of the split-K and cross-workgroup kernels
    const float *wq16;  // ... in 16x16x4 operand order (pack_weights16_kernel): 16-row tile kernel, direct gather kernel
    int debug;  // always 0 in the library; timing probes build with it set: 1 no MFMA loop, 2 tile16: weights from the first offset, 4 no halo row loads
    int splitk_pipe;  // split-K kernel: 1 software-pipelined stages, 2 also B operands straight from the packed weights (wq)
    void *ws;         // caller's scratch (eprecon_conv_desc.workspace): partial sums of the cross-workgroup split-K kernel, or
                      // the job counters of the persistent form (the two families share no shape)
    size_t ws_bytes;
    // BatchNorm form (c) (round 6): the producer adds its workgroups' per-channel sums to ORDER-INDEPENDENT
    // integer accumulators instead of (or beside) the per-workgroup summaries, and the consumer turns them into (scale, shift)
    // in its prologue — no finalize launch between two convolutions.  A block: int64[kBnCopies][ld][kBnWords] sums followed by
    // float[2][ld] (gamma, beta: written by the producer's first workgroup); *_c0 = first channel of this layer in the block.
    long long *bn_acc;
    int bn_acc_ld, bn_acc_c0;
    const float *bn_gamma, *bn_beta;      // the producer's BatchNorm parameters (copied into the block) or nullptr (1, 0)
    const long long *in_acc;              // consumer: the block its input's pending BatchNorm lives in
    int in_acc_ld, in_acc_c0;
    float in_eps;
};

// ---- BatchNorm form (c): exact, order-independent sums ------------------------------------------------------------------
// Per (copy, channel) seven int64 words: S1 = sum n_w mean_w and S2 = sum (M2_w + n_w mean_w^2) over the producer's workgroups
// w, each as THREE limbs of a 2^-40 fixed-point value (fraction, integer bits 0..39, integer bits 40.. signed), and the
// count.  Every add is a fire-and-forget 64-bit integer atomic (integer addition commutes: the result does not depend on the
// order the workgroups finish in, so inference stays run-to-run bit-identical); a limb sum cannot overflow (2^40 x 2^23 adds).
// The limbs are exact images of the doubles they come from, so sum n mean^2 - (sum n mean)^2 / N cancels exactly as the
// between-workgroup term of a Chan merge does.  kBnCopies copies spread the same-address atomics (21 ns each on this part).
constexpr int kBnCopies = 8, kBnWords = 7;
#ifndef EP_BN_ABL       // timing ablations of probe builds only: 1 no atomics, 2 no finish in the consumers (wrong results)
#define EP_BN_ABL 0
#endif

__device__ __forceinline__ void bn_limbs(double x, long long &l0, long long &l1, long long &l2)
{
    const double v = x * 1099511627776.0;                    // 2^40 (exact scaling)
    const double hi = floor(v * (1.0 / 1099511627776.0));    // floor(x)
    l0 = (long long)(v - hi * 1099511627776.0);              // fraction bits, in [0, 2^40) (below 2^-40: truncated)
    const long long h = (long long)hi;
    l1 = h & ((1ll << 40) - 1);
    l2 = h >> 40;
}

__device__ __forceinline__ void bn_acc_add(long long *acc, int ld, int c, int copy, float n, float mean, float m2)
{
    if (n <= 0.0f || (EP_BN_ABL & 1)) return;
    unsigned long long *a = reinterpret_cast<unsigned long long *>(acc) + ((size_t)copy * ld + c) * kBnWords;
    const double dn = (double)n, dm = (double)mean;
    long long l0, l1, l2;
    bn_limbs(dn * dm, l0, l1, l2);
    atomicAdd(a + 0, (unsigned long long)l0);
    if (EP_BN_ABL & 4) return;      // (one atomic per channel instead of seven)
    atomicAdd(a + 1, (unsigned long long)l1); atomicAdd(a + 2, (unsigned long long)l2);
    bn_limbs((double)m2 + dn * dm * dm, l0, l1, l2);
    atomicAdd(a + 3, (unsigned long long)l0); atomicAdd(a + 4, (unsigned long long)l1); atomicAdd(a + 5, (unsigned long long)l2);
    atomicAdd(a + 6, (unsigned long long)(long long)n);
}

// the BatchNorm of channel c of the block in affine form: y = x * scale + shift.  (The copies are walked ONE at a time: with the
// loop unrolled, 56 int64 loads in flight pushed the 1,024-thread split-K kernel, whose prologue inlines this, into scratch.)
__device__ __forceinline__ void bn_acc_affine(const long long *acc, int ld, int c, float eps, float &scale, float &shift)
{
    if (EP_BN_ABL & 2) { scale = 1.0f; shift = 0.0f; return; }
    long long w[kBnWords] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
    for (int k = 0; k < kBnCopies; ++k) {
        const long long *a = acc + ((size_t)k * ld + c) * kBnWords;
#pragma unroll
        for (int j = 0; j < kBnWords; ++j) w[j] += a[j];
    }
    const double two40 = 1099511627776.0;
    const double s1 = ((double)w[2] * two40 + (double)w[1]) + (double)w[0] * (1.0 / two40);
    const double s2 = ((double)w[5] * two40 + (double)w[4]) + (double)w[3] * (1.0 / two40);
    const double n = (double)w[6];
    const float *gb = reinterpret_cast<const float *>(acc + (size_t)kBnCopies * ld * kBnWords);
    const double mean = n > 0.0 ? s1 / n : 0.0;
    double var = n > 0.0 ? s2 / n - mean * mean : 0.0;     // biased variance
    if (var < 0.0) var = 0.0;
    const float sc = gb[c] / sqrtf((float)var + eps);
    scale = sc;
    shift = gb[ld + c] - (float)mean * sc;
}

// prologue of the gather kernels: (scale, shift) of the input channels -> sAff[0 .. cpad) / sAff[cpad .. 2 cpad), from the
// producer-finished vectors or from the accumulator block (zero beyond Cin)
template <int THREADS, bool ACC = true>
__device__ __forceinline__ void stage_in_affine(const ConvParams &p, float *sAff, int cpad, int tid)
{
    if (!p.in_scale) return;
    for (int c = tid; c < cpad; c += THREADS) {
        float sc = 0.0f, sh = 0.0f;
        if (c < p.Cin) {
            if (ACC && p.in_acc) bn_acc_affine(p.in_acc, p.in_acc_ld, p.in_acc_c0 + c, p.in_eps, sc, sh);
            else { sc = p.in_scale[c]; sh = p.in_shift[c]; }
        }
        sAff[c] = sc;
        sAff[cpad + c] = sh;
    }
}

// producer side: one thread per channel hands over its workgroup's summary; `first` (the launch's first workgroup) also leaves
// the BatchNorm parameters in the block
__device__ __forceinline__ void bn_acc_publish(const ConvParams &p, int col, int copy, bool first, float n, float mean, float m2)
{
    bn_acc_add(p.bn_acc, p.bn_acc_ld, p.bn_acc_c0 + col, copy & (kBnCopies - 1), n, mean, m2);
    if (first) {
        float *gb = reinterpret_cast<float *>(p.bn_acc + (size_t)kBnCopies * p.bn_acc_ld * kBnWords);
        gb[p.bn_acc_c0 + col] = p.bn_gamma ? p.bn_gamma[col] : 1.0f;
        gb[p.bn_acc_ld + p.bn_acc_c0 + col] = p.bn_beta ? p.bn_beta[col] : 0.0f;
    }
}

constexpr int kWaves = 4;
constexpr int kRowsPerWave = 32;
constexpr int kRowsPerBlock = kRowsPerWave * kWaves;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// Chan et al. merge of two (count, mean, M2) summaries; the caller fixes the order
__device__ __forceinline__ void chan_merge(float &n_a, float &mean_a, float &m2_a, float n_b, float mean_b, float m2_b)
{
    if (n_b == 0.0f) return;
    if (n_a == 0.0f) {
        n_a = n_b; mean_a = mean_b; m2_a = m2_b;
        return;
    }
    const float n = n_a + n_b;
    const float d = mean_b - mean_a;
    mean_a = mean_a + d * (n_b / n);
    m2_a = m2_a + m2_b + d * d * (n_a * n_b / n);
    n_a = n;
}

// One BatchNorm summary into bn_partial, channel-major: (count, mean, M2) of column `col` from summary row `row` at
// [(q * Cout + col) * bn_ld + row], q = 0, 1, 2.  The finalize of a channel then reads three contiguous runs of rows
// (csrc/norm.hip, bn_finalize_affine_kernel) instead of one float from each row's 64-byte segment.
__device__ __forceinline__ void bn_partial_store(const ConvParams &p, int row, int col, float n, float mean, float m2)
{
    const size_t plane = (size_t)p.Cout * p.bn_ld;
    float *dst = p.bn_partial + (size_t)col * p.bn_ld + row;
    dst[0] = n; dst[plane] = mean; dst[2 * plane] = m2;
}

// Epilogue of the 16-row tile kernels on v_mfma_f32_16x16x4_f32 (conv3d_tile16_kernel, conv2d_tile16_kernel): lane l holds
// output rows orow[0..3] (-1: no row) x columns 16 t + (l & 15) of its wave's CT accumulator tiles.  Bias, ReLU, residual (with
// its pending BatchNorm), row-wise LayerNorm (16-lane xor-shuffles), the stores, and the BatchNorm summaries of the workgroup
// (fixed-order Chan merges: lane groups, then waves) -> bn_partial row `partial_row`, and with ACC also into the accumulator block
// of BatchNorm form (c) (p.bn_acc).  sStat: >= NW * 3 * 16 CT floats of LDS no wave reads any more (the caller's barrier);
// every thread of the workgroup calls this.  NW: the waves of the workgroup (a wave whose rows are all -1 adds empty summaries).
template <int CT, bool ACC = false, int NW = kWaves>
__device__ __forceinline__ void tile16_epilogue(const ConvParams &p, const f32x4 (&acc)[CT], const int (&orow)[4], float *sStat,
                                                int partial_row)
{
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    float v[CT][4];
    bool colok[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) {
        const int col = 16 * t + l16;
        colok[t] = col < p.Cout;
        const float b = (p.bias && colok[t]) ? p.bias[col] : 0.0f;
        const float rs = (p.res_scale && colok[t]) ? p.res_scale[col] : 1.0f;
        const float rb = (p.res_scale && colok[t]) ? p.res_shift[col] : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float val = 0.0f;
            if (colok[t] && orow[j] >= 0) {
                val = acc[t][j] + b;
                if (p.relu) val = fmaxf(val, 0.0f);
                if (p.res) {
                    float rv = p.res[(size_t)orow[j] * p.ld_res + col];
                    if (p.res_scale) {
                        rv = fmaf(rv, rs, rb);
                        if (p.res_relu) rv = fmaxf(rv, 0.0f);
                    }
                    val += rv;
                }
            }
            v[t][j] = val;
        }
    }
    if (p.ln) {  // (uniform) row-wise LayerNorm over the C_out columns: 16 lanes x CT tiles hold a row
        const float inv_c = 1.0f / (float)p.Cout;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float sum = 0.0f;
#pragma unroll
            for (int t = 0; t < CT; ++t) sum += v[t][j];
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) sum += __shfl_xor(sum, m);
            const float mean = sum * inv_c;
            float sq = 0.0f;
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const float d = colok[t] ? v[t][j] - mean : 0.0f;
                v[t][j] = d;
                sq = fmaf(d, d, sq);
            }
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) sq += __shfl_xor(sq, m);
            const float inv = 1.0f / sqrtf(sq * inv_c + p.ln_eps);
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const int col = 16 * t + l16;
                float y = fmaf(v[t][j] * inv, (p.ln_gamma && colok[t]) ? p.ln_gamma[col] : 1.0f, (p.ln_beta && colok[t]) ? p.ln_beta[col] : 0.0f);
                if (p.ln_post_relu) y = fmaxf(y, 0.0f);
                v[t][j] = y;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < CT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (colok[t] && orow[j] >= 0) p.out[(size_t)orow[j] * p.ld_out + 16 * t + l16] = v[t][j];
    if (p.bn_partial || (ACC && p.bn_acc)) {  // (uniform) (count, mean, M2) of the stored values per column: rows in the lane, lane groups, waves
#pragma unroll
        for (int t = 0; t < CT; ++t) {
            float n = 0.0f, sum = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (orow[j] >= 0) { n += 1.0f; sum += v[t][j]; }
            float mean = n > 0.0f ? sum / n : 0.0f, m2 = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (orow[j] >= 0) { const float d = v[t][j] - mean; m2 = fmaf(d, d, m2); }
#pragma unroll
            for (int m = 16; m < 64; m <<= 1) {  // lane groups q in order: the lower group is the left operand
                const float on = __shfl_xor(n, m), om = __shfl_xor(mean, m), oq = __shfl_xor(m2, m);
                const bool lower = (lane & m) == 0;
                float a_n = lower ? n : on, a_mean = lower ? mean : om, a_m2 = lower ? m2 : oq;
                chan_merge(a_n, a_mean, a_m2, lower ? on : n, lower ? om : mean, lower ? oq : m2);
                n = a_n; mean = a_mean; m2 = a_m2;
            }
            if (q == 0) {
                float *d = sStat + (wave * 3) * 16 * CT + 16 * t + l16;
                d[0] = n; d[16 * CT] = mean; d[2 * 16 * CT] = m2;
            }
        }
        __syncthreads();
        if (tid < 16 * CT && tid < p.Cout) {
            float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
#pragma unroll
            for (int w = 0; w < NW; ++w)
                chan_merge(a_n, a_mean, a_m2, sStat[(w * 3) * 16 * CT + tid], sStat[(w * 3 + 1) * 16 * CT + tid], sStat[(w * 3 + 2) * 16 * CT + tid]);
            if (p.bn_partial) bn_partial_store(p, partial_row, tid, a_n, a_mean, a_m2);
            if (ACC && p.bn_acc) bn_acc_publish(p, tid, partial_row, partial_row == 0, a_n, a_mean, a_m2);
        }
    }
}

// 16-byte gathers need aligned rows; a channel count that is not a multiple of 4 is fine as long as the
// row pitch covers the rounded-up count (the tail lanes are zeroed after the load)
inline bool gather_vec4(const ConvParams &p)
{
    return (p.ld_x % 4 == 0) && ((reinterpret_cast<uintptr_t>(p.x) & 15) == 0) && (p.Cin % 4 == 0 || p.ld_x >= ((p.Cin + 3) & ~3));
}

// sparse_conv_dense3d.hip: the 3x3x3 stride-1 convolution on a dense grid (vox_rank), no kernel map
enum D3Kind { kD3None = 0, kD3Narrow = 1, kD3Tile16 = 2 };
// which of the two kernels the layer's shape is for (EPRECON_CONV_DENSE3D); exported as eprecon_conv_dense3d_kind only
__attribute__((visibility("hidden"))) int conv3d_shape_kind(const ConvParams &p);
int conv3d_kind(const ConvParams &p);                   // ... and which takes the launch: the 16-row kernel needs its wq16 packing
int d3_tiles_kind(const ConvParams &p, int kind, int *ty = nullptr, int *tz = nullptr);   // workgroups = BatchNorm summary rows
int launch_conv3d_16(const ConvParams &p, hipStream_t st);
int launch_conv3d_single_column(const ConvParams &p, hipStream_t st);

// sparse_conv_slab.hip: dense 2D 3x3 layers with C_in <= 40 on 8 x 16 pixel tiles (conv2d_tile_kernel)
// eligibility of the tile kernel; on success *blocks = workgroups per column block (= BatchNorm summary rows)
bool conv2d_tile_ok(const ConvParams &p, int *nt_out, int *nch_out, int64_t *blocks);
int launch_image_tile(const ConvParams &p, hipStream_t st);

// sparse_conv_wide.hip: medium lists with wide channels, the offsets split across workgroups (needs the caller's workspace)
constexpr int kWideRows = 128;
size_t wide_workspace_bytes(const ConvParams &p);
bool wide_shape_ok(const ConvParams &p);                // shape / alignment rule, independent of the workspace
bool wide_ok(const ConvParams &p);
int launch_wide(const ConvParams &p, hipStream_t st);

// sparse_conv_splitk.hip: short lists; one BatchNorm summary row per 32-row tile
constexpr int kSplitKRows = 32;
bool splitk_ok(const ConvParams &p);
int launch_splitk(ConvParams &p, hipStream_t st);       // (sets p.splitk_pipe)

// sparse_conv_slab.hip, sparse_conv_resident_nt{1,2}.hip: the gather kernels with 128-row (kRowsPerBlock) workgroups; the slab
// kernel takes whatever is left
bool resident_narrow_ok(const ConvParams &p);
int launch_resident_narrow(const ConvParams &p, hipStream_t st);
bool resident_wide_ok(const ConvParams &p);
int launch_resident_wide(const ConvParams &p, hipStream_t st);
int launch_mfma(const ConvParams &p, hipStream_t st);

// sparse_conv_direct.hip: the long-list 3x3x3 kernel on 16x16x4 MFMAs with operands straight from L2
bool direct16_ok(const ConvParams &p);
constexpr int kDirectRows = 128;          // output rows (and rows of a BatchNorm summary block) per workgroup
int launch_direct16(const ConvParams &p, hipStream_t st);
int direct16_partial_block_rows(const ConvParams &p);   // 128, or 32 when the persistent form takes the launch
size_t direct16_workspace_bytes(const ConvParams &p);   // 0, or the persistent form's job counters

// sparse_conv_tile2d.hip: the dense 2D 3x3 layers of the fusion stack on the 16-row image-tile kernel
// long pixel lists only (the rule dense2d.DIRECT_2D_MIN_ROWS hands the wq16 packing over by); shorter lists: the short-list kernel
constexpr int kT2MinRows = 40000;
// the two thresholds of the hand-over rule (eprecon_amd/sparse.py conv_packings) that the one-call SPVCNN pass needs at run
// time, where alone its row counts exist (spvcnn_forward.hip): sparse.DIRECT_MAX_COUT and sparse.K1_DIRECT_MIN_ROWS
constexpr int kDirectMaxCout = 64;
constexpr int64_t kK1DirectMinRows = 20000;
bool tile2d16_ok(const ConvParams &p);
int64_t tile2d16_partial_rows(const ConvParams &p);     // one BatchNorm summary row per workgroup (image tile)
int launch_tile2d16(const ConvParams &p, hipStream_t st);

// sparse_conv_tile2d_short.hip: the 3x3 layers of the 10,800-pixel level (one 16-pixel tile per workgroup, the reduction split
// across its three waves).  Lists below kT2ShortMaxRows (dense2d.SHORT_2D_MAX_ROWS hands the wq16 packing over by it); between
// that and kT2MinRows the previous rule holds (split-K, or the direct kernel when the caller packs for it)
constexpr int kT2ShortMaxRows = 20000;
bool tile2d_short_list(const ConvParams &p);            // a 3x3 image layer below kT2ShortMaxRows rows
bool tile2d_short_ok(const ConvParams &p);
int64_t tile2d_short_partial_rows(const ConvParams &p); // one BatchNorm summary row per workgroup (16-pixel tile)
int launch_tile2d_short(const ConvParams &p, hipStream_t st);


}  // namespace epconv
