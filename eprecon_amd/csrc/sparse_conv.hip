// Sparse 3D convolution for gfx950 as an output-stationary gather-GEMM on the fp32 matrix cores.
//
// Replaces (reference call sites; the CUDA kernels themselves live in the un-vendored torchsparse /
// spconv extensions, so the semantics below are this build's restatement — SURVEY.md appendix A):
//   spnn.Conv3d k=3 s=1, k=2 s=2, k=2 s=2 transposed, k=1     models/modules.py:19-64,90-122,181
//   spconv.SubMConv3d k=1 / k=3 (+bias)                         models/modules.py:252,444
//
//   out[i, :] = bias + sum_k  x[nbr[k][i], :] @ W[k]          (rows with nbr == -1 contribute 0)
//
// nbr is the kernel map int32[K][n_out] built once per coordinate set by kernel_map.hip and shared
// by every layer on that set (stride-1 k=3: K = 27, out coords = in coords; k2s2 down: K = 8 children
// of each coarse voxel; transposed: K = 8 with one live entry per fine voxel; k=1: identity map).
// There is no scatter-add and no atomic: every output row is produced by exactly one wave, so the
// result is deterministic.
//
// Mapping to CDNA4: a wave owns 32 output rows x (32*NT) output channels in NT accumulators of
// v_mfma_f32_32x32x2_f32 (exact fp32, k-ordered fma chain).  A operand: each lane holds 4 consecutive
// input channels of its row, one VGPR per MFMA step.  B operand: weights from LDS or, pre-packed in operand order
// (sparse_conv_pack.hip), straight from L2.  The kernel families share the prologue / epilogue fusions and differ in how the
// operands reach the wave; each lives in its own translation unit behind the contract of conv_common.hpp (eligibility rule,
// BatchNorm summary rows, launcher), and select_conv below is the one place that ranks them:
//   sparse_conv_dense3d.hip      conv3d_tile_narrow_kernel, conv3d_tile16_kernel: 3x3x3 layers on a dense grid, no kernel map;
//   sparse_conv_tile2d.hip       conv2d_tile16_kernel: dense 2D 3x3 layers on long pixel lists (16-row MFMA tiles);
//   sparse_conv_tile2d_short.hip conv2d_tile_short_kernel: the same on short pixel lists;
//   sparse_conv_slab.hip         conv2d_tile_kernel: dense 2D 3x3 layers with C_in <= 40: halo tile + all nine weight matrices
//                                in LDS, no kernel map, no global access in the MFMA loop;
//   sparse_conv_wide.hip         spconv_wide_kernel (+ its reduce kernel): medium lists with wide channels, the offsets split
//                                across workgroups;
//   sparse_conv_splitk.hip       spconv_splitk_kernel: short lists: 32-row workgroups whose waves split the (offset, slab)
//                                chain, wave-private slabs, fixed-order sum of the partials;
//   sparse_conv_direct*.hip      spconv_direct16_kernel: long lists, operands straight from L2;
//   sparse_conv_resident_*.hip   spconv_resident_kernel: C_in <= 64 (wide inputs in slabs): the weights of a group of offsets
//                                resident per barrier, the neighbour tile in LDS, rows gathered from global memory in
//                                software-pipelined batches (a fixed number of loads in flight -> vmcnt(N) waits);
//   sparse_conv_slab.hip         spconv_mfma_kernel: everything else: 32-channel weight slabs double-buffered in LDS.
// Shared device code of the 32x32x2 families: conv_gather.hpp.
// Prologue: the producer's pending BatchNorm (+ReLU) applied while loading (in_scale / in_shift).
// Epilogues (conv_epilogue): bias, ReLU, residual (with its own pending BatchNorm), per-workgroup
// BatchNorm summaries (count, mean, M2) of the stored values, or a row-wise LayerNorm over C_out.
// Roofline: fp32 MFMA (157 TFLOP/s) for wide layers on long lists (measured 41 % on 32->32, K = 27);
// narrow or short layers are bound by their dependent chain (staging round trips), see DESIGN.md 3b.
#include <stdio.h>
#include <stdlib.h>

#include "common.hpp"
#include "conv_common.hpp"

namespace {
using namespace ep;
using namespace epconv;

// One-shot timing hook for bench.py's `roofline_conv`: the next launch whose (K, Cin, Cout) match and whose list is
// at least min_rows long is bracketed by two events on the launch stream.
struct ConvProf {
    bool armed = false, recorded = false;
    int K = 0, cin = 0, cout = 0;
    int64_t min_rows = 0, rows = 0;
    const char *kernel = "";
    hipEvent_t start = nullptr, stop = nullptr;
    unsigned long long *pairs_dev = nullptr;  // [0] live (output row, offset) pairs of the bracketed launch, [1] the pairs it issues MFMAs for
} g_conv_prof;

// live pairs of a launch = what its algorithmic flop count rests on; counted on the launch stream BEHIND the stop event
__global__ void count_map_pairs_kernel(const int32_t *nbr, size_t total, unsigned long long *out)
{
    unsigned long long c = 0;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) c += nbr[e] >= 0;
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
__global__ void count_grid_pairs_kernel(const int32_t *rank, int gx, int gy, int gz, unsigned long long *out)
{
    unsigned long long c = 0;
    const int total = gx * gy * gz;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        if (rank[e] < 0) continue;
        const int z = e % gz, y = (e / gz) % gy, x = e / (gz * gy);
        for (int k = 0; k < 27; ++k) {
            const int xx = x + k % 3 - 1, yy = y + (k / 3) % 3 - 1, zz = z + k / 9 - 1;
            if (xx >= 0 && xx < gx && yy >= 0 && yy < gy && zz >= 0 && zz < gz) c += rank[(xx * gy + yy) * gz + zz] >= 0;
        }
    }
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
// rows of the (32-row group, offset) pairs with at least one neighbour: what the direct kernel issues MFMAs for
__global__ void count_map_groups_kernel(const int32_t *nbr, int n, int K, unsigned long long *out)
{
    const int groups = (n + 31) / 32;
    unsigned long long c = 0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < K * groups; e += gridDim.x * blockDim.x) {
        const int k = e / groups, g = e - k * groups;
        const int rows = min(32, n - 32 * g);
        bool any = false;
        for (int i = 0; i < rows; ++i) any |= nbr[(size_t)k * n + 32 * g + i] >= 0;
        if (any) c += rows;
    }
    for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
const char *g_last_conv_kernel = "";

// The kernel families in the order select_conv tries them, and the names the profiling entry points report for them.
enum ConvFamily {
    kFamDense3dNarrow, kFamDense3dTile16, kFamTile2d16, kFamTile2dShort, kFamImageTile, kFamWide, kFamSplitK, kFamDirect16,
    kFamResident, kFamResidentWide, kFamMfma
};
constexpr const char *kConvFamilyNames[] = {
    "conv3d_tile_narrow_kernel",
    "conv3d_tile16_kernel",
    "conv2d_tile16_kernel",
    "conv2d_tile_short_kernel",
    "conv2d_tile_kernel",
    "spconv_wide_kernel",
    "spconv_splitk_kernel",
    "spconv_direct16_kernel",
    "spconv_resident_kernel",
    "spconv_resident_kernel(wide)",
    "spconv_mfma_kernel",
};
static_assert(sizeof(kConvFamilyNames) / sizeof(kConvFamilyNames[0]) == kFamMfma + 1, "one name per family");

struct ConvChoice {
    ConvFamily family;
    const char *name;        // kConvFamilyNames[family]
    int64_t partial_rows;    // rows of bn_partial the launch writes
    int status;              // EPRECON_OK, or why the launch is refused (family and rows then say what the shape alone would get)
};

// Which family takes the launch: THE priority order (the dispatcher, eprecon_conv_desc_partial_rows and the profiling hook all
// ask here).  p.n_out and p.x_bytes are set.  The switches behind the family rules are read per call: tests flip them.
ConvChoice select_conv(const ConvParams &p)
{
    int status = EPRECON_OK;
    auto take = [&](ConvFamily f, int64_t rows) { return ConvChoice{f, kConvFamilyNames[f], rows, status}; };
    auto blocks_of = [&](int rows) { return ceil_div((int64_t)p.n_out, (int64_t)rows); };
    if (const int kind = conv3d_kind(p)) return take(kind == kD3Narrow ? kFamDense3dNarrow : kFamDense3dTile16, d3_tiles_kind(p, kind));
    if (!p.nbr && p.K != 1) status = EPRECON_ERR_ARG;  // dense-grid form requested for a shape it does not take, no map given
    // dense 2D 3x3 layers on long pixel lists: the 16-row image-tile kernel (EPRECON_CONV_TILE2D16=0: off)
    if (tile2d16_ok(p)) return take(kFamTile2d16, tile2d16_partial_rows(p));
    // ... and on short pixel lists: one 16-pixel tile per workgroup, the reduction split across its waves
    // (EPRECON_CONV_TILE2D_SHORT=0: off)
    if (tile2d_short_ok(p)) return take(kFamTile2dShort, tile2d_short_partial_rows(p));
    // the direct gather kernel wants the launch (the wq16 packing of a short image list is the short-list kernel's, which declined) ...
    const bool direct = direct16_ok(p) && !tile2d_short_list(p);
    // ... and for a dense 2D 3x3 layer whose caller packed the weights for it, it goes ahead of conv2d_tile and split-K
    const bool direct2d = p.K == 9 && direct;
    int nt, nch;
    int64_t tiles;
    if (!direct2d && conv2d_tile_ok(p, &nt, &nch, &tiles)) return take(kFamImageTile, tiles);
    // the gather forms hold a row's LayerNorm in one workgroup (<= 128 columns) and write no summaries beside it
    if (status == EPRECON_OK && p.ln && ((p.Cout + 31) / 32 > 4 || p.bn_partial || p.accumulate)) status = EPRECON_ERR_UNSUPPORTED;
    if (wide_ok(p)) return take(kFamWide, blocks_of(kWideRows));
    if (!direct2d && splitk_ok(p)) return take(kFamSplitK, blocks_of(kSplitKRows));
    if (direct) return take(kFamDirect16, blocks_of(direct16_partial_block_rows(p)));
    if (resident_narrow_ok(p)) return take(kFamResident, blocks_of(kRowsPerBlock));
    if (resident_wide_ok(p)) return take(kFamResidentWide, blocks_of(kRowsPerBlock));
    return take(kFamMfma, blocks_of(kRowsPerBlock));
}

int conv_dispatch_inner(ConvParams &p, hipStream_t st, ConvFamily *family_out = nullptr)
{
    const ConvChoice c = select_conv(p);
    if (c.status != EPRECON_OK) return c.status;
    g_last_conv_kernel = c.name;
    if (family_out) *family_out = c.family;
    switch (c.family) {
        case kFamDense3dNarrow: return launch_conv3d_single_column(p, st);
        case kFamDense3dTile16: return launch_conv3d_16(p, st);
        case kFamTile2d16: return launch_tile2d16(p, st);
        case kFamTile2dShort: return launch_tile2d_short(p, st);
        case kFamImageTile: return launch_image_tile(p, st);
        case kFamWide: return launch_wide(p, st);
        case kFamSplitK: return launch_splitk(p, st);
        case kFamDirect16: return launch_direct16(p, st);
        case kFamResident: return launch_resident_narrow(p, st);
        case kFamResidentWide: return launch_resident_wide(p, st);
        case kFamMfma: return launch_mfma(p, st);
    }
    return EPRECON_ERR_ARG;
}

int conv_dispatch(ConvParams &p, hipStream_t st)
{
    ConvProf &g = g_conv_prof;
    const bool hit = g.armed && p.K == g.K && p.Cin == g.cin && p.Cout == g.cout && p.n_out >= g.min_rows;
    // EPRECON_CONV_LOG=<file>: one line per launch (shape and the kernel that took it), in launch order, for joining with a
    // rocprofv3 kernel trace (tools/trace_cfg4_layers.py)
    static FILE *const layer_log = getenv("EPRECON_CONV_LOG") ? fopen(getenv("EPRECON_CONV_LOG"), "a") : nullptr;
    if (layer_log) {
        const int rc = conv_dispatch_inner(p, st);
        fprintf(layer_log, "%d %d %d %d %s ln=%d stats=%d acc=%d\n", p.n_out, p.K, p.Cin, p.Cout, g_last_conv_kernel, p.ln ? 1 : 0,
                p.bn_partial ? 1 : 0, p.accumulate ? 1 : 0);
        fflush(layer_log);
        return rc;
    }
    if (!hit) return conv_dispatch_inner(p, st);
    EP_HIP_CHECK(hipEventRecord(g.start, st));
    ConvFamily family = kFamMfma;
    const int rc = conv_dispatch_inner(p, st, &family);
    EP_HIP_CHECK(hipEventRecord(g.stop, st));
    g.armed = false;
    g.recorded = rc == EPRECON_OK;
    g.rows = p.n_out;
    g.kernel = g_last_conv_kernel;
    if (g.pairs_dev) {
        EP_HIP_CHECK(hipMemsetAsync(g.pairs_dev, 0, 2 * sizeof(unsigned long long), st));
        if (family == kFamDense3dNarrow || family == kFamDense3dTile16)
            hipLaunchKernelGGL(count_grid_pairs_kernel, dim3(256), dim3(256), 0, st, p.vox_rank, p.gx, p.gy, p.gz, g.pairs_dev);
        else if (p.nbr) {
            hipLaunchKernelGGL(count_map_pairs_kernel, dim3(256), dim3(256), 0, st, p.nbr, (size_t)p.K * p.n_out, g.pairs_dev);
            if (family == kFamDirect16)
                hipLaunchKernelGGL(count_map_groups_kernel, dim3(256), dim3(256), 0, st, p.nbr, p.n_out, p.K, g.pairs_dev + 1);
        } else  // identity map
            EP_HIP_CHECK(hipMemcpyAsync(g.pairs_dev, &g.rows, sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        EP_LAUNCH_CHECK();
    }
    return rc;
}

}  // namespace

// stage marker for kernel traces: an empty launch whose grid size carries the id
__global__ void profile_mark_kernel() {}
extern "C" int eprecon_profile_mark_async(int id, void *stream)
{
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(profile_mark_kernel, dim3((unsigned)id + 1), dim3(64), 0, st);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

extern "C" int eprecon_profile_conv_arm(int kvol, int cin, int cout, int64_t min_rows)
{
    ConvProf &g = g_conv_prof;
    if (!g.start) {
        EP_HIP_CHECK(hipEventCreate(&g.start));
        EP_HIP_CHECK(hipEventCreate(&g.stop));
        EP_HIP_CHECK(hipMalloc(&g.pairs_dev, 2 * sizeof(unsigned long long)));
    }
    g.K = kvol; g.cin = cin; g.cout = cout; g.min_rows = min_rows;
    g.armed = true;
    g.recorded = false;
    return EPRECON_OK;
}

extern "C" float eprecon_profile_conv_ms(int64_t *rows_out, const char **kernel_out)
{
    ConvProf &g = g_conv_prof;
    if (!g.recorded || hipEventSynchronize(g.stop) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, g.start, g.stop) != hipSuccess) return -1.0f;
    if (rows_out) *rows_out = g.rows;
    if (kernel_out) *kernel_out = g.kernel;
    return ms;
}

extern "C" const char *eprecon_profile_last_conv_kernel(void) { return g_last_conv_kernel; }

extern "C" int64_t eprecon_profile_conv_pairs(void)
{
    ConvProf &g = g_conv_prof;
    if (!g.recorded || !g.pairs_dev || hipEventSynchronize(g.stop) != hipSuccess) return -1;
    unsigned long long v = 0;
    if (hipMemcpy(&v, g.pairs_dev, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

extern "C" int64_t eprecon_profile_conv_executed_pairs(void)
{
    ConvProf &g = g_conv_prof;
    if (!g.recorded || !g.pairs_dev || hipEventSynchronize(g.stop) != hipSuccess) return -1;
    unsigned long long v = 0;
    if (hipMemcpy(&v, g.pairs_dev + 1, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;   // 0: the kernel that took the launch walks every offset of every row
}

extern "C" size_t eprecon_conv_bn_partial_bytes(int64_t n_out, int cout)
{
    return (size_t)ep::ceil_div(n_out > 0 ? n_out : 1, (int64_t)128) * 3 * (size_t)(cout > 0 ? cout : 1) * sizeof(float);
}

// bytes addressable from x: n_in rows of ld_x floats, the last one C_in floats rounded up to the 16-byte gathers
static int64_t conv_x_bytes(const ConvParams &p, int64_t n_in)
{
    return n_in > 0 ? ((n_in - 1) * (int64_t)p.ld_x + ((p.Cin + 3) & ~3)) * 4 : 0;
}

static int conv_check_and_run(ConvParams &p, int64_t n_in, int64_t n_out, void *stream)
{
    if (!p.x || !p.w || !p.out || n_in < 0 || n_out < 0 || p.K <= 0 || p.K > 64 || p.Cin <= 0 || p.Cout <= 0 ||
        p.ld_x < p.Cin || p.ld_out < p.Cout || (p.res && p.ld_res < p.Cout))
        return EPRECON_ERR_ARG;
    if (!p.nbr && !p.vox_rank && p.K != 1) return EPRECON_ERR_ARG;
    if (!p.nbr && n_in != n_out) return EPRECON_ERR_ARG;
    if ((p.in_scale == nullptr) != (p.in_shift == nullptr) || (p.res_scale == nullptr) != (p.res_shift == nullptr))
        return EPRECON_ERR_ARG;
    if (p.Cout > 4096 || n_out > 0x7fffffff) return EPRECON_ERR_UNSUPPORTED;
    if (n_out == 0) return EPRECON_OK;
    p.n_out = (int)n_out;
    p.x_bytes = conv_x_bytes(p, n_in);
    return conv_dispatch(p, (hipStream_t)stream);
}

// Descriptor form of the gather-GEMM (include/eprecon_hip.h: eprecon_conv_desc): every fused prologue /
// epilogue of the convolution blocks of the reference in one launch.
static void params_from_desc(ConvParams &p, const eprecon_conv_desc *d)
{
    p.x = d->x; p.nbr = d->nbr; p.w = d->weight; p.bias = d->bias; p.out = d->out;
    p.K = d->kvol; p.Cin = d->cin; p.Cout = d->cout; p.ld_x = d->ld_x; p.ld_out = d->ld_out;
    p.relu = d->relu; p.accumulate = d->accumulate;
    p.res = d->residual; p.ld_res = d->ld_res; p.bn_partial = d->bn_partial; p.bn_ld = d->bn_ld;
    p.in_scale = d->in_scale; p.in_shift = d->in_shift; p.in_relu = d->in_relu;
    p.res_scale = d->res_scale; p.res_shift = d->res_shift; p.res_relu = d->res_relu;
    p.ln = d->ln; p.ln_gamma = d->ln_gamma; p.ln_beta = d->ln_beta; p.ln_eps = d->ln_eps;
    p.ln_post_relu = d->ln_post_relu;
    p.img_h = d->img_h; p.img_w = d->img_w; p.img_maps = d->img_maps;
    p.vox_rank = d->vox_rank; p.gx = d->grid_x; p.gy = d->grid_y; p.gz = d->grid_z; p.wq = d->packed_weight;
    p.wq16 = d->packed_weight16;
    p.ws = d->workspace; p.ws_bytes = d->workspace_bytes;
    p.flex_partial = 1;
    p.bn_acc = d->bn_acc; p.bn_acc_ld = d->bn_acc_ld; p.bn_acc_c0 = d->bn_acc_c0; p.bn_gamma = d->bn_gamma; p.bn_beta = d->bn_beta;
    p.in_acc = d->in_acc; p.in_acc_ld = d->in_acc_ld; p.in_acc_c0 = d->in_acc_c0; p.in_eps = d->in_eps;
}

// What the descriptor's entry points ask the family rules with: the described launch with n_out / x_bytes set the way
// conv_check_and_run sets them.  false: no descriptor, or a row count that launches nothing (0, or more than 2^31 - 1 rows);
// p.n_out is 0 then.
static bool query_params(ConvParams &p, const eprecon_conv_desc *d)
{
    if (!d) return false;
    params_from_desc(p, d);
    const bool rows = d->n_out > 0 && d->n_out <= 0x7fffffff;
    p.n_out = rows ? (int)d->n_out : 0;
    p.x_bytes = conv_x_bytes(p, d->n_in);
    return rows;
}

extern "C" int eprecon_batchnorm_acc_affine_async(const long long *acc, int acc_ld, int acc_c0, int channels, float eps,
                                                  float *scale_out, float *shift_out, void *stream);

// BatchNorm form (c) — which launches take part.  PRODUCER: every kernel whose summaries go through conv_epilogue or
// direct_epilogue (all gather forms and the 2D image-tile kernel); the dense-grid 3D tile kernels keep their own epilogues.
// CONSUMER: the same families finish the accumulators in their prologue; for the others the library queues the stand-alone
// finish (one launch, like the finalize it replaces) into the caller's in_affine_scratch.
static bool bn_acc_family(const ConvParams &p) { return conv3d_kind(p) == kD3None; }

extern "C" size_t eprecon_bn_acc_words(int ld)
{
    return ld > 0 ? (size_t)epconv::kBnCopies * ld * epconv::kBnWords + (size_t)(2 * ld + 1) / 2 : 0;
}

extern "C" int eprecon_conv_desc_takes_bn_acc(const eprecon_conv_desc *d)
{
    ConvParams p = {};
    return query_params(p, d) && !p.ln && !p.accumulate && bn_acc_family(p) ? 1 : 0;
}

// which dense-grid kernel the described shape is for (0 none: the kernel map; 1 single column; 2 the 16-row kernel, which
// then wants packed_weight16): what a caller asks before it packs weights and drops the kernel map.  Dereferences nothing.
extern "C" int eprecon_conv_dense3d_kind(const eprecon_conv_desc *d)
{
    ConvParams p = {};
    return query_params(p, d) ? conv3d_shape_kind(p) : kD3None;
}

extern "C" int64_t eprecon_conv_desc_partial_rows(const eprecon_conv_desc *d);

extern "C" int eprecon_conv_desc_async(const eprecon_conv_desc *d, void *stream)
{
    if (!d) return EPRECON_ERR_ARG;
    ConvParams p = {};
    query_params(p, d);     // (an empty or oversized launch is conv_check_and_run's to answer)
    if (p.bn_partial) {     // row stride of the channel-major summaries: at least the rows this launch writes
        const int64_t rows = eprecon_conv_desc_partial_rows(d);
        if (p.bn_ld == 0) p.bn_ld = (int)(rows > 0 ? rows : 1);
        if (p.bn_ld < rows) return EPRECON_ERR_ARG;
    }
    if (p.bn_acc && (p.bn_acc_ld <= 0 || p.bn_acc_c0 < 0 || p.bn_acc_c0 + p.Cout > p.bn_acc_ld || p.ln || p.accumulate || !bn_acc_family(p)))
        return EPRECON_ERR_ARG;        // (ask eprecon_conv_desc_takes_bn_acc first)
    if (p.in_acc) {
        if (p.in_scale || p.in_shift || p.in_acc_ld <= 0 || p.in_acc_c0 < 0 || p.in_acc_c0 + p.Cin > p.in_acc_ld) return EPRECON_ERR_ARG;
        if (bn_acc_family(p)) {
            // (the kernels test in_scale for "there is a pending BatchNorm": any non-null value; stage_in_affine reads in_acc)
            p.in_scale = p.in_shift = reinterpret_cast<const float *>(p.in_acc);
        } else {
            if (!d->in_affine_scratch) return EPRECON_ERR_ARG;
            const int rc = eprecon_batchnorm_acc_affine_async(p.in_acc, p.in_acc_ld, p.in_acc_c0, p.Cin, p.in_eps, d->in_affine_scratch,
                                                              d->in_affine_scratch + p.Cin, stream);
            if (rc != EPRECON_OK) return rc;
            p.in_scale = d->in_affine_scratch;
            p.in_shift = d->in_affine_scratch + p.Cin;
            p.in_acc = nullptr;
        }
    }
    return conv_check_and_run(p, d->n_in, d->n_out, stream);
}

extern "C" size_t eprecon_conv_desc_workspace_bytes(const eprecon_conv_desc *d)
{
    ConvParams p = {};
    if (!query_params(p, d)) return 0;
    // (the two families that take scratch share no shape: the wide pair wants C_out > 64, the direct kernel at most 64)
    const size_t wide = wide_shape_ok(p) ? wide_workspace_bytes(p) : 0;
    const size_t direct = select_conv(p).family == kFamDirect16 ? direct16_workspace_bytes(p) : 0;
    return wide > direct ? wide : direct;
}

// rows of bn_partial the launch described by `d` writes (= the nblk to hand to
// eprecon_batchnorm_finalize_affine_async): the workgroups of the family select_conv gives the launch to
extern "C" int64_t eprecon_conv_desc_partial_rows(const eprecon_conv_desc *d)
{
    ConvParams p = {};
    return query_params(p, d) ? select_conv(p).partial_rows : 0;
}

// out = [ReLU]( sum_k x[nbr[k]] @ W[k] + bias [+ out] ) [+ residual]; optionally the per-workgroup
// BatchNorm summaries of the stored values (see conv_epilogue) -> bn_partial, to be consumed by
// eprecon_batchnorm_apply_partials_async.
extern "C" int eprecon_sparse_conv_fused_async(const float *x, int64_t n_in, int ld_x, const int32_t *nbr,
                                               int kvol, int64_t n_out, const float *weight, int cin,
                                               int cout, const float *bias, const float *residual,
                                               int ld_res, float *out, int ld_out, int relu,
                                               int accumulate, float *bn_partial, void *stream)
{
    ConvParams p = {};
    p.x = x; p.nbr = nbr; p.w = weight; p.bias = bias; p.out = out;
    p.K = kvol; p.Cin = cin; p.Cout = cout; p.ld_x = ld_x; p.ld_out = ld_out;
    p.relu = relu; p.accumulate = accumulate;
    p.res = residual; p.ld_res = ld_res; p.bn_partial = bn_partial;
    p.bn_ld = (int)ep::ceil_div(n_out > 0 ? n_out : 1, (int64_t)kRowsPerBlock);   // (no flex_partial: 128-row blocks only)
    return conv_check_and_run(p, n_in, n_out, stream);
}

extern "C" int eprecon_sparse_conv_async(const float *x, int64_t n_in, int ld_x, const int32_t *nbr,
                                         int kvol, int64_t n_out, const float *weight, int cin,
                                         int cout, const float *bias, float *out, int ld_out,
                                         int relu, int accumulate, void *stream)
{
    return eprecon_sparse_conv_fused_async(x, n_in, ld_x, nbr, kvol, n_out, weight, cin, cout, bias, nullptr, 0,
                                           out, ld_out, relu, accumulate, nullptr, stream);
}
