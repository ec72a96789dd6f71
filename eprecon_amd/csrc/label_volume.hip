// Scene ground truth from a labelled point cloud on gfx950: the two label steps the reference runs offline on the CPU.
//
// A. Label volumes (integrate_semantic, tools/tsdf_fusion/generate_gt.py:77-114, with the coordinate step of :199-202):
//      cell   = clip(rint((xyz - vol_min) / voxel_size), 0, dim - 1)        float64, ties to even (np.round)
//      colour = float64 sum of the cell's points IN ASCENDING POINT INDEX / max(count, 1)      (np.bincount(weights=...))
//      label  = the cell's most frequent label, the SMALLEST on a tie (np.argmax over the count table); 0 for an empty cell
//    Three steps on the caller's stream: one thread per point for the cell index (and the label range check), the CSR point
//    lists of eprecon_segment_lists_async (ascending point index inside a cell: the sums are bit-reproducible), one vote launch
//    with a thread per cell.  A list of at most kShortList points is voted by its own thread (count the equals of every entry:
//    <= 64 compares); longer lists are taken one after the other by the whole wave (a ballot names them): 64 entries per step
//    sit in the lanes, every lane counts the equals of its own entry over the list by lane broadcasts, and a wave maximum over
//    (count, -label) names the mode.  No [cells x labels] table, no float atomics, no sort; the label range plays no part
//    (instance ids run into the hundreds).  The work of a long list grows with length^2 / 64 broadcasts: 16 cm cells of a
//    ScanNet cloud hold hundreds of points, i.e. a few thousand broadcasts per cell.
//
// B. Nearest-label fill (datasets/scannet/label_interpolate.py:25-48): every cell takes the label of a nearest non-zero cell
//    (Euclidean distance in index space).  Exact separable squared-distance transform carrying the label, int32 throughout:
//      pass z:  (d2, label) of the nearest site in the cell's own z column           (d2 = kNoSite when the column has none)
//      pass y:  min over the cell's y line of dy^2 + d2, keeping that entry's label
//      pass x:  the same along x.
//    One kernel does all three: a block stages a slab of lines in LDS (16 neighbouring lines for y / x — neighbours along z,
//    so global accesses are 64-byte runs; whole z columns, contiguous, for z), then every cell walks outward from its own
//    position, -k before +k, and stops at k^2 >= best: the cost follows the distance to the surface, not the line length.
//    An entry replaces the best only when STRICTLY smaller, which fixes the tie rule: among the sites at the minimal distance
//    the one with the smallest |dx|, then the lower x, then the smallest |dy|, the lower y, the smallest |dz|, the lower z.
//    kNoSite = 2^30 - 1: with dims <= 4,096 a real d2 is at most 3 * 4095^2 < 2^26 and kNoSite + 4095^2 < 2^31.
#include <math.h>

#include "common.hpp"

namespace {
using namespace ep;

constexpr int kShortList = 8;
constexpr int32_t kNoSite = 0x3fffffff;
constexpr int kMaxAxis = 4096;
constexpr int kMaxLabel = 32767;

__global__ __launch_bounds__(256) void label_cells_kernel(const double *xyz, const int64_t *sem, const int64_t *ins, int64_t n,
                                                          double m0, double m1, double m2, double vs, int d0, int d1, int d2,
                                                          int32_t *cell, int32_t *bad)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    // fmax / fmin drop a NaN: such a point lands in cell 0 of its axis
    const double cx = fmin(fmax(rint((xyz[3 * i] - m0) / vs), 0.0), (double)(d0 - 1));
    const double cy = fmin(fmax(rint((xyz[3 * i + 1] - m1) / vs), 0.0), (double)(d1 - 1));
    const double cz = fmin(fmax(rint((xyz[3 * i + 2] - m2) / vs), 0.0), (double)(d2 - 1));
    cell[i] = ((int)cx * d1 + (int)cy) * d2 + (int)cz;
    const int64_t s = sem[i], t = ins[i];
    if (s < 0 || s > kMaxLabel || t < 0 || t > kMaxLabel) *bad = 1;
}

// wave maximum of a 64-bit key
__device__ __forceinline__ long long wave_max_key(long long k)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const long long other = __shfl_xor(k, o);
        k = other > k ? other : k;
    }
    return k;
}

__global__ __launch_bounds__(256) void label_vote_kernel(const int32_t *offsets, const int32_t *order, const double *rgb,
                                                         const int64_t *sem, const int64_t *ins, int64_t cells, double *rgb_out,
                                                         int64_t *sem_out, int64_t *ins_out)
{
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & (kWave - 1);
    const bool live = cell < cells;
    int start = 0, len = 0;
    if (live) {
        start = offsets[cell];
        len = offsets[cell + 1] - start;
    }
    if (live && len <= kShortList) {
        double r = 0.0, g = 0.0, b = 0.0;
        int best_s = 0, cnt_s = 0, best_i = 0, cnt_i = 0;
        for (int i = 0; i < len; ++i) {
            const int64_t p = order[start + i];
            r += rgb[3 * p];
            g += rgb[3 * p + 1];
            b += rgb[3 * p + 2];
            const int si = (int)sem[p], ii = (int)ins[p];
            int cs = 0, ci = 0;
            for (int j = 0; j < len; ++j) {
                const int64_t q = order[start + j];
                cs += (int)sem[q] == si;
                ci += (int)ins[q] == ii;
            }
            if (cs > cnt_s || (cs == cnt_s && si < best_s)) { cnt_s = cs; best_s = si; }
            if (ci > cnt_i || (ci == cnt_i && ii < best_i)) { cnt_i = ci; best_i = ii; }
        }
        const double den = (double)(len > 1 ? len : 1);
        rgb_out[3 * cell] = r / den;
        rgb_out[3 * cell + 1] = g / den;
        rgb_out[3 * cell + 2] = b / den;
        sem_out[cell] = best_s;
        ins_out[cell] = best_i;
    }
    // the long lists of this wave's 64 cells, one at a time by all 64 lanes (everything below is wave-uniform)
    unsigned long long todo = __ballot(live && len > kShortList);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int s0 = __shfl(start, src), l0 = __shfl(len, src);
        const int64_t c0 = cell - lane + src;
        double ar = 0.0, ag = 0.0, ab = 0.0;
        for (int base = 0; base < l0; base += kWave) {
            const int m = l0 - base < kWave ? l0 - base : kWave;
            double r = 0.0, g = 0.0, b = 0.0;
            if (lane < m) {
                const int64_t p = order[s0 + base + lane];
                r = rgb[3 * p];
                g = rgb[3 * p + 1];
                b = rgb[3 * p + 2];
            }
            for (int t = 0; t < m; ++t) {     // ascending point index: every lane carries the same running sums
                ar += __shfl(r, t);
                ag += __shfl(g, t);
                ab += __shfl(b, t);
            }
        }
        long long key_s = -1, key_i = -1;
        for (int ib = 0; ib < l0; ib += kWave) {
            const int mi = l0 - ib < kWave ? l0 - ib : kWave;
            int my_s = -1, my_i = -1;
            if (lane < mi) {
                const int64_t p = order[s0 + ib + lane];
                my_s = (int)sem[p];
                my_i = (int)ins[p];
            }
            int cs = 0, ci = 0;
            for (int jb = 0; jb < l0; jb += kWave) {
                const int mj = l0 - jb < kWave ? l0 - jb : kWave;
                int js = -2, ji = -2;
                if (lane < mj) {
                    const int64_t q = order[s0 + jb + lane];
                    js = (int)sem[q];
                    ji = (int)ins[q];
                }
                for (int t = 0; t < mj; ++t) {
                    cs += __shfl(js, t) == my_s;
                    ci += __shfl(ji, t) == my_i;
                }
            }
            if (lane < mi) {      // more votes first, then the smaller label (labels are 15 bits; a bad one is reported anyway)
                const long long ks = ((long long)cs << 16) | (long long)(kMaxLabel - (my_s & kMaxLabel));
                const long long ki = ((long long)ci << 16) | (long long)(kMaxLabel - (my_i & kMaxLabel));
                key_s = ks > key_s ? ks : key_s;
                key_i = ki > key_i ? ki : key_i;
            }
        }
        key_s = wave_max_key(key_s);
        key_i = wave_max_key(key_i);
        if (lane == 0) {
            const double den = (double)l0;
            rgb_out[3 * c0] = ar / den;
            rgb_out[3 * c0 + 1] = ag / den;
            rgb_out[3 * c0 + 2] = ab / den;
            sem_out[c0] = kMaxLabel - (int)(key_s & 0xffff);
            ins_out[c0] = kMaxLabel - (int)(key_i & 0xffff);
        }
    }
}

// One pass of the distance transform along an axis of length L whose elements are `inner` cells apart.  Line q (of
// n_lines = cells / L) starts at (q / inner) * L * inner + q % inner.  A block takes TL = 1 << tl_log2 consecutive lines.
// ZPASS (inner == 1): LDS index = line * L + p, the slab is one contiguous run of global memory.
// otherwise:          LDS index = p * TL + line, so a wave reads 4 positions x 16 neighbouring z: 64-byte runs in global
//                     memory, consecutive words (no bank conflict) in LDS.
// FIRST: the input is the label volume itself (d2 = 0 at a site, kNoSite elsewhere).  d2 / lab are updated in place: a block
// reads its whole slab before it writes, and no other block touches those lines.
template <bool ZPASS, bool FIRST>
__global__ __launch_bounds__(256) void label_fill_pass_kernel(const int32_t *vol, int32_t *d2, int32_t *lab, int64_t n_lines,
                                                              int L, int64_t inner, int tl_log2)
{
    extern __shared__ int32_t lds[];
    const int TL = 1 << tl_log2;
    int32_t *sd = lds, *sl = lds + (size_t)TL * L;
    const int64_t q0 = (int64_t)blockIdx.x * TL;
    const int total = TL * L;
    // non-ZPASS: 256 % TL == 0, so a thread keeps its line over the whole loop
    const int my_line = threadIdx.x & (TL - 1);
    const int64_t q = q0 + my_line;
    const int64_t o = q / inner;
    const int64_t line_base = o * L * inner + (q - o * inner);
    const bool line_live = q < n_lines;
    const int64_t live_total = (n_lines - q0 < TL ? n_lines - q0 : TL) * L;     // ZPASS: elements of the lines that exist

    for (int e = threadIdx.x; e < total; e += 256) {
        int64_t addr;
        if (ZPASS) {
            if (e >= live_total) break;
            addr = q0 * L + e;
        } else {
            if (!line_live) break;
            addr = line_base + (int64_t)(e >> tl_log2) * inner;
        }
        int32_t d, l;
        if (FIRST) {
            l = vol[addr];
            d = l != 0 ? 0 : kNoSite;
        } else {
            d = d2[addr];
            l = lab[addr];
        }
        sd[e] = d;
        sl[e] = l;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < total; e += 256) {
        int64_t addr;
        int p, step;
        if (ZPASS) {
            if (e >= live_total) break;
            addr = q0 * L + e;
            p = e % L;
            step = 1;
        } else {
            if (!line_live) break;
            p = e >> tl_log2;
            addr = line_base + (int64_t)p * inner;
            step = TL;
        }
        int32_t best = sd[e], bl = sl[e];
        const int kmax = p > L - 1 - p ? p : L - 1 - p;
        for (int k = 1; k <= kmax; ++k) {
            const int kk = k * k;
            if (kk >= best) break;
            if (k <= p) {
                const int32_t c = sd[e - k * step] + kk;
                if (c < best) { best = c; bl = sl[e - k * step]; }
            }
            if (p + k < L) {
                const int32_t c = sd[e + k * step] + kk;
                if (c < best) { best = c; bl = sl[e + k * step]; }
            }
        }
        d2[addr] = best;
        lab[addr] = bl;
    }
}

template <bool ZPASS, bool FIRST>
int launch_fill_pass(const int32_t *vol, int32_t *d2, int32_t *lab, int64_t cells, int L, int64_t inner, hipStream_t st)
{
    // slab = TL lines x L cells x (d2, label) = 8 TL L bytes, kept at or below 64 KB (L <= 4,096): 16 lines up to L = 512
    // (34.6 KB at 270: four blocks, 16 waves, per CU), halved from there on; z columns are packed to about 32 KB
    int tl_log2;
    if (ZPASS) {
        tl_log2 = 0;
        while (tl_log2 < 6 && ((size_t)2 << tl_log2) * L <= 4096) ++tl_log2;
    } else {
        tl_log2 = 4;
        while (tl_log2 > 0 && ((size_t)8 << tl_log2) * L > 65536) --tl_log2;
    }
    const int64_t n_lines = cells / L;
    const int64_t blocks = ceil_div(n_lines, (int64_t)1 << tl_log2);
    const size_t lds_bytes = ((size_t)8 << tl_log2) * L;
    hipLaunchKernelGGL((label_fill_pass_kernel<ZPASS, FIRST>), dim3((unsigned)blocks), dim3(256), lds_bytes, st, vol, d2, lab,
                       n_lines, L, inner, tl_log2);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

struct LabelVolumesLayout {
    size_t cell, offsets, order, bad, segment, total;
};

LabelVolumesLayout label_volumes_layout(int64_t n, int64_t cells)
{
    LabelVolumesLayout w;
    const size_t n1 = (size_t)(n > 0 ? n : 1), c1 = (size_t)(cells > 0 ? cells : 1);
    w.cell = 0;
    w.offsets = w.cell + align_up(n1 * 4, 256);
    w.order = w.offsets + align_up((c1 + 1) * 4, 256);
    w.bad = w.order + align_up(n1 * 4, 256);
    w.segment = w.bad + 256;
    w.total = w.segment + eprecon_segment_workspace_bytes(n, cells);
    return w;
}

}  // namespace

extern "C" size_t eprecon_label_volumes_workspace_bytes(int64_t n, int64_t cells)
{
    return label_volumes_layout(n, cells).total;
}

extern "C" int eprecon_label_volumes(const double *xyz, const double *rgb, const int64_t *semantic, const int64_t *instance,
                                     int64_t n, const double *vol_min_host, double voxel_size, const int32_t *dims_host,
                                     double *rgb_out, int64_t *semantic_out, int64_t *instance_out, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    if (n < 0 || !vol_min_host || !dims_host || !rgb_out || !semantic_out || !instance_out || !workspace ||
        !(voxel_size > 0.0) || (n > 0 && (!xyz || !rgb || !semantic || !instance)))
        return EPRECON_ERR_ARG;
    int64_t cells = 1;
    for (int k = 0; k < 3; ++k) {
        if (dims_host[k] <= 0) return EPRECON_ERR_ARG;
        if (dims_host[k] > (1 << 20)) return EPRECON_ERR_UNSUPPORTED;
        cells *= dims_host[k];
        if (cells > 0x7fffffff - 256) return EPRECON_ERR_UNSUPPORTED;        // int32 cell ids and list offsets
    }
    if (n > 0x7fffffff - 256) return EPRECON_ERR_UNSUPPORTED;
    const LabelVolumesLayout w = label_volumes_layout(n, cells);
    if (workspace_bytes < w.total) return EPRECON_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char *ws = reinterpret_cast<char *>(workspace);
    int32_t *cell = reinterpret_cast<int32_t *>(ws + w.cell);
    int32_t *offsets = reinterpret_cast<int32_t *>(ws + w.offsets);
    int32_t *order = reinterpret_cast<int32_t *>(ws + w.order);
    int32_t *bad = reinterpret_cast<int32_t *>(ws + w.bad);
    EP_HIP_CHECK(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    if (n > 0) {
        hipLaunchKernelGGL(label_cells_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, st, xyz, semantic, instance, n,
                           vol_min_host[0], vol_min_host[1], vol_min_host[2], voxel_size, dims_host[0], dims_host[1],
                           dims_host[2], cell, bad);
        EP_LAUNCH_CHECK();
    }
    const int rc = eprecon_segment_lists_async(cell, n, cells, offsets, order, ws + w.segment, workspace_bytes - w.segment, stream);
    if (rc != EPRECON_OK) return rc;
    hipLaunchKernelGGL(label_vote_kernel, dim3((unsigned)ceil_div(cells, 256)), dim3(256), 0, st, (const int32_t *)offsets,
                       (const int32_t *)order, rgb, semantic, instance, cells, rgb_out, semantic_out, instance_out);
    EP_LAUNCH_CHECK();
    int32_t bad_host = 0;
    EP_HIP_CHECK(hipMemcpyAsync(&bad_host, bad, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    EP_HIP_CHECK(hipStreamSynchronize(st));
    return bad_host ? EPRECON_ERR_ARG : EPRECON_OK;
}

extern "C" size_t eprecon_label_fill_workspace_bytes(int dx, int dy, int dz)
{
    if (dx <= 0 || dy <= 0 || dz <= 0) return 0;
    return align_up((size_t)dx * dy * dz * 4, 256);
}

extern "C" int eprecon_label_fill_async(const int32_t *vol, const int32_t *dims_host, int32_t *out, void *workspace,
                                        size_t workspace_bytes, void *stream)
{
    if (!dims_host) return EPRECON_ERR_ARG;
    for (int k = 0; k < 3; ++k)
        if (dims_host[k] <= 0) return EPRECON_ERR_ARG;
    for (int k = 0; k < 3; ++k)
        if (dims_host[k] > kMaxAxis) return EPRECON_ERR_UNSUPPORTED;
    if (!vol || !out || !workspace) return EPRECON_ERR_ARG;
    const int dx = dims_host[0], dy = dims_host[1], dz = dims_host[2];
    if (workspace_bytes < eprecon_label_fill_workspace_bytes(dx, dy, dz)) return EPRECON_ERR_WORKSPACE;
    const int64_t cells = (int64_t)dx * dy * dz;
    hipStream_t st = (hipStream_t)stream;
    int32_t *d2 = reinterpret_cast<int32_t *>(workspace);
    int rc = launch_fill_pass<true, true>(vol, d2, out, cells, dz, 1, st);
    if (rc != EPRECON_OK) return rc;
    rc = launch_fill_pass<false, false>(nullptr, d2, out, cells, dy, dz, st);
    if (rc != EPRECON_OK) return rc;
    return launch_fill_pass<false, false>(nullptr, d2, out, cells, dx, (int64_t)dy * dz, st);
}
