// ---------------------------------------------------------------------------------------------
// Group-resident variant for narrow layers (Cin <= 64): the weights of a GROUP of kernel offsets
// (up to ~24 KB, e.g. 9 offsets of a 32x32 layer) are staged per barrier instead of one 32-channel
// slab, so a 27-offset layer needs 3 barriers instead of 27, and four workgroups fit a CU.
// The gathers are issued in BATCHES of KB offsets (KB * NCH 16-byte loads per lane in flight)
// before the first MFMA of the batch: the per-offset loop with one offset of prefetch paid one
// memory latency (~1.5 us) per offset - 27 us of the 30 us a 20->20 3x3 layer took on 43,200 pixels,
// 40 of the 76 us of a 27-offset 32->32 layer.  Offsets with no live row in a wave's 32 rows are skipped.
// ---------------------------------------------------------------------------------------------
// (Included by sparse_conv_resident_nt{1,2}.hip, which instantiate the kernels of one column-tile count each — 24 instantiations per
// unit compile side by side; sparse_conv_slab.hip holds the eligibility rules and picks the unit.)
#pragma once
#include "common.hpp"
#include "conv_common.hpp"
#include "conv_gather.hpp"

namespace {
using namespace ep;
using namespace epconv;

// gather batch size: KB * NCH <= 16 float4 per lane in flight (<= 64 VGPRs of A operands)
constexpr int resident_kb(int nch) { return nch <= 1 ? 9 : nch == 2 ? 8 : nch == 3 ? 5 : nch == 4 ? 4 : nch == 5 ? 3 : 2; }

template <int NT, bool VEC4, int NCH, bool PIPE>
__global__ __launch_bounds__(256) void spconv_resident_kernel(ConvParams p, int kgroup, int nslab)
{
    // nslab > 1: wide inputs.  The input channels are walked in `nslab` slabs of cin_pad = 8 * NCH channels; per
    // slab the kernel is the narrow-layer kernel (offset groups resident in LDS, software-pipelined gathers), the
    // accumulators carry over.  One flat sequence of (slab, offset batch) steps, so the gather pipeline never drains.
    constexpr int cin_pad = NCH * 8;
    constexpr int KB = PIPE ? (resident_kb(NCH) + 1) / 2 : resident_kb(NCH);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TN = 32 * NT;
    float *sW = reinterpret_cast<float *>(smem);  // [kgroup][cin_pad][TN], zero padded; kgroup % KB == 0
    constexpr int per_k = cin_pad * TN;
    int *sNbr = reinterpret_cast<int *>(sW + kgroup * per_k);  // [K][128] neighbour tile
    const int cin_all = nslab * cin_pad;
    float *sAff = reinterpret_cast<float *>(sNbr + p.K * kRowsPerBlock);  // [2][cin_all] input scale / shift
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int r32 = lane & 31, half = lane >> 5;
    const int wrow0 = blockIdx.x * kRowsPerBlock + wave * kRowsPerWave;
    const int col0 = blockIdx.y * TN;
    const float *wbase = p.w + col0;
    stage_in_affine<256>(p, sAff, cin_all, tid);
    // the neighbour indices of the whole tile go to LDS up front: a gather then depends on ONE
    // memory latency (the rows), not two (index, then rows)
    for (int e = tid; e < p.K * kRowsPerBlock; e += 256) {
        const int k = e / kRowsPerBlock, r = e - k * kRowsPerBlock;
        const int row = blockIdx.x * kRowsPerBlock + r;
        sNbr[e] = row < p.n_out ? (p.nbr ? p.nbr[(size_t)k * p.n_out + row] : row) : -1;
    }
    __syncthreads();

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

    const int nb = (p.K + KB - 1) / KB;  // offset batches per slab
    const int total = nb * nslab;
    const int *nbr_row = sNbr + wave * kRowsPerWave + r32;
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.x), 0, PIPE ? (int)p.x_bytes : 0, 0x00020000);
    const unsigned row_bytes = (unsigned)p.ld_x * 4u, oob = (unsigned)p.x_bytes;
    auto issue = [&](int b, ARows(&a)[KB], int(&jj)[KB]) {
        const int sl = min(b / nb, nslab - 1);
        const int kb = (b - (b / nb) * nb) * KB;
        const bool in = b < total;
#pragma unroll
        for (int u = 0; u < KB; ++u) jj[u] = (in && kb + u < p.K) ? nbr_row[min(kb + u, p.K - 1) * kRowsPerBlock] : -1;
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            if (PIPE) gather_rows_buf<NCH>(rsrc, row_bytes, oob, jj[u], half, a[u], sl * cin_pad * 4);
            else gather_rows<VEC4, NCH>(p, jj[u], half, a[u], sl * cin_pad);
        }
    };
    auto consume = [&](int b, ARows(&a)[KB], int(&jj)[KB]) {
        const int sl = b / nb;
        const int kb = (b - sl * nb) * KB;
        const int cbase = sl * cin_pad;
        if (PIPE && cbase + cin_pad > p.Cin) {  // ragged channel count: what the last chunk read past C_in is not data
#pragma unroll
            for (int u = 0; u < KB; ++u) fix_rows<NCH>(p, jj[u], half, a[u], cbase);
        }
        // ---- weights of the group this batch belongs to (loads above stay in flight) ----
        const int k0 = kb / kgroup * kgroup;
        if (kb == k0) {
            const int kn = min(kgroup, p.K - k0);
            __syncthreads();  // every wave is done with the previous group's weights
            stage_weights_quads<NT, NCH>(sW, p, k0, kn, cbase, col0, tid);
            __syncthreads();
        }
        // ---- MFMAs of the batch ----
#pragma unroll
        for (int u = 0; u < KB; ++u) {
            if (kb + u >= p.K) break;
            const bool live = __ballot(jj[u] >= 0) != 0ull;
            if (!live) continue;
            const float *wk = sW + (kb + u - k0) * per_k + (half * NT * 32 + r32) * 4;
            if (p.in_scale) {
                // BatchNorm (+ReLU) of the producer applied to the gathered values; padding stays 0
                const bool ok = jj[u] >= 0;
#pragma unroll
                for (int ch = 0; ch < NCH; ++ch) {
                    const float4 sc = *reinterpret_cast<const float4 *>(sAff + cbase + ch * 8 + 4 * half);
                    const float4 sh = *reinterpret_cast<const float4 *>(sAff + cin_all + cbase + ch * 8 + 4 * half);
                    const float scv[4] = {sc.x, sc.y, sc.z, sc.w}, shv[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        float v = fmaf(a[u].v[ch][s], scv[s], shv[s]);
                        if (p.in_relu) v = fmaxf(v, 0.0f);
                        a[u].v[ch][s] = (ok && cbase + ch * 8 + 4 * half + s < p.Cin) ? v : 0.0f;
                    }
                }
            }
            // B operands: one 16-byte LDS read per (chunk, column block) gives the four channel steps of this lane.  The
            // reads of the first two chunks are issued ahead of the first MFMAs and the rest between MFMA groups
            // (sched_group_barrier: left alone the scheduler sinks each read to just in front of its MFMA pair and
            // every pair then sits behind an LDS round trip).
            float4 bq[NCH][NT];
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    bq[ch][t] = *reinterpret_cast<const float4 *>(wk + (ch * 2 * NT + t) * 128);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch)
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][0], bq[ch][t].x, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][1], bq[ch][t].y, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][2], bq[ch][t].z, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u].v[ch][3], bq[ch][t].w, acc[t], 0, 0, 0);
                }
            __builtin_amdgcn_sched_group_barrier(0x100, NCH >= 2 ? 2 * NT : NT, 0);   // DS reads of the first two chunks
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                __builtin_amdgcn_sched_group_barrier(0x008, 4 * NT, 0);               // MFMAs of chunk ch
                if (ch + 2 < NCH) __builtin_amdgcn_sched_group_barrier(0x100, NT, 0);   // reads of chunk ch + 2
            }
        }
    };
    if (PIPE) {
        // software pipeline: the gathers of step b+1 are always issued (clamped past the end) before the
        // MFMAs of step b, so exactly KB * NCH loads are younger than the ones being waited for
        ARows a0[KB], a1[KB];
        int j0[KB], j1[KB];
        issue(0, a0, j0);
        for (int b = 0; b < total; b += 2) {
            issue(b + 1, a1, j1);
            consume(b, a0, j0);
            issue(b + 2, a0, j0);
            if (b + 1 < total) consume(b + 1, a1, j1);
        }
    } else {
        for (int b = 0; b < total; ++b) {
            ARows a[KB];
            int jj[KB];
            issue(b, a, jj);
            consume(b, a, jj);
        }
    }
    conv_epilogue<NT>(p, acc, LinearRows{wrow0, p.n_out}, col0, r32, half, wave, sW, (int)blockIdx.x, (int)gridDim.y);
}

template <int NT, int NCH>
int launch_resident_nch(const ConvParams &p, bool vec4, hipStream_t st, int nslab = 1)
{
    // weights of `kgroup` offsets resident at a time (a multiple of the gather batch, ~24 KB -> 4 workgroups per CU)
    // vec4: 16-byte aligned rows whose pitch covers Cin rounded up to 4; the buffer-load gathers address x with
    // 32-bit byte offsets formed by a 24-bit multiply
    const bool pipe = vec4 && p.x_bytes > 0 && p.x_bytes < 0x7fffffffll && (int64_t)p.ld_x * 4 < (1 << 24) &&
                      p.x_bytes / ((int64_t)p.ld_x * 4) < (1 << 24);
    const int KB = pipe ? (resident_kb(NCH) + 1) / 2 : resident_kb(NCH);  // the kernel's batch size: kgroup % KB == 0
    const size_t per_k = (size_t)NCH * 8 * 32 * NT * sizeof(float);
    constexpr int group_kb = 24;   // (36 KB: -1 %, 48 KB = two workgroups per CU: +37 %)
    int kgroup = (int)max((size_t)KB, (size_t)(group_kb * 1024) / per_k / KB * KB);
    kgroup = min(kgroup, (p.K + KB - 1) / KB * KB);
    const size_t lds = max((size_t)kgroup * per_k + (size_t)p.K * kRowsPerBlock * sizeof(int) +
                               (size_t)2 * nslab * NCH * 8 * sizeof(float),
                           max((size_t)kWaves * 3 * 32 * NT, (size_t)3 * 256) * sizeof(float));
    const dim3 grid((unsigned)ceil_div(p.n_out, kRowsPerBlock), (unsigned)ceil_div(p.Cout, 32 * NT));
    if (pipe)
        hipLaunchKernelGGL((spconv_resident_kernel<NT, true, NCH, true>), grid, dim3(256), lds, st, p, kgroup, nslab);
    else if (vec4)
        hipLaunchKernelGGL((spconv_resident_kernel<NT, true, NCH, false>), grid, dim3(256), lds, st, p, kgroup, nslab);
    else
        hipLaunchKernelGGL((spconv_resident_kernel<NT, false, NCH, false>), grid, dim3(256), lds, st, p, kgroup, nslab);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

template <int NT>
int launch_resident(const ConvParams &p, bool vec4, int cin_pad, hipStream_t st)
{
    // wide inputs: the fewest slabs of at most 64 channels, all of the same width (8 * NCH)
    const int chunks = cin_pad / 8;
    const int nslab = (chunks + 7) / 8;
    const int nch = (chunks + nslab - 1) / nslab;
    switch (nch) {
        case 1: return launch_resident_nch<NT, 1>(p, vec4, st, nslab);
        case 2: return launch_resident_nch<NT, 2>(p, vec4, st, nslab);
        case 3: return launch_resident_nch<NT, 3>(p, vec4, st, nslab);
        case 4: return launch_resident_nch<NT, 4>(p, vec4, st, nslab);
        case 5: return launch_resident_nch<NT, 5>(p, vec4, st, nslab);
        case 6: return launch_resident_nch<NT, 6>(p, vec4, st, nslab);
        case 7: return launch_resident_nch<NT, 7>(p, vec4, st, nslab);
        default: return launch_resident_nch<NT, 8>(p, vec4, st, nslab);
    }
}
}  // namespace
