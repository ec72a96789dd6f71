// ---------------------------------------------------------------------------------------------
// Dense-grid 3x3x3 stride-1 convolution: the 3D twin of conv2d_tile_kernel, for voxel sets that fill most of their
// bounding grid (the initialisation stack runs on 85 % of the dense 48^3 grid, models/occupancy_initialization.py:131-174).
// The gather form re-reads every input row 27 times through L1/L2 behind a [27][N] kernel map and pays a memory
// latency per batch of offsets (73 us for 32 -> 32 on 94k voxels, 0.40 of the MFMA bound; ablation: gathers alone 53 us).
// Here a workgroup owns a 4 x 4 x 8 block of grid cells (x slowest, z fastest = the row order of a raster-ordered set):
//   1. the rank volume gives the row of each of the 6 x 6 x 10 halo cells (-1: no voxel)          -> LDS (360 ints)
//   2. the halo rows are staged ONCE with coalesced 16-byte loads, the producer's pending BatchNorm (+ReLU) applied on
//      the way in, zeros where there is no voxel                                                   -> LDS (360 x (C_in + 4) floats)
//   3. the 27 offsets read their A operands from LDS with one ds_read_b128 per 8-channel chunk at compile-time offsets
//      (no address arithmetic in the loop).  B operands do NOT go through LDS: the weights are pre-packed in operand
//      order (pack_weights_kernel), so a wave fetches the four channel steps of a chunk with ONE coalesced 1 KB
//      global_load_dwordx4 (L1 / L2 hits: every wave of the chip reads the same 27 * C_in * C_out * 4 bytes), issued two
//      chunks ahead of its MFMAs.  No weight staging, no barrier inside the MFMA loop, 53 KB of LDS at C_in = 32:
//      three workgroups per CU, so one workgroup's staging overlaps the others' MFMAs.
//   4. the shared epilogue (bias, ReLU, residual, BatchNorm summaries or row-wise LayerNorm); rows are addressed
//      through the ranks, cells without a voxel are computed and dropped.
// Bit-identical to the gather kernels: the same k-ordered fma chain per output element, zeros for missing neighbours.
// No kernel map and no hash grid are needed for such layers.
//   wave w -> x = x0 + w; MFMA row r32 -> (y, z) = (y0 + r32 / 8, z0 + r32 % 8)
// ---------------------------------------------------------------------------------------------
#include <stdlib.h>

#include "common.hpp"
#include "conv_common.hpp"
#include "conv_gather.hpp"

namespace {
using namespace ep;
using namespace epconv;

// tile = WV x 4 x 8 cells, one wave per x slice (WV waves per workgroup).  WV = 2 for the MFMA kernel: what balances the
// chip is the number of 32-row wave jobs (11.5 us of MFMAs each at C_in = C_out = 32) per SIMD, and 64-cell workgroups
// with a 35 KB halo fit four to a CU where 128-cell workgroups with 52 KB fit three and ran the 94k-voxel layer in two
// rounds (measured 88 us against 73 us for the gather form; profiles/r03/conv3d_probe.txt)
constexpr int kD3Y = 4, kD3Z = 8;
constexpr int kD3HY = kD3Y + 2, kD3HZ = kD3Z + 2;
constexpr int d3_halo(int wv) { return (wv + 2) * kD3HY * kD3HZ; }
constexpr int kD3WvNarrow = 4;

template <int WV>
__device__ __forceinline__ void d3_tile_origin(int tile, int tiles_y, int tiles_z, int &x0, int &y0, int &z0)
{
    const int tz = tile % tiles_z, ty = (tile / tiles_z) % tiles_y, tx = tile / (tiles_z * tiles_y);
    x0 = tx * WV; y0 = ty * kD3Y; z0 = tz * kD3Z;
}

// steps 1 + 2 of the tile kernels: the row (rank) of every halo cell -> the first pad word of the cell, halo rows -> sX
// (pitch P = cin_pad + 4 floats; no separate rank array: 51,840 bytes at C_in = 32, three workgroups per CU).
// Returns false (block-uniform) when no cell of the tile holds a voxel.
__device__ __forceinline__ int d3_rank(const float *sX, int cell, int P, int cin_pad) { return __float_as_int(sX[cell * P + cin_pad]); }

// step 1: rows (ranks) of the halo cells -> the first pad word of each cell; false (block-uniform) for a tile without a voxel
template <int NCH, int WV, int THREADS = 64 * WV>
__device__ __forceinline__ bool d3_stage_ranks(const ConvParams &p, int x0, int y0, int z0, float *sX, int tid)
{
    constexpr int cin_pad = NCH * 8, P = cin_pad + 4;
    constexpr int kThreads = THREADS, kD3Halo = d3_halo(WV);
    for (int e = tid; e < kD3Halo; e += kThreads) {
        const int hz = e % kD3HZ, hy = (e / kD3HZ) % kD3HY, hx = e / (kD3HZ * kD3HY);
        const int x = x0 - 1 + hx, y = y0 - 1 + hy, z = z0 - 1 + hz;
        const bool in = x >= 0 && x < p.gx && y >= 0 && y < p.gy && z >= 0 && z < p.gz;
        sX[e * P + cin_pad] = __int_as_float(in ? p.vox_rank[((size_t)x * p.gy + y) * p.gz + z] : -1);
    }
    __syncthreads();
    // this thread's output cell (the threads cover the 32 WV cells at least once)
    const int v = tid % (32 * WV);
    const int own = d3_rank(sX, (((v >> 5) + 1) * kD3HY + ((v >> 3) & 3) + 1) * kD3HZ + (v & 7) + 1, P, cin_pad);
    return __syncthreads_or(own >= 0) != 0;
}

// step 2: channels [cbase, cbase + 8 NCH) of the halo rows -> sX (pitch P = 8 NCH + 4 floats), the producer's pending BatchNorm
// (+ReLU) applied on the way in, zeros where there is no voxel or no channel.  Ends with a barrier.
template <int NCH, int WV, int THREADS = 64 * WV>
__device__ __forceinline__ void d3_stage_rows(const ConvParams &p, float *sX, int tid, int dbg, int cbase)
{
    constexpr int cin_pad = NCH * 8, P = cin_pad + 4, C4 = cin_pad / 4;
    constexpr int kThreads = THREADS, kD3Halo = d3_halo(WV);
    constexpr int kItems = kD3Halo * C4;
    constexpr int kIter = (kItems + kThreads - 1) / kThreads;
    float4 hv[kIter];
    int hr[kIter];
    const int last4 = ((p.Cin + 3) & ~3) - 4;
    // the channel group of an item is tid % C4 in every iteration when C4 divides the block size: its scale / shift are loaded once
    constexpr bool kFixedGroup = kThreads % C4 == 0;
    float4 sc0 = make_float4(1.f, 1.f, 1.f, 1.f), sh0 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kFixedGroup && p.in_scale) {
        sc0 = *reinterpret_cast<const float4 *>(p.in_scale + min(cbase + (tid % C4) * 4, last4));
        sh0 = *reinterpret_cast<const float4 *>(p.in_shift + min(cbase + (tid % C4) * 4, last4));
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {  // all loads first (clamped addresses), then the fix-ups and LDS stores
        const int e = min(tid + it * kThreads, kItems - 1);
        const int cell = e / C4, c4 = e - cell * C4;
        hr[it] = d3_rank(sX, cell, P, cin_pad);
        if (dbg & 4) hv[it] = make_float4(1.f, 1.f, 1.f, 1.f);
        else hv[it] = *reinterpret_cast<const float4 *>(p.x + (size_t)max(hr[it], 0) * p.ld_x + min(cbase + c4 * 4, last4));
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int e = tid + it * kThreads;
        if (e >= kItems) break;
        const int cell = e / C4, c4 = e - cell * C4;
        const int c = cbase + c4 * 4;
        float4 v4 = hv[it];
        if (p.in_scale) {
            float4 sc = sc0, sh = sh0;
            if (!kFixedGroup) {
                sc = *reinterpret_cast<const float4 *>(p.in_scale + min(c, last4));
                sh = *reinterpret_cast<const float4 *>(p.in_shift + min(c, last4));
            }
            v4.x = fmaf(v4.x, sc.x, sh.x); v4.y = fmaf(v4.y, sc.y, sh.y);
            v4.z = fmaf(v4.z, sc.z, sh.z); v4.w = fmaf(v4.w, sc.w, sh.w);
            if (p.in_relu) {
                v4.x = fmaxf(v4.x, 0.f); v4.y = fmaxf(v4.y, 0.f); v4.z = fmaxf(v4.z, 0.f); v4.w = fmaxf(v4.w, 0.f);
            }
        }
        if (hr[it] < 0 || c >= p.Cin) v4 = make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4 *>(sX + cell * P + c4 * 4) = v4;
    }
    __syncthreads();
}

template <int NCH, int WV, int THREADS = 64 * WV>
__device__ __forceinline__ bool d3_stage_halo(const ConvParams &p, int x0, int y0, int z0, float *sX, int tid, int dbg)
{
    if (!d3_stage_ranks<NCH, WV, THREADS>(p, x0, y0, z0, sX, tid)) return false;
    d3_stage_rows<NCH, WV, THREADS>(p, sX, tid, dbg, 0);
    return true;
}

// C_out == 1 (the occupancy-logit layer, models/occupancy_initialization.py:171): a 32-column MFMA tile would spend 31/32
// of its work on padding.  Same halo staging; two lanes per cell split the 16-byte channel groups, the weights of the one
// output column come from LDS as broadcasts, plain fma chains, the BatchNorm summary of the tile by Chan merges in
// lane / wave order.
template <int NCH>
__global__ __launch_bounds__(256) void conv3d_tile_narrow_kernel(ConvParams p, int tiles_y, int tiles_z, int ntiles)
{
    constexpr int cin_pad = NCH * 8, P = cin_pad + 4, C4 = cin_pad / 4;
    constexpr int WV = kD3WvNarrow, kD3Halo = d3_halo(WV);
    static_assert(WV == 4, "the cell mapping below covers 128 cells with 256 threads");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sX = reinterpret_cast<float *>(smem);
    float *sWn = sX + kD3Halo * P;                            // [27][cin_pad] weights of the single column, zero padded
    float *sRed = sWn + 27 * cin_pad;                          // [4][3] wave summaries
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    if (tile >= ntiles) return;
    int x0, y0, z0;
    d3_tile_origin<WV>(tile, tiles_y, tiles_z, x0, y0, z0);
    for (int e = tid; e < 27 * cin_pad; e += 256) {
        const int k = e / cin_pad, c = e - k * cin_pad;
        sWn[e] = c < p.Cin ? p.w[((size_t)k * p.Cin + c) * p.Cout] : 0.0f;
    }
    if (!d3_stage_halo<NCH, WV>(p, x0, y0, z0, sX, tid, p.debug)) {  // (its barriers also publish sWn)
        if (p.bn_partial && tid == 0) bn_partial_store(p, tile, 0, 0.0f, 0.0f, 0.0f);
        return;
    }
    const int v = tid >> 1, part = tid & 1;  // cell (x = v / 32, y = (v / 8) % 4, z = v % 8), half of the channel groups
    const int cell0 = (((v >> 5) + 1) * kD3HY + ((v >> 3) & 3) + 1) * kD3HZ + (v & 7) + 1;
    const int row = d3_rank(sX, cell0, P, cin_pad);
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 27; ++k) {
        const int dx = k % 3 - 1, dy = (k / 3) % 3 - 1, dz = k / 9 - 1;
        const float *xk = sX + (cell0 + (dx * kD3HY + dy) * kD3HZ + dz) * P;
#pragma unroll
        for (int j = 0; j < C4 / 2; ++j) {
            const int c = (2 * j + part) * 4;
            const float4 a = *reinterpret_cast<const float4 *>(xk + c);
            const float4 w = *reinterpret_cast<const float4 *>(sWn + k * cin_pad + c);
            acc = fmaf(a.x, w.x, acc); acc = fmaf(a.y, w.y, acc); acc = fmaf(a.z, w.z, acc); acc = fmaf(a.w, w.w, acc);
        }
    }
    acc += __shfl_xor(acc, 1);
    float n = 0.0f, mean = 0.0f, m2 = 0.0f;
    if (part == 0 && row >= 0) {
        float *o = p.out + (size_t)row * p.ld_out;
        float val = acc + (p.bias ? p.bias[0] : 0.0f);
        if (p.accumulate) val += *o;
        if (p.relu) val = fmaxf(val, 0.0f);
        if (p.res) {
            float rv = p.res[(size_t)row * p.ld_res];
            if (p.res_scale) {
                rv = fmaf(rv, p.res_scale[0], p.res_shift[0]);
                if (p.res_relu) rv = fmaxf(rv, 0.0f);
            }
            val += rv;
        }
        *o = val;
        n = 1.0f; mean = val;
    }
    if (p.bn_partial) {  // (uniform)
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {  // lane-order tree: the lower lane of a pair is the left operand
            const float on = __shfl_xor(n, m), omean = __shfl_xor(mean, m), om2 = __shfl_xor(m2, m);
            const bool lower = (lane & m) == 0;
            float a_n = lower ? n : on, a_mean = lower ? mean : omean, a_m2 = lower ? m2 : om2;
            chan_merge(a_n, a_mean, a_m2, lower ? on : n, lower ? omean : mean, lower ? om2 : m2);
            n = a_n; mean = a_mean; m2 = a_m2;
        }
        if (lane == 0) { sRed[wave * 3] = n; sRed[wave * 3 + 1] = mean; sRed[wave * 3 + 2] = m2; }
        __syncthreads();
        if (tid == 0) {
            float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
            for (int w = 0; w < kWaves; ++w) chan_merge(a_n, a_mean, a_m2, sRed[w * 3], sRed[w * 3 + 1], sRed[w * 3 + 2]);
            bn_partial_store(p, tile, 0, a_n, a_mean, a_m2);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// 16-row form of the dense-grid kernel on v_mfma_f32_16x16x4_f32, for C_out <= 32 and C_in a multiple of 16.
// The 32-row tile kernel loses on the 94k-voxel initialisation set because its unit of work is too coarse (DESIGN.md 3b:
// 3.1 jobs of 11.5 us per SIMD = four rounds) and because a 32-column MFMA tile is half empty for the C_out = 16 layers.
// Here a workgroup owns 2 x 4 x 8 cells (halo 4 x 6 x 10 = 240 cells, 35 KB at C_in = 32: four workgroups per CU), a wave
// 16 of them (one x, two y, eight z) in CT accumulator tiles of 16 x 16; a job is a quarter of the 32-row kernel's.
//   A operand (lane l: row l & 15, k index q = l >> 4): x[cell(row)][16 kc + 4 q + s] for step s — one ds_read_b128 per chunk
//   B operand: W[k][16 kc + 4 q + s][16 t + (l & 15)], pre-packed so that a wave fetches (k, kc, t) with one 1 KB buffer load
//   C / D: column l & 15, rows 4 (l >> 4) + reg
// Summation order differs from the 32x32x2 kernels (four channels per MFMA): equal within fp32 round-off, not bit for bit.
// Own epilogue for this accumulator layout (conv_common.hpp: tile16_epilogue, shared with the 2D twin conv2d_tile16_kernel):
// bias, ReLU, residual (with its pending BatchNorm), row-wise LayerNorm, BatchNorm summaries.
// ---------------------------------------------------------------------------------------------
constexpr int kD16X = 2;                                     // tile x extent; y, z as the other tile kernels
constexpr int kD16Halo = (kD16X + 2) * kD3HY * kD3HZ;        // 240

// EP_TILE16_MIX (compile time): 1 (default) the loads an offset issues — CT weight quads two offsets ahead, the next offset's A
// quad from LDS — are spread among its 4 CT MFMAs (sched_group_barrier: one VMEM read per four MFMAs, then the LDS read) instead
// of issued in front of them behind a scheduling fence (0: the round-3..5 schedule; 2: no fence at all, the compiler's choice —
// measured equal to 0).  32 -> 32 + LayerNorm on the 94k-voxel set: 71.3 -> 64.5 us, 0.44 -> 0.49 of the fp32-MFMA peak; the cfg2
// step 1.595 -> 1.574 ms (tools/probes/t16_ab.sh, two interleaved rounds).  The same products in the same order: bit-identical.
#ifndef EP_TILE16_MIX
#define EP_TILE16_MIX 1
#endif
template <int CT, int KCH>
__global__ __launch_bounds__(256, 7) void conv3d_tile16_kernel(ConvParams p, int tiles_y, int tiles_z, int ntiles)
{
    // The input channels are walked in KCH PASSES of 16: the halo tile in LDS holds 16 channels at a time (240 cells x 80 B =
    // 19.2 KB whatever C_in is), so that seven to eight workgroups fit a CU and ALL tiles of the 94k-voxel set (1,594 non-empty,
    // 6.2 per CU) are resident at once — with the 32-channel halo (35 KB, four per CU) the layer ran in two batches and its
    // MFMA loop took 58 us for 36 us of MFMAs.  Accumulators carry over; one staging + barrier per pass.
    constexpr int cin_pad = 16, NCH = 2;
    constexpr int P = cin_pad + 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *sX = reinterpret_cast<float *>(smem);   // [kD16Halo][P]: 16 channels + the cell's row in the first pad word
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, q = lane >> 4;
    const int tile = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    if (tile >= ntiles) return;
    int x0, y0, z0;
    d3_tile_origin<kD16X>(tile, tiles_y, tiles_z, x0, y0, z0);
    float *sStat = sX;  // (after the loop) [4 waves][3][16 CT] summaries

    if (!d3_stage_ranks<NCH, kD16X, 256>(p, x0, y0, z0, sX, tid)) {
        if (p.bn_partial && tid < 16 * CT && tid < p.Cout) bn_partial_store(p, tile, tid, 0.0f, 0.0f, 0.0f);
        return;
    }
    // wave -> (x = wave / 2, y pair = wave % 2); MFMA row r -> cell (y = 2 (wave % 2) + r / 8, z = r % 8)
    const int wx = wave >> 1, wy = 2 * (wave & 1);
    const int cell_a = ((wx + 1) * kD3HY + wy + (l16 >> 3) + 1) * kD3HZ + (l16 & 7) + 1;   // this lane's A row
    int orow[4];   // output rows of this lane's accumulator rows 4 q + j
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r = 4 * q + j;
        orow[j] = d3_rank(sX, ((wx + 1) * kD3HY + wy + (r >> 3) + 1) * kD3HZ + (r & 7) + 1, P, cin_pad);
    }
    const bool work = __ballot(d3_rank(sX, cell_a, P, cin_pad) >= 0) != 0ull && !(p.debug & 1);   // (wave-uniform)

    f32x4 acc[CT];
#pragma unroll
    for (int t = 0; t < CT; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const float *xa = sX + (cell_a - (kD3HY + 1) * kD3HZ - 1) * P + 4 * q;
    constexpr unsigned kStepBytes = CT * 1024u, kOffBytes = KCH * kStepBytes;
    const __amdgpu_buffer_rsrc_t wrsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.wq), 0, (int)(27 * kOffBytes), 0x00020000);
    const unsigned wlane = (unsigned)lane * 16u;
    constexpr int kAheadB = 2;
    for (int pass = 0; pass < KCH; ++pass) {
        if (pass > 0) __syncthreads();  // every wave is done reading the previous pass's channels
        d3_stage_rows<NCH, kD16X, 256>(p, sX, tid, p.debug, 16 * pass);
        if (!work) continue;
        float4 bq[kAheadB + 1][CT];
        float4 aq[2];
        auto load_b = [&](int k, float4(&dst)[CT]) {
#pragma unroll
            for (int t = 0; t < CT; ++t) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(wrsrc, wlane + (unsigned)t * 1024u,
                                                                      (unsigned)((p.debug & 2) ? 0 : k) * kOffBytes + (unsigned)pass * kStepBytes, 0);
                dst[t] = make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
            }
        };
        auto load_a = [&](int k) {
            const int dx = k % 3, dy = (k / 3) % 3, dz = k / 9;
            return *reinterpret_cast<const float4 *>(xa + ((dx * kD3HY + dy) * kD3HZ + dz) * P);
        };
#pragma unroll
        for (int k = 0; k < kAheadB; ++k) load_b(k, bq[k]);
        aq[0] = load_a(0);
#pragma unroll
        for (int k = 0; k < 27; ++k) {
            if (k + kAheadB < 27) load_b(k + kAheadB, bq[(k + kAheadB) % (kAheadB + 1)]);
            if (k + 1 < 27) aq[(k + 1) & 1] = load_a(k + 1);
#if EP_TILE16_MIX == 0
            __builtin_amdgcn_sched_barrier(0);
#endif
            const float4 av = aq[k & 1];
            const float4(&bk)[CT] = bq[k % (kAheadB + 1)];
            // the CT accumulators alternate: a 16x16x4 MFMA issues every 32 cycles but returns after 40
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, bk[t].x, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, bk[t].y, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, bk[t].z, acc[t], 0, 0, 0);
#pragma unroll
            for (int t = 0; t < CT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, bk[t].w, acc[t], 0, 0, 0);
#if EP_TILE16_MIX == 1      // (probe builds: this offset's loads spread among its MFMAs instead of in front of them)
#pragma unroll
            for (int sg = 0; sg < CT; ++sg) {
                __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
#endif
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    __syncthreads();  // every wave is done with the halo: the summaries' scratch overlays it

    tile16_epilogue<CT>(p, acc, orow, sStat, tile);
}

size_t conv3d_narrow_lds(int nch)
{
    return ((size_t)d3_halo(kD3WvNarrow) * (nch * 8 + 4) + (size_t)27 * nch * 8 + 16) * sizeof(float);
}

template <int CT, int KCH>
int launch_conv3d_tile16(const ConvParams &p, hipStream_t st)
{
    int ty, tz;
    const int ntiles = d3_tiles_kind(p, kD3Tile16, &ty, &tz);
    const size_t lds = max((size_t)kD16Halo * (16 + 4) * sizeof(float), (size_t)kWaves * 3 * 16 * CT * sizeof(float));
    if (lds > 64 * 1024) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv3d_tile16_kernel<CT, KCH>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (attr != hipSuccess) return EPRECON_ERR_HIP_BASE - (int)attr;
    }
    ConvParams q = p;
    q.wq = p.wq16;
    hipLaunchKernelGGL((conv3d_tile16_kernel<CT, KCH>), dim3((unsigned)ntiles), dim3(256), lds, st, q, ty, tz, ntiles);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}

template <int NCH>
int launch_conv3d_narrow(const ConvParams &p, hipStream_t st)
{
    int ty, tz;
    const int ntiles = d3_tiles_kind(p, kD3Narrow, &ty, &tz);
    const size_t lds = conv3d_narrow_lds(NCH);
    if (lds > 64 * 1024) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void *>(&conv3d_tile_narrow_kernel<NCH>),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
        if (attr != hipSuccess) return EPRECON_ERR_HIP_BASE - (int)attr;
    }
    hipLaunchKernelGGL((conv3d_tile_narrow_kernel<NCH>), dim3((unsigned)ntiles), dim3(256), lds, st, p, ty, tz, ntiles);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
}  // namespace

namespace epconv {
int d3_tiles_kind(const ConvParams &p, int kind, int *ty, int *tz)
{
    const int wv = kind == kD3Tile16 ? kD16X : kD3WvNarrow;
    const int tx = (p.gx + wv - 1) / wv, tyy = (p.gy + kD3Y - 1) / kD3Y, tzz = (p.gz + kD3Z - 1) / kD3Z;
    if (ty) *ty = tyy;
    if (tz) *tz = tzz;
    return tx * tyy * tzz;
}

// eligibility of the dense-grid kernels (independent of the data: shapes, alignment, fusions)
// EPRECON_CONV_DENSE3D: 0 off; 1 the single-column kernel only; 2 (default) also the 16-row MFMA kernel.
// Measured on the 94k-voxel initialisation set (rocprofv3 kernel durations, profiles/r03/conv3d_*):
//   32 -> 1   24 us   against 82 us for the gather form            (single-column kernel)
//   16 -> 16  24 us   against 50 us,  32 -> 16  37 us against 76 us,  32 -> 32  71 us against 78 us     (16-row kernel)
// (a 32-row tile kernel on v_mfma_f32_32x32x2_f32 was built in round 3, bit-identical to the gather form and slower on this
// set — 97 us against 78 us: 3,185 wave jobs of 11.5 us on 1,024 SIMDs = four rounds, DESIGN.md 3b — and removed in round 4.)
inline int d3_level()
{
    const char *e = getenv("EPRECON_CONV_DENSE3D");   // (read per launch: tests flip it)
    return e ? atoi(e) : 2;
}

// which dense-grid kernel the SHAPE of this layer is for (everything but the weight packing: what the caller asks through
// eprecon_conv_dense3d_kind before it packs): level 1 the single-column kernel, level 2 also the 16-row MFMA kernel
// (C_out <= 32, C_in a multiple of 16); every other shape runs on the kernel map
int conv3d_shape_kind(const ConvParams &p)
{
    const int level = d3_level();
    if (level <= 0 || !p.vox_rank || p.K != 27 || p.gx <= 0 || p.gy <= 0 || p.gz <= 0) return kD3None;
    if (p.Cin % 4 != 0 || p.Cin > 64 || p.ld_x % 4 != 0 || (reinterpret_cast<uintptr_t>(p.x) & 15) != 0) return kD3None;
    if (p.in_scale && ((reinterpret_cast<uintptr_t>(p.in_scale) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.in_shift) & 15) != 0))
        return kD3None;
    if (p.Cout == 1 && !p.ln) return kD3Narrow;
    if (level < 2 || p.accumulate) return kD3None;
    if (p.Cout <= 32 && p.Cin % 16 == 0 && !(p.ln && p.bn_partial)) return kD3Tile16;
    return kD3None;
}

// ... and which one takes the launch: the 16-row kernel only with its packing (a missing one means "not this kernel", never
// an error)
int conv3d_kind(const ConvParams &p)
{
    const int kind = conv3d_shape_kind(p);
    if (kind == kD3Tile16 && (!p.wq16 || (reinterpret_cast<uintptr_t>(p.wq16) & 15) != 0)) return kD3None;
    return kind;
}

int launch_conv3d_16(const ConvParams &p, hipStream_t st)
{
    const int kch = p.Cin / 16;
    if (p.Cout <= 16) {
        switch (kch) {
            case 1: return launch_conv3d_tile16<1, 1>(p, st);
            case 2: return launch_conv3d_tile16<1, 2>(p, st);
            case 3: return launch_conv3d_tile16<1, 3>(p, st);
            default: return launch_conv3d_tile16<1, 4>(p, st);
        }
    }
    switch (kch) {
        case 1: return launch_conv3d_tile16<2, 1>(p, st);
        case 2: return launch_conv3d_tile16<2, 2>(p, st);
        case 3: return launch_conv3d_tile16<2, 3>(p, st);
        default: return launch_conv3d_tile16<2, 4>(p, st);
    }
}

int launch_conv3d_single_column(const ConvParams &p, hipStream_t st)
{
    switch ((p.Cin + 7) / 8) {
        case 1: return launch_conv3d_narrow<1>(p, st);
        case 2: return launch_conv3d_narrow<2>(p, st);
        case 3: return launch_conv3d_narrow<3>(p, st);
        case 4: return launch_conv3d_narrow<4>(p, st);
        case 5: return launch_conv3d_narrow<5>(p, st);
        case 6: return launch_conv3d_narrow<6>(p, st);
        case 7: return launch_conv3d_narrow<7>(p, st);
        default: return launch_conv3d_narrow<8>(p, st);
    }
}

}  // namespace epconv
