// probe: what does bn_finalize_affine_kernel (csrc/norm.hip) cost as a function of the number of summary rows nblk, with the
// summaries stored row-major, partial[nblk][3][C] (one float of each 64-byte segment per workgroup: 3 nblk segments through one
// CU), against channel-major, partial[3][C][ld] (three contiguous runs of nblk floats, all of a thread's rows loaded before its
// first merge)?  The model in DESIGN.md 7l: ~4.3 us floor + segments at ~1 / clk / CU + ~1.5 us per extra memory round trip.
//
//   hipcc --offload-arch=gfx950 -O3 -o tools/probes/bn_finalize_layout tools/probes/bn_finalize_layout.hip
//   tools/probes/bn_finalize_layout [out.txt]
//
// Both kernels merge thread t's rows t, t + 256, ... in order, then the xor butterfly, then the four waves in order: the probe
// also checks that their (scale, shift) are bit-identical on the same summaries.  Times: HIP events around 200 back-to-back
// launches of one shape (per-launch mean), after 20 warm-up launches; run under rocprofv3 --kernel-trace --stats for the
// per-kernel durations.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#define CHECK(x)                                                                                      \
    do {                                                                                              \
        hipError_t e_ = (x);                                                                          \
        if (e_ != hipSuccess) {                                                                       \
            fprintf(stderr, "%s:%d %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_));         \
            exit(1);                                                                                  \
        }                                                                                             \
    } while (0)

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

__device__ __forceinline__ void finish(float a_n, float a_mean, float a_m2, int tid, float g_c, float b_c, float eps, int c,
                                       float *scale_out, float *shift_out)
{
    __shared__ float sN[4], sMean[4], sM2[4];
    const int lane = tid & 63;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const float on = __shfl_xor(a_n, m), om = __shfl_xor(a_mean, m), oq = __shfl_xor(a_m2, m);
        float ln = (lane & m) ? on : a_n, lm = (lane & m) ? om : a_mean, lq = (lane & m) ? oq : a_m2;
        chan_merge(ln, lm, lq, (lane & m) ? a_n : on, (lane & m) ? a_mean : om, (lane & m) ? a_m2 : oq);
        a_n = ln; a_mean = lm; a_m2 = lq;
    }
    if (lane == 0) { sN[tid >> 6] = a_n; sMean[tid >> 6] = a_mean; sM2[tid >> 6] = a_m2; }
    __syncthreads();
    if (tid == 0) {
        float n = sN[0], mean = sMean[0], m2 = sM2[0];
        for (int w = 1; w < 4; ++w) chan_merge(n, mean, m2, sN[w], sMean[w], sM2[w]);
        const float var = n > 0.0f ? m2 / n : 0.0f;
        const float sc = g_c / sqrtf(var + eps);
        scale_out[c] = sc;
        shift_out[c] = b_c - mean * sc;
    }
}

// row-major summaries: the finalize of the parent commit, four rows per loop trip
__global__ __launch_bounds__(256) void finalize_row_major(const float *partial, int nblk, int C, const float *gamma,
                                                          const float *beta, float eps, float *scale_out, float *shift_out)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    const float g_c = gamma[c], b_c = beta[c];
    float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
    for (int b = tid; b < nblk; b += 4 * 256) {
        float vn[4], vm[4], vq[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int bb = b + u * 256;
            const float *p = partial + (size_t)(bb < nblk ? bb : b) * 3 * C;
            vn[u] = bb < nblk ? p[c] : 0.0f;
            vm[u] = p[C + c];
            vq[u] = p[2 * C + c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) chan_merge(a_n, a_mean, a_m2, vn[u], vm[u], vq[u]);
    }
    finish(a_n, a_mean, a_m2, tid, g_c, b_c, eps, c, scale_out, shift_out);
}

// channel-major summaries: three contiguous runs per channel, up to 16 rows per thread loaded before the first merge
constexpr int kRows = 16;
__global__ __launch_bounds__(256) void finalize_channel_major(const float *partial, int nblk, int64_t ld, int C, const float *gamma,
                                                              const float *beta, float eps, float *scale_out, float *shift_out)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    const float g_c = gamma[c], b_c = beta[c];
    const float *pn = partial + (size_t)c * ld, *pm = pn + (size_t)C * ld, *pq = pm + (size_t)C * ld;
    float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
    for (int b = tid; b < nblk; b += kRows * 256) {
        float vn[kRows], vm[kRows], vq[kRows];
#pragma unroll
        for (int u = 0; u < kRows; ++u) {
            const int bb = b + u * 256;
            const bool ok = bb < nblk;
            vn[u] = ok ? pn[bb] : 0.0f;
            vm[u] = ok ? pm[bb] : 0.0f;
            vq[u] = ok ? pq[bb] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < kRows; ++u) chan_merge(a_n, a_mean, a_m2, vn[u], vm[u], vq[u]);
    }
    finish(a_n, a_mean, a_m2, tid, g_c, b_c, eps, c, scale_out, shift_out);
}

// ... the same with the rows per thread and trip a template argument NU (1, 2, 4, 8, 16), the smallest that covers nblk in one
// trip: short lists do not pay for 16 row groups of empty loads and merges.  (A uniform `u < nu` guard on each row group instead
// was measured too: it splits the loads into guarded groups, and at nblk = 2,700 cost 1 us more than NU = 16.)
template <int NU>
__global__ __launch_bounds__(256) void finalize_channel_major_nu(const float *partial, int nblk, int64_t ld, int C, const float *gamma,
                                                                 const float *beta, float eps, float *scale_out, float *shift_out)
{
    const int c = blockIdx.x, tid = threadIdx.x;
    const float g_c = gamma[c], b_c = beta[c];
    const float *pn = partial + (size_t)c * ld, *pm = pn + (size_t)C * ld, *pq = pm + (size_t)C * ld;
    float a_n = 0.0f, a_mean = 0.0f, a_m2 = 0.0f;
    for (int b = tid; b < nblk; b += NU * 256) {
        float vn[NU], vm[NU], vq[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int bb = b + u * 256;
            const bool ok = bb < nblk;
            vn[u] = ok ? pn[bb] : 0.0f;
            vm[u] = ok ? pm[bb] : 0.0f;
            vq[u] = ok ? pq[bb] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) chan_merge(a_n, a_mean, a_m2, vn[u], vm[u], vq[u]);
    }
    finish(a_n, a_mean, a_m2, tid, g_c, b_c, eps, c, scale_out, shift_out);
}

static void launch_channel_major_nu(hipStream_t st, const float *partial, int nblk, int C, const float *g, const float *b,
                                    float *o)
{
    const int need = (nblk + 255) / 256;
#define L(NU) hipLaunchKernelGGL(finalize_channel_major_nu<NU>, dim3(C), dim3(256), 0, st, partial, nblk, (int64_t)nblk, C, g, b, \
                                 1e-5f, o, o + C)
    if (need <= 1) L(1);
    else if (need <= 2) L(2);
    else if (need <= 4) L(4);
    else if (need <= 8) L(8);
    else L(16);
#undef L
}

int main(int argc, char **argv)
{
    FILE *out = argc > 1 ? fopen(argv[1], "w") : stdout;
    if (!out) return 1;
    const int nblks[] = {85, 338, 675, 1350, 2700, 5400};
    const int Cs[] = {12, 24, 40, 80};
    const int kWarm = 20, kIters = 200;
    hipStream_t st;
    CHECK(hipStreamCreate(&st));
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    fprintf(out, "# bn_finalize_affine: row-major [nblk][3][C] vs channel-major [3][C][nblk] summaries, MI355X\n");
    fprintf(out, "# per-launch mean of %d back-to-back launches (HIP events), after %d warm-up launches\n", kIters, kWarm);
    fprintf(out, "%6s %4s %12s %12s %12s %8s %10s\n", "nblk", "C", "row_major_us", "chan16_us", "chan_nu_us", "ratio", "bit_equal");
    int bad = 0;
    for (int nblk : nblks)
        for (int C : Cs) {
            // summaries as a 128-row-block producer would leave them: counts 1..128, means in [-2, 2], M2 >= 0; some rows empty
            std::vector<float> rm((size_t)nblk * 3 * C), cm((size_t)3 * C * nblk), g(C), bt(C);
            unsigned s = 12345u + nblk * 7u + C;
            auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (s >> 8) * (1.0f / 16777216.0f); };
            for (int r = 0; r < nblk; ++r)
                for (int c = 0; c < C; ++c) {
                    const float n = (r % 37 == 5) ? 0.0f : (float)(1 + (int)(rnd() * 128.0f) % 128);
                    const float mean = n > 0.0f ? 4.0f * rnd() - 2.0f : 0.0f;
                    const float m2 = n > 0.0f ? n * rnd() : 0.0f;
                    const float v[3] = {n, mean, m2};
                    for (int q = 0; q < 3; ++q) {
                        rm[((size_t)r * 3 + q) * C + c] = v[q];
                        cm[((size_t)q * C + c) * nblk + r] = v[q];
                    }
                }
            for (int c = 0; c < C; ++c) { g[c] = 0.5f + rnd(); bt[c] = rnd() - 0.5f; }
            float *d_rm, *d_cm, *d_g, *d_b, *d_o1, *d_o2, *d_o3;
            CHECK(hipMalloc(&d_rm, rm.size() * 4));
            CHECK(hipMalloc(&d_cm, cm.size() * 4));
            CHECK(hipMalloc(&d_g, C * 4));
            CHECK(hipMalloc(&d_b, C * 4));
            CHECK(hipMalloc(&d_o1, 2 * C * 4));
            CHECK(hipMalloc(&d_o2, 2 * C * 4));
            CHECK(hipMalloc(&d_o3, 2 * C * 4));
            CHECK(hipMemcpy(d_rm, rm.data(), rm.size() * 4, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(d_cm, cm.data(), cm.size() * 4, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(d_g, g.data(), C * 4, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(d_b, bt.data(), C * 4, hipMemcpyHostToDevice));
            float ms[3];
            for (int k = 0; k < 3; ++k) {
                auto launch = [&]() {
                    if (k == 0)
                        hipLaunchKernelGGL(finalize_row_major, dim3(C), dim3(256), 0, st, d_rm, nblk, C, d_g, d_b, 1e-5f, d_o1, d_o1 + C);
                    else if (k == 1)
                        hipLaunchKernelGGL(finalize_channel_major, dim3(C), dim3(256), 0, st, d_cm, nblk, (int64_t)nblk, C, d_g, d_b,
                                           1e-5f, d_o2, d_o2 + C);
                    else
                        launch_channel_major_nu(st, d_cm, nblk, C, d_g, d_b, d_o3);
                };
                for (int i = 0; i < kWarm; ++i) launch();
                CHECK(hipGetLastError());
                CHECK(hipEventRecord(e0, st));
                for (int i = 0; i < kIters; ++i) launch();
                CHECK(hipEventRecord(e1, st));
                CHECK(hipEventSynchronize(e1));
                CHECK(hipEventElapsedTime(&ms[k], e0, e1));
            }
            std::vector<float> o1(2 * C), o2(2 * C), o3(2 * C);
            CHECK(hipMemcpy(o1.data(), d_o1, 2 * C * 4, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(o2.data(), d_o2, 2 * C * 4, hipMemcpyDeviceToHost));
            CHECK(hipMemcpy(o3.data(), d_o3, 2 * C * 4, hipMemcpyDeviceToHost));
            const bool eq = memcmp(o1.data(), o2.data(), 2 * C * 4) == 0 && memcmp(o1.data(), o3.data(), 2 * C * 4) == 0;
            bad += !eq;
            const float u0 = ms[0] * 1000.0f / kIters, u1 = ms[1] * 1000.0f / kIters, u2 = ms[2] * 1000.0f / kIters;
            fprintf(out, "%6d %4d %12.2f %12.2f %12.2f %8.2f %10s\n", nblk, C, u0, u1, u2, u0 / u2, eq ? "yes" : "NO");
            fflush(out);
            CHECK(hipFree(d_rm)); CHECK(hipFree(d_cm)); CHECK(hipFree(d_g)); CHECK(hipFree(d_b));
            CHECK(hipFree(d_o1)); CHECK(hipFree(d_o2)); CHECK(hipFree(d_o3));
        }
    fprintf(out, "# %s\n", bad ? "MISMATCH between the two layouts" : "all (scale, shift) bit-identical between the layouts");
    if (out != stdout) fclose(out);
    return bad ? 2 : 0;
}
