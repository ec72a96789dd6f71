// Several device regions filled with a 32-bit pattern each in ONE launch (FillRegion, common.hpp): what the prologues of the
// stage calls reset — index volumes, counters, hash tables, the upper half of a self map.
// (The kernel sits in ep's anonymous namespace, as it did in kernel_map.hip: its symbol keeps its name.)
#include "common.hpp"

namespace ep {
namespace {
struct FillParams {
    uint32_t *base[kMaxFillRegions];            // the region's start rounded DOWN to 16 bytes
    unsigned long long end[kMaxFillRegions];    // exclusive prefix end, in 16-byte chunks
    unsigned lead[kMaxFillRegions];             // 32-bit words of the first chunk in front of the region
    unsigned long long words[kMaxFillRegions];  // the region's length in 32-bit words
    uint32_t value[kMaxFillRegions];
    int count;
};
// one thread per 16-byte chunk; chunks that straddle a region's first / last word write word by word
__global__ __launch_bounds__(256) void multi_fill_kernel(FillParams f)
{
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    unsigned long long begin = 0;
#pragma unroll 1
    for (int r = 0; r < f.count; ++r) {
        if (e < f.end[r]) {
            const uint32_t v = f.value[r];
            const unsigned long long w0 = (e - begin) * 4;                    // first word of the chunk, from the rounded-down base
            const unsigned long long lo = f.lead[r], hi = f.lead[r] + f.words[r];
            uint32_t *p = f.base[r] + w0;
            if (w0 >= lo && w0 + 4 <= hi) {
                *reinterpret_cast<uint4 *>(p) = make_uint4(v, v, v, v);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (w0 + k >= lo && w0 + k < hi) p[k] = v;
            }
            return;
        }
        begin = f.end[r];
    }
}
}  // namespace

int multi_fill(const FillRegion *regions, int count, hipStream_t st)
{
    if (count < 0 || count > kMaxFillRegions) return EPRECON_ERR_ARG;
    FillParams f;
    f.count = 0;
    unsigned long long total = 0;
    for (int r = 0; r < count; ++r) {
        if (regions[r].bytes == 0) continue;
        const uintptr_t a = reinterpret_cast<uintptr_t>(regions[r].p);
        if (!regions[r].p || (a & 3) || (regions[r].bytes & 3)) return EPRECON_ERR_ARG;
        const unsigned lead = (unsigned)((a & 15) / 4);
        const unsigned long long words = regions[r].bytes / 4;
        total += (lead + words + 3) / 4;
        f.base[f.count] = reinterpret_cast<uint32_t *>(a & ~(uintptr_t)15);
        f.lead[f.count] = lead;
        f.words[f.count] = words;
        f.end[f.count] = total;
        f.value[f.count] = regions[r].value;
        ++f.count;
    }
    if (total == 0) return EPRECON_OK;
    hipLaunchKernelGGL(multi_fill_kernel, dim3((unsigned)ceil_div((int64_t)total, 256)), dim3(256), 0, st, f);
    EP_LAUNCH_CHECK();
    return EPRECON_OK;
}
}  // namespace ep
