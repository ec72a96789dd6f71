// The library's identity and its gather timing hook: one event pair around the gather launch of whichever variant ran last
// (eprecon_profile_enable; the variants bracket their launch with ep::profile_bracket_begin / _end, common.hpp).
#include "common.hpp"

namespace {
struct ProfileState {
    bool on = false, recorded = false, one_shot = false;
    hipEvent_t start = nullptr, stop = nullptr;
    const char *kernel = "";
} g_prof;
}  // namespace

namespace ep {
int profile_bracket_begin(hipStream_t st)
{
    if (g_prof.on && g_prof.start) EP_HIP_CHECK(hipEventRecord(g_prof.start, st));
    return EPRECON_OK;
}
int profile_bracket_end(hipStream_t st, const char *kernel)
{
    if (g_prof.on && g_prof.start) {
        EP_HIP_CHECK(hipEventRecord(g_prof.stop, st));
        g_prof.recorded = true;
        g_prof.kernel = kernel;
        if (g_prof.one_shot) g_prof.on = false;
    }
    return EPRECON_OK;
}
}  // namespace ep

extern "C" {

int eprecon_abi_version(void) { return EPRECON_ABI_VERSION; }
const char *eprecon_build_arch(void) { return "gfx950"; }

int eprecon_profile_enable(int on)
{
    if (on && !g_prof.start) {
        EP_HIP_CHECK(hipEventCreate(&g_prof.start));
        EP_HIP_CHECK(hipEventCreate(&g_prof.stop));
    }
    g_prof.on = on != 0;
    g_prof.one_shot = on == 2;
    if (on != 0) g_prof.recorded = false;  // disabling keeps the last recorded pair readable
    return EPRECON_OK;
}

float eprecon_profile_gather_ms(void)
{
    if (!g_prof.recorded) return -1.0f;
    if (hipEventSynchronize(g_prof.stop) != hipSuccess) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, g_prof.start, g_prof.stop) != hipSuccess) return -1.0f;
    return ms;
}

const char *eprecon_profile_gather_kernel(void) { return g_prof.kernel; }

}  // extern "C"
