// The count mailbox: a handful of int32 counts go from the kernel thread that writes them to the host through host-coherent
// pinned memory, with no copy launch, no event and nothing queued on the stream.
//
//   host    eprecon_mailbox_acquire -> a slot: the payload's device-visible address, its host address, a sequence number
//   device  the ONE thread that writes the final count to device memory also calls ep::mailbox_publish (common.hpp): plain
//           stores of the payload, a system-scope fence, a system-scope release store of the sequence word
//   host    eprecon_mailbox_wait spins (pause, then yield, with a cap) until the sequence word equals the number handed out,
//           then reads the payload behind an acquire load; eprecon_mailbox_release returns the slot
//
// The GPU never waits for the host and never reads the mailbox; only the host waits, and only up to its cap.  The ring logic
// (which slot, which sequence number, when a slot may be reused) is count_mailbox_ring.hpp, host-only.
#include <sched.h>

#include <chrono>
#include <mutex>

#include "common.hpp"
#include "count_mailbox_ring.hpp"

namespace {
using namespace ep;

// EPRECON_COUNT_MAILBOX=0: every count read takes the copy path, as before the mailbox.  Read ONCE, when the library is loaded.
const bool g_switch_on = !switch_off("EPRECON_COUNT_MAILBOX");

struct Mailbox {
    int32_t *host = nullptr, *dev = nullptr;
    MailboxRing *ring = nullptr;
    int rc = EPRECON_OK;
};

// one ring per process, allocated at the first acquire (never freed: kernels of a dying process may still publish)
Mailbox &mailbox()
{
    static Mailbox mb;
    static std::once_flag once;
    std::call_once(once, [] {
        const size_t bytes = sizeof(int32_t) * kMailboxSlots * kSlotWords;
        void *h = nullptr, *d = nullptr;
        hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocCoherent | hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
        if (e != hipSuccess) {
            mb.rc = EPRECON_ERR_HIP_BASE - (int)e;
            return;
        }
        volatile int32_t *w = static_cast<volatile int32_t *>(h);
        for (int i = 0; i < kMailboxSlots * kSlotWords; ++i) w[i] = 0;
        mb.host = static_cast<int32_t *>(h);
        mb.dev = static_cast<int32_t *>(d);
        mb.ring = new MailboxRing(w);
    });
    return mb;
}

}  // namespace

extern "C" {

int eprecon_count_mailbox(void) { return g_switch_on ? 1 : 0; }

int eprecon_mailbox_acquire(int words, eprecon_mailbox_slot *out)
{
    if (!out || words <= 0) return EPRECON_ERR_ARG;
    *out = eprecon_mailbox_slot{};
    out->index = -1;
    if (!g_switch_on || words > EPRECON_MAILBOX_WORDS) return EPRECON_EMPTY;
    Mailbox &mb = mailbox();
    if (mb.rc != EPRECON_OK) return mb.rc;
    uint32_t seq = 0;
    const int s = mb.ring->acquire(&seq);
    if (s < 0) return EPRECON_EMPTY;
    out->payload_dev = mb.dev + (size_t)s * kSlotWords + 1;
    out->payload_host = mb.host + (size_t)s * kSlotWords + 1;
    out->seq = seq;
    out->index = s;
    out->words = words;
    return EPRECON_OK;
}

int eprecon_mailbox_wait(const eprecon_mailbox_slot *slot, int64_t timeout_us, int32_t *out)
{
    if (!slot || !out || slot->index < 0 || slot->index >= kMailboxSlots || slot->words <= 0 ||
        slot->words > EPRECON_MAILBOX_WORDS || timeout_us < 0)
        return EPRECON_ERR_ARG;
    Mailbox &mb = mailbox();
    if (mb.rc != EPRECON_OK) return mb.rc;
    using clock = std::chrono::steady_clock;
    const clock::time_point deadline = clock::now() + std::chrono::microseconds(timeout_us);
    // a count is usually there already, or a few microseconds away: pause first; then give the core away between looks.  The
    // clock is read every 64 looks while pausing and at every look while yielding: the spin never outlasts its cap by more.
    for (uint32_t spins = 0; !mb.ring->published(slot->index, slot->seq); ++spins) {
        if (spins < 4096) {
            __builtin_ia32_pause();
            if ((spins & 63) != 63) continue;
        } else {
            sched_yield();
        }
        if (clock::now() >= deadline) {
            if (mb.ring->published(slot->index, slot->seq)) break;
            return EPRECON_ERR_TIMEOUT;
        }
    }
    // (published() is an acquire load: the payload stores in front of the publisher's release store are visible here)
    const volatile int32_t *p = slot->payload_host;
    for (int i = 0; i < slot->words; ++i) out[i] = p[i];
    return EPRECON_OK;
}

int eprecon_mailbox_release(const eprecon_mailbox_slot *slot)
{
    if (!slot || slot->index < 0) return EPRECON_ERR_ARG;
    Mailbox &mb = mailbox();
    if (mb.rc != EPRECON_OK) return mb.rc;
    return mb.ring->release(slot->index, slot->seq, slot->armed != 0) ? EPRECON_OK : EPRECON_ERR_ARG;
}

int eprecon_mailbox_free_slots(void)
{
    Mailbox &mb = mailbox();
    return mb.rc != EPRECON_OK ? mb.rc : mb.ring->free_slots();
}

}  // extern "C"
