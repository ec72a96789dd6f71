// Stand-alone driver of eprecon_amd/csrc/count_mailbox_ring.hpp (tests/test_count_mailbox_ring.py builds it under the host
// sanitizers): four threads acquire, publish (as the GPU thread would: payload, then the sequence word), release and abandon
// slots of one ring on plain host memory.  Checked: no slot is handed out twice at once, sequence numbers never repeat per
// slot and never are 0, an abandoned (armed, unpublished) slot is not handed out until its publisher has stored, and a full
// ring reports full.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>
#include <vector>

#include "count_mailbox_ring.hpp"

using ep::kMailboxSlots;
using ep::kSlotWords;

static int32_t g_words[kMailboxSlots * kSlotWords];
static std::atomic<int> g_owner[kMailboxSlots];       // 0: nobody, else the thread (1-based) that holds the slot
static std::atomic<uint32_t> g_last_seq[kMailboxSlots];
static std::atomic<int> g_failures{0};

#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            g_failures++;                                               \
        }                                                               \
    } while (0)

static void publish(int s, uint32_t seq, int32_t value)
{
    g_words[s * kSlotWords + 1] = value;
    __atomic_store_n(&g_words[s * kSlotWords], (int32_t)seq, __ATOMIC_RELEASE);
}

struct Late {
    int slot;
    uint32_t seq;
};

static void worker(ep::MailboxRing *ring, int me, int rounds)
{
    std::vector<Late> late;     // abandoned slots whose publisher has not stored yet
    unsigned rng = 12345u * me;
    for (int r = 0; r < rounds; ++r) {
        rng = rng * 1664525u + 1013904223u;
        uint32_t seq = 0;
        const int s = ring->acquire(&seq);
        if (s < 0) {            // full: finish the late publishers, which lets their slots drain
            for (const Late &l : late) {
                CHECK(g_owner[l.slot].load() == -me);
                g_owner[l.slot].store(0);
                publish(l.slot, l.seq, 7);
            }
            late.clear();
            std::this_thread::yield();
            continue;
        }
        CHECK(s < kMailboxSlots && seq != 0);
        int expected = 0;
        CHECK(g_owner[s].compare_exchange_strong(expected, me));      // handed out to nobody else, draining included
        const uint32_t before = g_last_seq[s].exchange(seq);
        CHECK(seq > before);                                           // rises per slot (no wrap within this run)
        switch ((rng >> 16) % 4) {
        case 0:     // never armed: free at once
            g_owner[s].store(0);
            CHECK(ring->release(s, seq, false));
            break;
        case 1:     // published, read, released
        case 2:
            publish(s, seq, (int32_t)seq);
            CHECK(ring->published(s, seq));
            CHECK(g_words[s * kSlotWords + 1] == (int32_t)seq);
            g_owner[s].store(0);
            CHECK(ring->release(s, seq, true));
            break;
        default:    // abandoned: armed, released before its publisher stores; the slot stays ours (-me) until it does
            g_owner[s].store(-me);
            CHECK(ring->release(s, seq, true));
            CHECK(!ring->release(s, seq, true));                       // (a second release of the same hand-out is refused)
            late.push_back({s, seq});
            break;
        }
    }
    for (const Late &l : late) {
        g_owner[l.slot].store(0);
        publish(l.slot, l.seq, 7);
    }
}

int main()
{
    ep::MailboxRing ring(g_words);
    // a full ring reports full, and hands out again what is released
    uint32_t seqs[kMailboxSlots], extra = 0;
    bool seen[kMailboxSlots] = {};
    for (int i = 0; i < kMailboxSlots; ++i) {
        const int s = ring.acquire(&seqs[i]);
        CHECK(s >= 0 && s < kMailboxSlots && !seen[s] && seqs[i] == 1);
        if (s >= 0) seen[s] = true;
    }
    CHECK(ring.acquire(&extra) == -1 && ring.free_slots() == 0);
    CHECK(ring.release(5, 1, true));            // armed, unpublished: drains
    CHECK(ring.acquire(&extra) == -1);
    publish(5, 1, 3);
    CHECK(ring.acquire(&extra) == 5 && extra == 2);
    CHECK(!ring.release(5, 1, true));           // the old hand-out's number does not release the new one
    CHECK(ring.release(5, 2, false));
    for (int s = 0; s < kMailboxSlots; ++s)
        if (s != 5) CHECK(ring.release(s, 1, false));
    CHECK(ring.free_slots() == kMailboxSlots);
    for (int s = 0; s < kMailboxSlots; ++s) g_last_seq[s].store(s == 5 ? 2 : 1);

    std::vector<std::thread> threads;
    for (int t = 1; t <= 4; ++t) threads.emplace_back(worker, &ring, t, 20000);
    for (std::thread &t : threads) t.join();
    uint32_t seq = 0;
    int got = 0;
    while (ring.acquire(&seq) >= 0) ++got;      // every late publisher has stored: every slot comes back
    CHECK(got == kMailboxSlots);
    if (g_failures.load()) return 1;
    puts("ring ok");
    return 0;
}
