// The count mailbox's ring: which of its slots is handed out, with which sequence number, and when a slot may be handed out
// again.  Host-only and free of HIP, so that it compiles on its own (tests/test_count_mailbox_ring.py runs it under the host
// sanitizers); count_mailbox.hip puts it on host-coherent pinned memory and exports it.
//
// A slot is kSlotWords int32: word 0 is the sequence word, words 1 .. 15 the payload.  acquire() hands out a free slot with the
// next sequence number of THAT slot (32 bits, never 0, rising; after 2^32 - 1 hand-outs of one slot it wraps past 0).  The
// publisher -- one GPU thread -- stores the payload and then the sequence word; the reader waits until the sequence word
// equals the number it was handed.  release() gives the slot back:
//   - published (the sequence word equals the number handed out) or never armed (no launch carries it): free at once;
//   - armed and not published yet (a reader that was dropped, a wait that ran into its cap): the slot DRAINS -- its publisher
//     may still store into it, and a publisher of the next hand-out on another stream could be overtaken by it -- and becomes
//     free when an acquire() finds its sequence word at the number it was waiting for.
// Thread-safe (one mutex: a handful of acquires per step).
#pragma once
#include <stdint.h>

#include <mutex>

namespace ep {

constexpr int kMailboxSlots = 64;   // a bit per slot in one word
constexpr int kSlotWords = 16;      // one 64-byte line: the sequence word and at most 15 counts (the largest publisher: 1 + B)

class MailboxRing {
public:
    // words: kMailboxSlots * kSlotWords int32, zeroed, that outlive the ring
    explicit MailboxRing(volatile int32_t *words) : words_(words) {}

    // -> the slot (0 .. 63) and its sequence number, or -1 when every slot is handed out or draining
    int acquire(uint32_t *seq_out)
    {
        std::lock_guard<std::mutex> lock(mu_);
        reap();
        if (!free_) return -1;
        // the slot after the last one handed out, so that every slot is used in turn
        const uint64_t rot = cursor_ ? (free_ >> cursor_) | (free_ << (kMailboxSlots - cursor_)) : free_;
        const int s = (__builtin_ctzll(rot) + cursor_) % kMailboxSlots;
        cursor_ = (s + 1) % kMailboxSlots;
        free_ &= ~(1ull << s);
        if (++seq_[s] == 0) seq_[s] = 1;
        *seq_out = seq_[s];
        return s;
    }

    // armed: a launch that publishes into the slot has been queued.  false for a slot that is not handed out, or not with `seq`.
    bool release(int s, uint32_t seq, bool armed)
    {
        std::lock_guard<std::mutex> lock(mu_);
        if (s < 0 || s >= kMailboxSlots || ((free_ | draining_) >> s & 1) || seq_[s] != seq) return false;
        if (!armed || seq_word(s) == seq) free_ |= 1ull << s;
        else draining_ |= 1ull << s;
        return true;
    }

    // has the publisher of this hand-out stored its sequence word?  (acquire load: the payload may be read behind it)
    bool published(int s, uint32_t seq) const { return seq_word(s) == seq; }

    // slots an acquire() could hand out right now
    int free_slots()
    {
        std::lock_guard<std::mutex> lock(mu_);
        reap();
        return __builtin_popcountll(free_);
    }

private:
    // draining slots whose publisher has stored by now are free again (mu_ held)
    void reap()
    {
        for (uint64_t d = draining_; d; d &= d - 1) {
            const int s = __builtin_ctzll(d);
            if (seq_word(s) == seq_[s]) {
                draining_ &= ~(1ull << s);
                free_ |= 1ull << s;
            }
        }
    }

    uint32_t seq_word(int s) const
    {
        return (uint32_t)__atomic_load_n(const_cast<const int32_t *>(words_) + (size_t)s * kSlotWords, __ATOMIC_ACQUIRE);
    }

    volatile int32_t *words_;
    std::mutex mu_;
    uint64_t free_ = ~0ull, draining_ = 0;
    int cursor_ = 0;
    uint32_t seq_[kMailboxSlots] = {};
};

}  // namespace ep
