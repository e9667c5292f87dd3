// spt_streams.h -- which stream must wait for which, when launches of one
// prepared scene are in flight on several streams (issued by one host thread
// at a time): the bookkeeping of spt_sched.h's work-counter ring and learnt
// order, as plain host code without a HIP call.  The caller owns one event per
// ring entry, one per reader slot and one per write; the functions here say
// which entry or slot a launch takes and which of those events its stream
// waits for first.  Streams are compared as opaque handles.
// Swept by tests/native/stream_order_check.cpp against a model that tracks
// every launch.
#ifndef SPT_STREAMS_H
#define SPT_STREAMS_H

#include <stdint.h>

namespace sptstreams {

// ---- the work-counter ring: an entry has one user at a time.
struct RingBook {
    static constexpr int N = 64;
    int next = 0;
    uint64_t captured = 0;            // held by a captured graph: never handed out
    uint64_t used = 0;                // an uncaptured launch recorded the entry's event
    const void *last[N] = {};         //   ... on this stream
};

struct RingTake {
    int entry;                        // -1: every entry is held by a captured graph
    bool wait;                        // the stream first waits for the entry's event (its last user was another stream)
};

// The next entry for a launch on `stream`.  A capturing launch keeps its
// entry for good and neither waits nor records.
inline RingTake ring_take(RingBook &r, const void *stream, bool capturing)
{
    for (int tries = 0; tries < RingBook::N; tries++) {
        const int k = r.next++ % RingBook::N;
        r.next %= RingBook::N;
        if ((r.captured >> k) & 1ull) continue;
        if (capturing) {
            r.captured |= 1ull << k;
            return {k, false};
        }
        return {k, ((r.used >> k) & 1ull) && r.last[k] != stream};
    }
    return {-1, false};
}

// After the uncaptured launch that uses entry k: its event was recorded on `stream`.
inline void ring_recorded(RingBook &r, int k, const void *stream)
{
    r.used |= 1ull << k;
    r.last[k] = stream;
}

// ---- a buffer written now and then (the learnt order) and read by launches
// on any stream: K reader slots, one event each, recorded after every launch
// of the slot's stream that reads the buffer.  A further stream takes over
// the slot of another (round robin) and first waits for that slot's event,
// so the slot's event still stands for every launch it stood for.
struct Readers {
    static constexpr int K = 8;
    const void *stream[K] = {};
    unsigned live = 0;                // slot i's event stands for launches since the last write
    unsigned seen = 0;                // slot i's stream is ordered after the last write
    int victim = 0;
    const void *writer = nullptr;     // the stream of the last write
};

struct ReaderSlot {
    int slot;                         // the event to record after the launch
    bool wait_slot;                   // first wait for this slot's event (taken over from another stream)
    bool wait_write;                  // first wait for the last write's event (made on another stream)
};

inline ReaderSlot reader_slot(Readers &r, const void *stream)
{
    int k = -1;
    for (int i = 0; i < Readers::K; i++)
        if (((r.live >> i) & 1u) && r.stream[i] == stream) k = i;
    bool wait_slot = false;
    if (k < 0) {
        for (int i = 0; i < Readers::K && k < 0; i++)
            if (!((r.live >> i) & 1u)) k = i;
        if (k < 0) {
            k = r.victim;
            r.victim = (r.victim + 1) % Readers::K;
            wait_slot = true;
        }
        r.seen &= ~(1u << k);
    }
    r.stream[k] = stream;
    const bool wait_write = stream != r.writer && !((r.seen >> k) & 1u);
    r.live |= 1u << k;
    r.seen |= 1u << k;
    return {k, wait_slot, wait_write};
}

// Before a write on `stream`: the slots whose events it waits for first (bit
// i: slot i) -- every reader since the last write but the stream's own.
inline unsigned write_waits(const Readers &r, const void *stream)
{
    unsigned m = 0;
    for (int i = 0; i < Readers::K; i++)
        if (((r.live >> i) & 1u) && r.stream[i] != stream) m |= 1u << i;
    return m;
}

// The write was queued on `stream` (after write_waits' waits) and its event recorded.
inline void written(Readers &r, const void *stream)
{
    r.live = r.seen = 0;
    r.writer = stream;
}

// Two such buffers, one of them in use (cur): the one a write on a stream
// goes into, given for each the slots of write_waits whose events are not
// yet complete.  The current one if no launch elsewhere still reads it, or
// if the other is being read as well (the stream then waits for busy_cur).
inline int write_target(int cur, unsigned busy_cur, unsigned busy_other)
{
    return busy_cur == 0 || busy_other != 0 ? cur : cur ^ 1;
}

}  // namespace sptstreams

#endif
