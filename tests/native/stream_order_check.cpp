// CPU check of csrc/spt_streams.h: the bookkeeping that orders one scene's
// launches across streams -- which work-counter entry a launch takes, which
// reader slot, and which events its stream waits for first -- against a
// model that tracks every launch.
//
// The model keeps what the device would do.  Every launch gets a number; a
// stream's "knows" set holds the launches that are complete before the
// stream's next operation runs (its own earlier ones, and whatever the
// events it waited for stood for).  An event, when recorded on a stream,
// stands for that stream's knows set.  The properties, checked at every step
// of random sequences on 1 to 12 streams (an event query of the caller's is
// answered at random: "complete" makes the event's launches known to every
// stream):
//   ring    an entry is handed to a launch only when the stream knows the
//           entry's previous uncaptured user; a captured entry is never
//           handed out again until release; -1 exactly when all are captured;
//           `wait` is set only when the previous user was another stream.
//   order   a write is queued into one of two buffers only when its stream
//           knows every launch that read that buffer since its previous
//           write, and waits for none while either buffer is free of readers
//           elsewhere; a reader launch runs only when its stream knows the
//           last write.
// Prints the number of steps checked; exits non-zero at the first failure.
#include <stdint.h>
#include <stdio.h>
#include <set>
#include <vector>
#include "spt_streams.h"

using namespace sptstreams;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n)
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (unsigned)((rng_state >> 11) % n);
}

typedef std::set<long> Set;
static void merge(Set &into, const Set &from) { into.insert(from.begin(), from.end()); }

#define FAIL(...) do { printf("FAILED: " __VA_ARGS__); printf("\n"); return 1; } while (0)

static long steps = 0;

static int ring_case(int nstreams, int pcapture, int nlaunch)
{
    RingBook r;
    char handles[16];                                 // a stream's handle is &handles[i]
    std::vector<Set> knows(nstreams);
    Set ev[RingBook::N];                              // what entry k's event stands for
    long user[RingBook::N];                           // the entry's last uncaptured launch (-1: none)
    bool held[RingBook::N] = {};                      // by a captured graph
    for (long &u : user) u = -1;
    long id = 0;
    int expect = 0;
    for (int n = 0; n < nlaunch; n++, steps++) {
        if (rnd(997) == 0) {                          // spt_scene_release_captures
            r.captured = 0;
            for (bool &h : held) h = false;
        }
        const int s = (int)rnd(nstreams);
        const bool capturing = (int)rnd(100) < pcapture;
        int nheld = 0;
        for (bool h : held) nheld += h;
        RingTake t = ring_take(r, &handles[s], capturing);
        if ((t.entry < 0) != (nheld == RingBook::N)) FAIL("ring: entry %d with %d entries held", t.entry, nheld);
        if (t.entry < 0) continue;
        // work_entry passes over an entry whose event is not complete yet (here: at random)
        for (int tries = 0;; tries++) {
            while (held[expect % RingBook::N]) expect++;  // round robin over the entries not held
            if (t.entry != expect % RingBook::N) FAIL("ring: entry %d, round robin gives %d", t.entry, expect % RingBook::N);
            expect = t.entry + 1;
            if (!t.wait || tries == RingBook::N - 1 || rnd(3)) break;
            t = ring_take(r, &handles[s], capturing);
            if (t.entry < 0) FAIL("ring: no entry after one was passed over");
        }
        if (held[t.entry]) FAIL("ring: entry %d is held by a captured graph", t.entry);
        if (capturing) {
            if (t.wait) FAIL("ring: a capturing launch waits");
            held[t.entry] = true;
            continue;                                 // (a graph: it runs when replayed, not here)
        }
        const bool other = user[t.entry] >= 0 && !knows[s].count(user[t.entry]);
        if (t.wait) merge(knows[s], ev[t.entry]);
        if (user[t.entry] >= 0 && !knows[s].count(user[t.entry]))
            FAIL("ring: entry %d zeroed on stream %d under launch %ld", t.entry, s, user[t.entry]);
        if (t.wait && !other && nstreams == 1) FAIL("ring: a wait on the only stream");
        knows[s].insert(id);                          // the launch, then its event
        ev[t.entry] = knows[s];
        user[t.entry] = id++;
        ring_recorded(r, t.entry, &handles[s]);
    }
    return 0;
}

static int order_case(int nstreams, int pwrite, int nops)
{
    Readers r[2];
    int cur = 0;
    char handles[16];
    std::vector<Set> knows(nstreams);
    Set rd_ev[2][Readers::K], up_ev;
    Set readers_since[2];                             // launches that read buffer b since its last write
    long last_write = -1, id = 0;                     // (the last write went into buffer cur)
    int switched = 0;
    {                                                 // the first upload (state 2 follows one)
        const int s = (int)rnd(nstreams);
        if (write_waits(r[cur], &handles[s]) != 0) FAIL("order: waits before anything read");
        knows[s].insert(id);
        up_ev = knows[s];
        last_write = id++;
        written(r[cur], &handles[s]);
    }
    for (int n = 0; n < nops; n++, steps++) {
        const int s = (int)rnd(nstreams);
        if ((int)rnd(100) < pwrite) {
            // the caller's event queries: a complete event's launches are complete for every stream
            unsigned busy[2];
            for (int b = 0; b < 2; b++) {
                busy[b] = write_waits(r[b], &handles[s]);
                for (int i = 0; i < Readers::K; i++)
                    if (((busy[b] >> i) & 1u) && rnd(2)) {
                        busy[b] &= ~(1u << i);
                        for (Set &k : knows) merge(k, rd_ev[b][i]);
                    }
            }
            const int t = write_target(cur, busy[cur], busy[cur ^ 1]);
            if (t != cur && (busy[cur] == 0 || busy[t] != 0)) FAIL("order: switched to a buffer that is being read");
            if (t == cur && busy[cur] != 0 && busy[cur ^ 1] == 0) FAIL("order: waits though the other buffer is free");
            switched += t != cur;
            cur = t;
            for (int i = 0; i < Readers::K; i++)
                if ((busy[cur] >> i) & 1u) merge(knows[s], rd_ev[cur][i]);
            for (long x : readers_since[cur])
                if (!knows[s].count(x)) FAIL("order: write on stream %d under reader %ld", s, x);
            knows[s].insert(id);
            up_ev = knows[s];
            last_write = id++;
            readers_since[cur].clear();
            written(r[cur], &handles[s]);
        } else {
            const ReaderSlot q = reader_slot(r[cur], &handles[s]);
            if (q.slot < 0 || q.slot >= Readers::K) FAIL("order: slot %d", q.slot);
            if (q.wait_slot) merge(knows[s], rd_ev[cur][q.slot]);
            if (q.wait_write) merge(knows[s], up_ev);
            if (!knows[s].count(last_write)) FAIL("order: reader on stream %d before write %ld", s, last_write);
            if (nstreams == 1 && (q.wait_slot || q.wait_write)) FAIL("order: a wait on the only stream");
            knows[s].insert(id);
            rd_ev[cur][q.slot] = knows[s];            // recorded after the launch
            readers_since[cur].insert(id++);
        }
    }
    if (nstreams == 1 && switched) FAIL("order: one stream switched buffers");
    return 0;
}

int main()
{
    for (int nstreams = 1; nstreams <= 12; nstreams++)
        for (int rep = 0; rep < 6; rep++) {
            const int pcap[] = {0, 0, 3, 10, 40, 100};
            if (ring_case(nstreams, pcap[rep], 3000)) return 1;
            const int pwr[] = {1, 5, 20, 50, 1, 5};
            if (order_case(nstreams, pwr[rep], 3000)) return 1;
        }
    // the issue's two sequences, spelled out
    {
        RingBook r;
        char a, b;
        const RingTake ta = ring_take(r, &a, false);
        ring_recorded(r, ta.entry, &a);
        for (int i = 0; i < 63; i++) {
            const RingTake t = ring_take(r, &b, false);
            if (t.wait || t.entry == ta.entry) FAIL("ring: launch %d of stream B", i);
            ring_recorded(r, t.entry, &b);
        }
        const RingTake t = ring_take(r, &b, false);   // the 64th comes back to A's entry
        if (t.entry != ta.entry || !t.wait) FAIL("ring: the wrap does not wait for stream A");
        ring_recorded(r, t.entry, &b);
        if (ring_take(r, &b, false).wait) FAIL("ring: stream B waits for itself");
    }
    {
        Readers r;
        char a, b;
        written(r, &a);
        const ReaderSlot qa = reader_slot(r, &a);
        if (qa.wait_slot || qa.wait_write) FAIL("order: the writer's own stream waits");
        if (write_waits(r, &b) != 1u << qa.slot) FAIL("order: the rewrite on B does not wait for A's reader");
        if (write_target(0, 1u << qa.slot, 0) != 1) FAIL("order: the rewrite does not take the free buffer");
        written(r, &b);
        if (!reader_slot(r, &a).wait_write) FAIL("order: A reads without waiting for B's write");
        if (reader_slot(r, &a).wait_write) FAIL("order: A waits for the same write twice");
    }
    printf("stream_order_check ok: %ld\n", steps);
    return 0;
}
