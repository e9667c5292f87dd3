// CPU check of the shadow-ray ring's arithmetic (csrc/spt_policy.h, sq_*):
// for every threshold T the ring allows, random push counts of 0..64 per step
// run against the flush rule exactly as render_kernel's loop applies it
// (flush passes while count >= T, then one push), beside a model queue of
// serial numbers.  The ring never holds more than its capacity, no live
// entry is overwritten, pops come out in push order, and every position --
// push, pop, an owner's distance from the head -- wraps into the ring.
// Also the sq tune key and the threshold's packed field.  Prints the number
// of checks; exits non-zero at the first failure.
#include <stdint.h>
#include <deque>
#include <vector>
#include "spt_policy.h"

using namespace sptpolicy;

static long nchecks = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        nchecks++;                                                       \
        if (!(c)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                    \
        }                                                                \
    } while (0)

static uint32_t rnd(uint32_t &s) { return s = s * 1664525u + 1013904223u; }

int main()
{
    CHECK(sq_max_threshold() >= 1 && sq_capacity(sq_max_threshold()) == SQ_RING);
    CHECK(SQ_DEFAULT >= 1 && SQ_DEFAULT <= sq_max_threshold());
    CHECK(SQ_RING < 256);                       // a position fits one byte of the kernel's pidx
    for (int T = 1; T <= sq_max_threshold(); T++) {
        CHECK(sq_threshold(T) == T);
        uint32_t seed = 12345u + (uint32_t)T;
        std::vector<long> ring(SQ_RING, -1);    // serial number held by each position (-1: free)
        std::deque<long> model;
        long serial = 0;
        int head = 0, count = 0;
        for (int step = 0; step < 4000; step++) {
            // the flush passes of one iteration
            while (sq_flush(count, T)) {
                const int m = sq_pop(count);
                CHECK(m >= 1 && m <= 64 && m <= count);
                for (int lane = 0; lane < m; lane++) {
                    const int e = sq_wrap(head + lane);
                    CHECK(e >= 0 && e < SQ_RING);
                    CHECK(ring[e] == model.front());            // FIFO: the oldest entries, in order
                    CHECK(sq_rel(e, head) == lane);             // the owner finds its bit
                    model.pop_front();
                    ring[e] = -1;
                }
                // an entry that stays is not among the popped ones
                if (count > m) CHECK(sq_rel(sq_wrap(head + m), head) == m);
                head = sq_wrap(head + m);
                count -= m;
                CHECK(head >= 0 && head < SQ_RING);
            }
            CHECK(count < T);
            // one push of 0..64 entries (every fourth step a full 64)
            const int n = step % 4 == 3 ? 64 : (int)(rnd(seed) >> 8) % 65;
            for (int rank = 0; rank < n; rank++) {
                const int pos = sq_push_pos(head, count, rank);
                CHECK(pos >= 0 && pos < SQ_RING);
                CHECK(ring[pos] == -1);                         // never over a live entry
                CHECK(sq_rel(pos, head) == count + rank);
                ring[pos] = serial;
                model.push_back(serial++);
            }
            count += n;
            CHECK(count <= sq_capacity(T) && count <= SQ_RING);
            CHECK((int)model.size() == count);
        }
        // the drain: passes until the ring is empty
        while (count > 0) {
            const int m = sq_pop(count);
            for (int lane = 0; lane < m; lane++) {
                const int e = sq_wrap(head + lane);
                CHECK(ring[e] == model.front());
                model.pop_front();
                ring[e] = -1;
            }
            head = sq_wrap(head + m);
            count -= m;
        }
        CHECK(model.empty());
    }
    // the tune key: clamped to [1, 64] by the parser, to the ring by the launch
    CHECK(spt_tune_parse(nullptr).sq == 0 && spt_tune_parse("wpb=4").sq == 0);
    CHECK(spt_tune_parse("sq=33").sq == 33 && spt_tune_parse("sq=0").sq == 1 && spt_tune_parse("sq=-5").sq == 1);
    CHECK(spt_tune_parse("sq=64").sq == 64 && spt_tune_parse("sq=1000").sq == 64);
    CHECK(spt_tune_parse("wpb=16,sq=17").sq == 17 && spt_tune_parse("wpb=16,sq=17").wpb == 16);
    CHECK(spt_tune_parse("sq").sq == 0 && spt_tune_parse("sqq=5").sq == 0);
    CHECK(sq_threshold(0) == SQ_DEFAULT && sq_threshold(64) == sq_max_threshold() && sq_threshold(1) == 1);
    for (int T = 0; T <= 64; T++)
        for (int r = 0; r < 2; r++)
            for (int m = 0; m < 2; m++) {
                const int w = pack_sflags(r != 0, m != 0, T);
                CHECK(sflags_sq(w) == T && sflags_no_refr(w) == (r != 0) && sflags_cost_max(w) == (m != 0));
            }
    CHECK(pack_sflags(true, true) == 5);
    printf("sq_ring_check ok: %ld\n", nchecks);
    return 0;
}
