// CPU check of the pixel-list kernel's claim arithmetic (csrc/spt_pixels.h:
// pix_cursor, pix_claim_entry, pix_claim_advance, pix_claim_step).  Every wave
// of a (waves per block, blocks) grid runs claim steps with random need masks
// -- the empty and the full mask among them -- until it has been told
// "exhausted", and a few steps more.  Over all waves every entry of
// [0, nlist) is handed out exactly once; within a wave the entries grow
// strictly and lie in the wave's own chunks; the cursor keeps 0 <= pos <= 64
// and advances at most one chunk a step; exhaustion is permanent.  Also the
// edge of the index range: a list of INT32_MAX entries.  Prints the number of
// checks; exits non-zero at the first failure.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "spt_pixels.h"

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

// A need mask: empty, full, one lane, sparse, dense or uniform random.
static unsigned long long mask(uint32_t &s, int step)
{
    const unsigned long long r = ((unsigned long long)rnd(s) << 32) | rnd(s);
    switch (step % 7) {
    case 0: return 0ull;
    case 1: return ~0ull;
    case 2: return 1ull << (rnd(s) >> 26);
    case 3: return r & (((unsigned long long)rnd(s) << 32) | rnd(s)) & (((unsigned long long)rnd(s) << 32) | rnd(s));
    case 4: return r | (((unsigned long long)rnd(s) << 32) | rnd(s));
    default: return r;
    }
}

static int sweep(int nlist, int wpb, int nblocks, uint32_t seed)
{
    const int stride = wpb * nblocks;
    std::vector<int> times((size_t)nlist, 0);
    for (int v = 0; v < stride; v++) {
        PixCursor c = pix_cursor(v);
        int last = -1, after = 0;
        bool exhausted = false;
        for (int step = 0; after < 6; step++) {
            const unsigned long long need = mask(seed, step + v);
            int entry[64];
            for (int l = 0; l < 64; l++) entry[l] = -7;
            const PixCursor before = c;
            const bool out = pix_claim_step(c, need, stride, nlist, entry);
            const int count = __builtin_popcountll(need);
            CHECK(c.pos >= 0 && c.pos <= 64);
            CHECK(c.chunk == before.chunk || c.chunk == before.chunk + stride);     // at most one advance
            CHECK((long long)(c.chunk - v) / stride * 64 + c.pos ==
                  (long long)(before.chunk - v) / stride * 64 + before.pos + count);
            bool any_out = false;
            for (int l = 0; l < 64; l++) {
                if (!((need >> l) & 1)) {
                    CHECK(entry[l] == -7);                                          // a lane that did not ask
                    continue;
                }
                const int e = entry[l];
                if (e < 0) {
                    CHECK(e == -1);
                    any_out = true;
                    continue;
                }
                CHECK(!exhausted && !any_out);                                      // nothing after "exhausted"
                CHECK(e < nlist && e > last);                                       // in range, strictly growing
                CHECK((e / 64) % stride == v);                                      // one of the wave's chunks
                times[(size_t)e]++;
                last = e;
            }
            CHECK(out == any_out);
            exhausted = exhausted || out;
            if (exhausted) after++;
        }
    }
    for (int e = 0; e < nlist; e++) CHECK(times[(size_t)e] == 1);
    return 0;
}

int main()
{
    const int sizes[] = {0, 1, 63, 64, 65, 128, 129, 4097};
    const int shapes[][2] = {{1, 1}, {4, 1}, {4, 3}, {16, 1}, {16, 2}, {4, 17}, {4, 2048}};
    uint32_t seed = 2024u;
    for (int nlist : sizes)
        for (const auto &sh : shapes)
            for (int rep = 0; rep < 4; rep++)
                if (sweep(nlist, sh[0], sh[1], seed += 77u)) return 1;
    // the chunk-synchronous pattern: every step the full mask
    {
        PixCursor c = pix_cursor(2);
        int entry[64];
        for (int step = 0; step < 5; step++) {
            CHECK(!pix_claim_step(c, ~0ull, 8, 64 * 8 * 5, entry));
            for (int l = 0; l < 64; l++) CHECK(entry[l] == (2 + 8 * step) * 64 + l);
            CHECK(c.pos == 64 && c.chunk == 2 + 8 * step);
        }
        CHECK(pix_claim_step(c, ~0ull, 8, 64 * 8 * 5, entry) && entry[0] == -1 && entry[63] == -1);
    }
    // the edge of the index range: INT32_MAX entries, the wave that owns the last chunk
    {
        const int nlist = INT32_MAX, stride = 8192;
        const int last_chunk = (int)(((long long)nlist + 63) / 64 - 1);
        PixCursor c = pix_cursor(last_chunk);
        CHECK(pix_claim_entry(c, 0, stride, nlist) == last_chunk * 64);
        CHECK(pix_claim_entry(c, 62, stride, nlist) == INT32_MAX - 1);
        CHECK(pix_claim_entry(c, 63, stride, nlist) == -1);                         // entry INT32_MAX itself
        c = pix_claim_advance(c, 64, stride);
        CHECK(c.chunk == last_chunk && c.pos == 64);
        CHECK(pix_claim_entry(c, 0, stride, nlist) == -1 && pix_claim_entry(c, 63, stride, nlist) == -1);
        c = pix_claim_advance(c, 64, stride);
        CHECK(c.chunk == last_chunk + stride && c.pos == 64);
        CHECK(pix_claim_entry(c, 5, stride, nlist) == -1);
        PixCursor d = pix_cursor(last_chunk - stride);                              // its last chunk but one
        d = pix_claim_advance(d, 60, stride);
        CHECK(pix_claim_entry(d, 3, stride, nlist) == (last_chunk - stride) * 64 + 63);
        CHECK(pix_claim_entry(d, 4, stride, nlist) == last_chunk * 64);
    }
    printf("pixel_claim_check ok: %ld\n", nchecks);
    return 0;
}
