// CPU check of the sample plan's index arithmetic (csrc/spt_plan.h: plan_tiles*,
// plan_x, plan_y, plan_inside, plan_pixel, plan_slot, plan_key, plan_take_*,
// plan_scratch_*).  Over frames of 1 x 1, 7 x 9, 8 x 8, 9 x 8, 37 x 19 and
// 1920 x 1080, walking tiles and lanes as the kernels' waves do: every pixel
// is visited exactly once, by a lane inside the frame; the keys ascend and
// are budget_list's ((y >> 3) * tiles_x + (x >> 3)) * 64 + (y & 7) * 8 +
// (x & 7); the pixel index is y * w + x and the slot (h - y - 1) * w + x; a
// lane outside the frame is outside on its own coordinates.  Then the edge of
// the index range (w = INT32_MAX), the integer part of the decision, and the
// scratch layout.  Prints the number of checks; exits non-zero at the first
// failure.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "spt_plan.h"

static long nchecks = 0;
#define CHECK(c)                                                         \
    do {                                                                 \
        nchecks++;                                                       \
        if (!(c)) {                                                      \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);        \
            return 1;                                                    \
        }                                                                \
    } while (0)

static int sweep(int w, int h)
{
    const int tx = plan_tiles_x(w), ty = plan_tiles_y(h), ntiles = plan_tiles(w, h);
    CHECK(tx == (w + 7) / 8 && ty == (h + 7) / 8 && ntiles == tx * ty);
    CHECK((long long)ntiles * 64 >= (long long)w * h && ntiles <= w * h);
    std::vector<unsigned char> seen_pixel((size_t)w * h, 0), seen_slot((size_t)w * h, 0);
    long long last_key = -1, inside_count = 0;
    for (int tile = 0; tile < ntiles; tile++) {
        for (int lane = 0; lane < 64; lane++) {
            const unsigned x = plan_x(tile, lane, w), y = plan_y(tile, lane, w);
            const long long key = plan_key(tile, lane);
            CHECK(key > last_key);
            last_key = key;
            CHECK(x / 8 == (unsigned)(tile % tx) && y / 8 == (unsigned)(tile / tx));
            CHECK((int)(y & 7) == (lane >> 3) && (int)(x & 7) == (lane & 7));
            CHECK(key == ((long long)(y >> 3) * tx + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7));
            const bool inside = plan_inside(x, y, w, h);
            CHECK(inside == (x < (unsigned)w && y < (unsigned)h));
            if (!inside) continue;                                  // never listed: the kernels zero its take
            inside_count++;
            const int p = plan_pixel(x, y, w), s = plan_slot(x, y, w, h);
            CHECK(p >= 0 && p < w * h && s >= 0 && s < w * h);
            CHECK((long long)p == (long long)y * w + x);
            CHECK((long long)s == ((long long)h - y - 1) * w + x);
            CHECK(!seen_pixel[(size_t)p] && !seen_slot[(size_t)s]);
            seen_pixel[(size_t)p] = seen_slot[(size_t)s] = 1;
        }
    }
    CHECK(inside_count == (long long)w * h);
    for (size_t i = 0; i < seen_pixel.size(); i++) CHECK(seen_pixel[i] == 1 && seen_slot[i] == 1);
    return 0;
}

int main()
{
    const int sizes[][2] = {{1, 1}, {7, 9}, {8, 8}, {9, 8}, {37, 19}, {1920, 1080}};
    for (const auto &s : sizes)
        if (sweep(s[0], s[1])) return 1;
    // the edge of the index range: one row of INT32_MAX pixels, and one column
    {
        const int w = INT32_MAX, h = 1;
        const int ntiles = plan_tiles(w, h);
        CHECK(ntiles == 268435456 && plan_tiles_y(h) == 1);
        const int last = ntiles - 1;
        CHECK(plan_x(last, 0, w) == 2147483640u && plan_y(last, 0, w) == 0u);
        CHECK(plan_inside(plan_x(last, 6, w), 0u, w, h) && plan_pixel(plan_x(last, 6, w), 0u, w) == INT32_MAX - 1);
        CHECK(plan_slot(plan_x(last, 6, w), 0u, w, h) == INT32_MAX - 1);
        CHECK(!plan_inside(plan_x(last, 7, w), 0u, w, h));          // x == w, past an int's range
        CHECK(!plan_inside(plan_x(last, 8, w), plan_y(last, 8, w), w, h));      // the tile's second row
        CHECK(plan_key(last, 63) == (long long)ntiles * 64 - 1);
        CHECK(plan_tiles(1, INT32_MAX) == 268435456);
        CHECK(plan_y(268435455, 48, 1) == 2147483646u && plan_inside(0u, 2147483646u, 1, INT32_MAX));
        CHECK(plan_slot(0u, 2147483646u, 1, INT32_MAX) == 0 && plan_pixel(0u, 2147483646u, 1) == INT32_MAX - 1);
        CHECK(!plan_inside(0u, plan_y(268435455, 56, 1), 1, INT32_MAX));
    }
    // the decision's integer part
    {
        CHECK(plan_take_bootstrap(0, 8) == 8 && plan_take_bootstrap(7, 8) == 1 && plan_take_bootstrap(0, INT32_MAX) == INT32_MAX);
        CHECK(plan_take_bootstrap(-5, 8) == 13 && plan_take_bootstrap(INT32_MIN, INT32_MAX) == INT32_MAX);
        for (int n = 1; n <= 20; n++)
            for (int step = 1; step <= 9; step++)
                for (int max = n - 2; max <= n + 12; max++) {
                    const int t = plan_take_step(n, true, step, max);
                    CHECK(plan_take_step(n, false, step, max) == 0);
                    CHECK(t == (n < max ? (step < max - n ? step : max - n) : 0));
                    CHECK(t >= 0 && (t == 0 || n + t <= max));
                }
        CHECK(plan_take_step(1, true, INT32_MAX, INT32_MAX) == INT32_MAX - 1);
        CHECK(plan_take_step(INT32_MAX, true, 1, INT32_MAX) == 0);
    }
    // the scratch layout: parts in order, aligned, inside the size
    {
        alignas(16) static unsigned char buf[4096];
        for (int ntiles : {1, 2, 3, 15, 200}) {
            const size_t bytes = plan_scratch_bytes(ntiles);
            CHECK(bytes % 16 == 0 && bytes <= sizeof buf);
            unsigned char *head = (unsigned char *)plan_scratch_head(buf), *sums = (unsigned char *)plan_scratch_sums(buf);
            unsigned char *counts = (unsigned char *)plan_scratch_counts(buf, ntiles);
            CHECK(head == buf && sums == buf + 16 && counts == sums + 8 * (size_t)ntiles);
            CHECK(counts + 4 * (size_t)ntiles <= buf + bytes);
        }
    }
    printf("plan_index_check ok: %ld\n", nchecks);
    return 0;
}
