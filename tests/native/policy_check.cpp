// CPU check of smallpt's launch policy (csrc/spt_policy.h, what smallpt.hip
// launches render_kernel by): the launch shapes, the priority words, the
// heavy-tile tiers and the packed split / nheavy words of DESIGN.md §3's
// windows at 256 CUs and a 1920-pixel-wide frame -- every kernel result is
// bit-exact whatever these are, so nothing else pins them -- the RT_SPT_TUNE
// parser, the tier clamps, and that every accessor the kernel reads a packed
// word through inverts its encoder over the fields' full ranges.
// Prints the number of checks, or the first failure.
#include <stdio.h>
#include "spt_policy.h"

using namespace sptpolicy;

static long g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        g_checks++;                                                  \
        if (!(cond)) {                                               \
            printf("FAIL line %d: %s\n", __LINE__, #cond);           \
            return 1;                                                \
        }                                                            \
    } while (0)

constexpr int CUS = 256, W = 1920;
static const int g_order[1] = {0};     // (any non-null order: heavy_tiers only tests it)

static Shape wide_shape(int gstride, const char *tune = nullptr, int nlist = 0)
{
    Shape g = launch_shape(CUS, true, W, 0, 1080, gstride, nlist, spt_tune_parse(tune));
    g.order = g_order;
    return g;
}

int main()
{
    // ---- full-scan shapes: rows -> ntiles, wpb, nblocks, nslots, prio word
    const struct { int r1, ntiles, wpb, nblocks, nslots, prio; } scan[] = {
        {1080, 32400, 4, 8100, 8100, 0xC08040}, {540, 16320, 4, 4080, 4080, 0xC08040},
        {270, 8160, 16, 510, 2040, 0xE0C080},   {168, 5040, 4, 1260, 1260, 0xC08040},
        {135, 4080, 16, 255, 1020, 0xE0C080},
    };
    for (const auto &c : scan) {
        const Shape g = launch_shape(CUS, false, W, 0, c.r1, 1, 0, SptTune());
        CHECK(g.tiles_x == 240 && g.ntiles == c.ntiles && g.work == c.ntiles);
        CHECK(g.wpb == c.wpb);
        CHECK(g.nblocks == c.nblocks);
        CHECK(g.nslots == c.nslots);
        CHECK(prio_schedule(g) == c.prio);
        // no 8-wide tree: no tiers, with or without an order
        Shape o = g;
        o.order = g_order;
        for (const Shape *s : {&g, (const Shape *)&o}) {
            const Tiers t = heavy_tiers(*s, CUS);
            CHECK(t.n1 == 0 && t.n2 == 0 && t.cg == 0 && t.hw == 0);
            CHECK(pack_nheavy(t.n1, t.n2) == 0);
        }
    }

    // ---- 8-wide shapes, rows [0, 1080), with an order and tiers
    const struct { int gstride, ntiles, nblocks, nslots, n1, n2, cg, hw, stop; unsigned split, nheavy; } wide[] = {
        {1, 32400, 256, 8100, 0, 1024, 0, 0, 32, 0x20101000u, 1024u << 16},
        {2, 16320, 256, 4080, 1024, 0, 2, 0, 16, 0x10101005u, 1024u},
        {4, 8160, 256, 2040, 1024, 0, 4, 16, 16, 0x10101086u, 1024u},
        {8, 4080, 255, 1020, 512, 0, 8, 16, 16, 0x10101087u, 512u},
    };
    for (const auto &c : wide) {
        Shape g = wide_shape(c.gstride);
        CHECK(g.wpb == WIDE_WPB && g.ntiles == c.ntiles && g.nblocks == c.nblocks && g.nslots == c.nslots);
        const Tiers t = heavy_tiers(g, CUS);
        CHECK(t.n1 == c.n1);
        CHECK(t.n2 == c.n2);
        CHECK(t.cg == c.cg);
        CHECK(t.hw == c.hw);
        CHECK(t.stop == c.stop);
        CHECK((unsigned)split_word(g, t) == c.split);
        CHECK((unsigned)pack_nheavy(t.n1, t.n2) == c.nheavy);
        // the same window without an order, or with an unordered list (tiers = false)
        Shape plain = g, flat = g;
        plain.order = nullptr;
        flat.tiers = false;
        for (const Shape *s : {&plain, &flat}) {
            const Tiers u = heavy_tiers(*s, CUS);
            CHECK(u.n1 == 0 && u.n2 == 0 && u.cg == 0);
            CHECK((unsigned)split_word(*s, u) == 0x20101000u);
            CHECK(pack_nheavy(u.n1, u.n2) == 0);
        }
    }

    // ---- the RT_SPT_TUNE parser
    {
        const Shape g = wide_shape(1, "coop=512");
        const Tiers t = heavy_tiers(g, CUS);
        CHECK(t.n1 == 512 && t.n2 == 0 && t.cg == 8);
        CHECK((unsigned)split_word(g, t) == 0x10101007u);
    }
    {
        const SptTune t = spt_tune_parse("coop=1024,coop_g=4");
        CHECK(t.coop == 1024 && t.coop_g == 4 && t.coop_waves == -1 && t.routed == -1);
        const Shape g = wide_shape(1, "coop=1024,coop_g=4");
        const Tiers h = heavy_tiers(g, CUS);
        CHECK(h.n1 == 1024 && h.n2 == 0 && h.cg == 4 && h.hw == 0 && h.stop == 16);
        CHECK((unsigned)split_word(g, h) == 0x10101006u);
    }
    {
        const SptTune t = spt_tune_parse("walk=8/4/64");
        CHECK(t.budget == 8 && t.batch == 4 && t.stop == 64);
        const Shape g = wide_shape(1, "walk=8/4/64");
        const int s = split_word(g, heavy_tiers(g, CUS));
        CHECK(split_budget(s) == 8 && split_batch(s) == 4 && split_stop(s) == 64 && split_hs(s) == 0 && !split_coop(s));
    }
    {
        const SptTune t = spt_tune_parse("prio=10/20/30");
        CHECK(t.prio[0] == 10 && t.prio[1] == 20 && t.prio[2] == 30);
        const Shape g = launch_shape(CUS, false, W, 0, 1080, 1, 0, t);
        CHECK(prio_schedule(g) == (10 | 20 << 8 | 30 << 16));
    }
    {
        CHECK(spt_tune_parse("wpb=16").wpb == 16 && spt_tune_parse("wpb=4").wpb == 4 && spt_tune_parse("wpb=7").wpb == 4);
        const Shape g = launch_shape(CUS, false, W, 0, 1080, 1, 0, spt_tune_parse("wpb=16"));
        CHECK(g.wpb == 16 && g.nblocks == 2025 && g.nslots == 8100 && prio_schedule(g) == 0xE0C080);
    }
    {
        CHECK(spt_tune_parse("blocks=7").blocks == 7);
        const Shape g = wide_shape(1, "blocks=7");
        CHECK(g.nblocks == 7 && g.nslots == 8100);
        CHECK(heavy_tiers(g, CUS).n2 == 28);            // routed tiles: 4 x blocks
        CHECK(launch_shape(CUS, false, W, 0, 1080, 1, 0, spt_tune_parse("blocks=7")).nblocks == 8100);
    }
    for (const char *s : {"bogus=3", "coop", "", (const char *)nullptr, ",,", "coop_gg=4,=5"}) {
        const SptTune t = spt_tune_parse(s), d;
        CHECK(t.coop == d.coop && t.coop_g == d.coop_g && t.coop_waves == d.coop_waves && t.routed == d.routed);
        CHECK(t.budget == 16 && t.batch == 16 && t.stop == -1);
        CHECK(t.prio[0] == -1 && t.prio[1] == -1 && t.prio[2] == -1 && t.wpb == 0 && t.blocks == 0);
    }
    {
        const SptTune t = spt_tune_parse("coop_waves=99,routed=-4,bogus=1,coop=-2");
        CHECK(t.coop_waves == 16 && t.routed == 0 && t.coop == 0);
    }

    // ---- clamps: a list of 3 groups has 12 tiles
    {
        const Shape g = wide_shape(1, nullptr, 3);
        CHECK(g.work == 12 && g.nslots == 3 && g.nblocks == 1);
        const Tiers t = heavy_tiers(g, CUS);
        CHECK(t.n1 == 12 && t.n2 == 0);                 // 2 x CUs cooperative tiles asked for
        CHECK(t.n1 <= 4 * g.nslots);
        const Shape g2 = wide_shape(1, "coop=8,routed=100", 3);
        const Tiers t2 = heavy_tiers(g2, CUS);
        CHECK(t2.n1 == 8 && t2.n2 == 4);
        CHECK(t2.n1 + t2.n2 <= 4 * g2.nslots);
        const Shape g3 = wide_shape(1, "coop=0,routed=100", 3);
        CHECK(heavy_tiers(g3, CUS).n1 == 0 && heavy_tiers(g3, CUS).n2 == 12);
        // walk options outside their fields
        const Shape g4 = wide_shape(1, "walk=0/-3/900");
        const int s = split_word(g4, heavy_tiers(g4, CUS));
        CHECK(split_budget(s) == 1 && split_batch(s) == 0 && split_stop(s) == 64);
        const Shape g5 = wide_shape(1, "walk=999/99/7");
        const int s5 = split_word(g5, heavy_tiers(g5, CUS));
        CHECK(split_budget(s5) == 255 && split_batch(s5) == 64 && split_stop(s5) == 7);
    }

    // ---- every accessor inverts its encoder
    for (int hs = 0; hs <= 3; hs++)
        for (int coop = 0; coop <= 1; coop++)
            for (int hw = 0; hw <= 31; hw++) {
                const int s = pack_split(hs, coop != 0, hw, 16, 16, 32);
                CHECK(split_hs(s) == hs && split_coop(s) == (coop != 0) && split_hw(s) == hw);
                CHECK(split_budget(s) == 16 && split_batch(s) == 16 && split_stop(s) == 32);
            }
    for (int budget = 1; budget <= 255; budget++)
        for (int batch = 0; batch <= 64; batch++)
            for (int stop = 0; stop <= 64; stop += (stop < 4 || stop >= 60) ? 1 : 7) {
                const int s = pack_split(3, true, 31, budget, batch, stop);
                CHECK(split_budget(s) == budget && split_batch(s) == batch && split_stop(s) == stop);
                CHECK(split_hs(s) == 3 && split_coop(s) && split_hw(s) == 31);
            }
    for (int stop = 0; stop <= 64; stop++) {
        const int s = pack_split(0, false, 0, 1, 0, stop);
        CHECK(split_stop(s) == stop && split_budget(s) == 1 && split_batch(s) == 0 && !split_coop(s));
    }
    for (int n1 = 0; n1 <= 65535; n1 += (n1 < 64 || n1 >= 65500) ? 1 : 257)
        for (int n2 = 0; n2 <= 65535; n2 += (n2 < 64 || n2 >= 65500) ? 1 : 263) {
            const int w = pack_nheavy(n1, n2);
            CHECK(nheavy_n1(w) == n1 && nheavy_n2(w) == n2);
        }
    CHECK(nheavy_n1(pack_nheavy(70000, 70000)) == 65535 && nheavy_n2(pack_nheavy(70000, 70000)) == 65535);
    for (int a = 0; a <= 255; a += 5)
        for (int b = 0; b <= 255; b += 3) {
            const int w = pack_prio(a, b, 255 - a);
            CHECK(prio_bound(w, 0) == a && prio_bound(w, 1) == b && prio_bound(w, 2) == 255 - a);
        }
    for (int r = 0; r <= 1; r++)
        for (int m = 0; m <= 1; m++) {
            const int w = pack_sflags(r != 0, m != 0);
            CHECK(sflags_no_refr(w) == (r != 0) && sflags_cost_max(w) == (m != 0));
        }
    printf("%ld\n", g_checks);
    return 0;
}
