// CPU check of smallpt's kernel variants and LDS layout (csrc/spt_layout.h,
// what render_kernel addresses its dynamic LDS by and launch() sizes it by):
// over every variant, block shape and a sweep of scene sizes, the regions of
// the carve are pairwise disjoint, aligned and inside block_lds_bytes; a
// wave's lanes reach 64 banks in every slot; the figures DESIGN.md §3
// documents, restated here as literals; the occupancy the block shapes are
// built for; and that no launch asks for more LDS than a CU has.
// Prints the number of checks, or the first failure.
#include <stdio.h>
#include <vector>
#include "spt_bvh.h"
#include "spt_layout.h"

using namespace sptlayout;

static long g_checks = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        g_checks++;                                                  \
        if (!(cond)) {                                               \
            printf("FAIL line %d: %s\n", __LINE__, #cond);           \
            return 1;                                                \
        }                                                            \
    } while (0)

struct Region { size_t begin, end; };

// Pairwise disjoint and inside [0, total).
static bool disjoint_inside(const std::vector<Region> &r, size_t total)
{
    for (size_t i = 0; i < r.size(); i++) {
        if (r[i].begin > r[i].end || r[i].end > total) return false;
        for (size_t j = 0; j < i; j++)
            if (r[i].begin < r[j].end && r[j].begin < r[i].end) return false;
    }
    return true;
}

// The regions of one block, by the expressions render_kernel addresses them with.
static int check_block(const Variant &v, const SceneSizes &s, int wpb)
{
    const size_t total = block_lds_bytes(v, s, wpb);
    std::vector<Region> r;
    if (v.lds()) {
        r.push_back({0, (size_t)scene_bytes(s.n, s.nlights)});
        CHECK(scene_bytes(s.n, s.nlights) == 16 * scene_records(s.n, s.nlights));
    }
    if (v.park()) {
        const size_t head = park_offset(v, s.n, s.nlights);
        CHECK(head % 16 == 0 && (v.lds() || head == 0));
        r.push_back({head, head + PARK_HEAD_BYTES});
        const int nslots = v.dq() ? DQ_SLOTS : PARK_SLOTS;
        for (int w = 0; w < wpb; w++) {
            const size_t dw0 = (head + PARK_HEAD_BYTES) / 4 + (size_t)w * wave_dwords(v.dq());    // park_ptr() of lane 0
            r.push_back({4 * dw0, 4 * (dw0 + 64 * nslots)});
            for (int slot = 0; slot < nslots; slot++) {
                unsigned long long banks = 0;
                for (int lane = 0; lane < 64; lane++) banks |= 1ull << ((dw0 + lane + 64 * slot) % 64);
                CHECK(banks == ~0ull);
            }
            if (v.dq()) {
                const size_t ring = dw0 + RING_BASE_DW;                                            // ring_ptr()
                r.push_back({4 * ring, 4 * (ring + RING_FIELDS * RING_FIELD_DW)});
                const size_t last = ring + (RING_FIELDS - 1) * RING_FIELD_DW + (sptpolicy::SQ_RING - 1);
                CHECK(last < dw0 + wave_dwords(true) && 4 * last + 4 <= total);
            }
        }
        CHECK(SLOT_COL + 3 <= PARK_SLOTS && SLOT_RAD >= PARK_SLOTS && SLOT_RAD + 3 <= SLOT_PEND &&
              SLOT_PEND + 3 <= DQ_SLOTS);
    }
    if (v.gstore()) {
        for (int g = 0; g < wpb / 4; g++) {
            const size_t base = (size_t)g * GS_BYTES;                                              // GS_BASE()
            r.push_back({base + GS_COL_OFF, base + GS_COL_OFF + 8 * 96 * 4});
            r.push_back({base + GS_SEED_OFF, base + GS_SEED_OFF + 8 * 64 * 4});
            r.push_back({base + GS_PX_OFF, base + GS_PX_OFF + 8 * 32 * 4});
            r.push_back({base + GS_COUNT_OFF, base + GS_COUNT_OFF + 4});
            CHECK(base % 16 == 0);
        }
    }
    if (v.geo == GEO_WIDE) {
        const size_t stacks = wide_stack_offset(s.wnodes, v.count());
        r.push_back({0, stacks});
        CHECK(stacks % 16 == 0);
        for (int w = 0; w < wpb; w++) {
            const size_t b = stacks + (size_t)w * WIDE_LEVEL_DW * (s.wdepth - 1) * 4;               // wstk
            r.push_back({b, b + (size_t)WIDE_LEVEL_DW * (s.wdepth - 1) * 4});
        }
        CHECK(total == sptbvh::wide_lds_bytes(s.wnodes, s.wdepth, wpb, v.count()));
        CHECK(total == (size_t)(v.count() ? 144 : 112) * s.wnodes + (size_t)wpb * 256 * (s.wdepth > 1 ? s.wdepth - 1 : 1));
    }
    CHECK(disjoint_inside(r, total));
    // a 16-wave block is alone on its CU: by its LDS, or (8-wide) by its registers
    if (wpb == 16 && v.geo != GEO_WIDE && total <= 163840) CHECK(163840 / total == 1);
    return 0;
}

int main()
{
    // ---- the predicates, against their definitions written out once more
    for (int geo = 0; geo < 4; geo++)
        for (int dl = 0; dl < 2; dl++)
            for (int dual = 0; dual < 2; dual++)
                for (int cmode = 0; cmode < 3; cmode++)
                    for (int cg : {0, 2, 4, 8}) {
                        const Variant v{geo, dl != 0, dual != 0, cmode, cg};
                        const bool full = geo == 0 || geo == 1;
                        CHECK(v.lds() == (geo == 0) && v.park() == full && v.persist() == (geo == 3));
                        CHECK(v.sched() == !full && v.gstore() == (geo == 2));
                        CHECK(v.dq() == (dual && cmode == 0 && full));
                        CHECK(v.count() == (cmode == 1) && v.rays() == (cmode == 2));
                        CHECK(v.min_waves() == (geo == 2 ? (cmode ? 4 : 6) : geo == 3 ? 4 : (dual && !cmode) ? 7 : 1));
                        const Variant t = variant_of(geo, dl, dual, cmode == 1, cmode == 2, cg);
                        CHECK(t.geo == geo && t.dl == v.dl && t.dual == v.dual && t.cmode == cmode && t.cg == cg);
                    }

    // ---- the documented figures
    CHECK(4 * wave_dwords(false) == 768 && 4 * wave_dwords(true) == 5440);
    CHECK(GS_BYTES == 6160 && GS_SEED_OFF == 3072 && GS_PX_OFF == 5120 && GS_COUNT_OFF == 6144);
    CHECK(wide_node_bytes(false) == 112 && wide_node_bytes(true) == 144);
    CHECK(PARK_HEAD_BYTES == 64 && CU_LDS_BYTES == 163840 && MAX_LDS_BYTES == 98304);
    CHECK(ONE_PER_CU_LDS_BYTES == 82944 && 2 * ONE_PER_CU_LDS_BYTES > CU_LDS_BYTES);
    CHECK(sptbvh::WIDE_LDS_MAX == 147456);
    const SceneSizes cornell{9, 1, 0, 0};
    const Variant deferred{GEO_LDS, false, true, CNT_NONE, 0}, counted{GEO_LDS, false, true, CNT_FULL, 0};
    CHECK(block_lds_bytes(deferred, cornell, 4) == 22304);
    CHECK(block_lds_bytes(deferred, cornell, 16) == 87584);
    CHECK(block_lds_bytes(counted, cornell, 16) == 82944);
    CHECK(163840 / block_lds_bytes(deferred, cornell, 4) >= 7);         // the two-query kernel's occupancy

    // ---- every variant x block shape x scene size: the regions
    const int wide_depth = 5, wide_most = (147456 - 16 * 256 * (wide_depth - 1)) / 144;   // the largest counted tree
    CHECK(sptbvh::wide_lds_bytes(wide_most, wide_depth, 16) <= sptbvh::WIDE_LDS_MAX &&
          sptbvh::wide_lds_bytes(wide_most + 1, wide_depth, 16) > sptbvh::WIDE_LDS_MAX);
    const int wide_sizes[3][2] = {{1, 1}, {539, 5}, {wide_most, wide_depth}};
    for (int geo = 0; geo < 4; geo++)
        for (int dl = 0; dl < 2; dl++)
            for (int dual = 0; dual < 2; dual++)
                for (int cmode = 0; cmode < 3; cmode++)
                    for (int cg : {0, 2, 4, 8})
                        for (int wpb : {4, 16})
                            for (int n : {1, 9, 255, 1597, 1598, 2047})
                                for (int nlights : {0, 1, 3})
                                    for (int wi = 0; wi < 3; wi++) {
                                        const int *ws = wide_sizes[wi];
                                        if (geo != GEO_WIDE && (cg != 0 || wi != 0)) continue;
                                        Variant v{geo, dl != 0, dual != 0, cmode, cg};
                                        const SceneSizes s{n, nlights, geo == GEO_WIDE ? ws[0] : 0, geo == GEO_WIDE ? ws[1] : 0};
                                        // as the kernel is written (the LDS family even where a CU cannot hold it)
                                        if (check_block(v, s, wpb)) return 1;
                                        // as the host launches: the two-query form for path tracing over the
                                        // full scan only, and the family launch_geo leaves
                                        if (dual && (dl || !v.park())) continue;
                                        v.geo = launch_geo(v, s, wpb);
                                        CHECK(v.geo == geo || (geo == GEO_LDS && v.geo == GEO_GLOBAL));
                                        if (check_block(v, s, wpb)) return 1;
                                        CHECK(block_lds_bytes(v, s, wpb) <= 163840);
                                    }

    // ---- the LDS family where its block no longer fits: from 1,598 spheres
    // with one light, sixteen waves with rings
    CHECK(launch_geo(deferred, SceneSizes{1597, 1, 0, 0}, 16) == GEO_LDS);
    CHECK(block_lds_bytes(deferred, SceneSizes{1597, 1, 0, 0}, 16) == 163808);
    CHECK(launch_geo(deferred, SceneSizes{1598, 1, 0, 0}, 16) == GEO_GLOBAL);
    CHECK(block_lds_bytes(deferred, SceneSizes{1598, 1, 0, 0}, 16) == 163856);
    CHECK(launch_geo(deferred, SceneSizes{2047, 1, 0, 0}, 4) == GEO_LDS);
    CHECK(launch_geo(counted, SceneSizes{2047, 1, 0, 0}, 16) == GEO_LDS);
    const Variant fallen{GEO_GLOBAL, false, true, CNT_NONE, 0};
    CHECK(block_lds_bytes(fallen, SceneSizes{1598, 1, 0, 0}, 16) == 64 + 16 * 5440);

    printf("layout checks: %ld\n", g_checks);
    return 0;
}
