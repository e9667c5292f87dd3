// spt_policy.h -- the launch policy of smallpt's render_kernel: the tuning
// knobs, the launch shape, the heavy-tile tiers and the four packed words the
// kernel receives (split, nheavy, sflags, prio_sched).  Arithmetic only, no
// HIP types: smallpt.hip launches by it, the kernel and the walks (spt_walk.h)
// read the words through the accessors below, and the CPU check
// tests/native/policy_check.cpp pins its defaults under g++.
#ifndef SPT_POLICY_H
#define SPT_POLICY_H

#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <string>

#ifdef __HIPCC__
#define SPT_HD __host__ __device__ __forceinline__
#else
#define SPT_HD
#endif

namespace sptpolicy {

// ---- the packed words: one encoder each, and the accessors the device uses
//
// split: hs in bits 0..1 (a tier-1 tile is 2^hs sub-items of 64 >> hs pixels),
// bit 2 = tier-1 tiles walk cooperatively, bits 3..7 = hw, the waves of a
// block that take tier-1 sub-items first (0: 4 << hs); wide_walk's options
// above them: trip budget per call (8..15), leaf batch threshold (16..23) and
// early stop (24..31), both in 1/64 of the call's lanes.
inline int pack_split(int hs, bool coop, int hw, int budget, int batch, int stop)
{
    return (int)((unsigned)hs | (coop ? 4u : 0u) | ((unsigned)hw << 3) | ((unsigned)budget << 8) |
                 ((unsigned)batch << 16) | ((unsigned)stop << 24));
}
SPT_HD constexpr int split_hs(int split) { return split & 3; }
SPT_HD constexpr bool split_coop(int split) { return split & 4; }
SPT_HD constexpr int split_hw(int split) { return (split >> 3) & 31; }
SPT_HD constexpr int split_budget(int split) { return (split >> 8) & 255; }
SPT_HD constexpr int split_batch(int split) { return (split >> 16) & 255; }
SPT_HD constexpr int split_stop(int split) { return (split >> 24) & 255; }

// nheavy: n1 tier-1 tiles in bits 0..15, n2 tier-2 (routed) tiles in 16..31.
inline int pack_nheavy(int n1, int n2)
{
    return (int)((unsigned)std::min(n1, 0xffff) | ((unsigned)std::min(n2, 0xffff) << 16));
}
SPT_HD constexpr int nheavy_n1(int nheavy) { return nheavy & 0xffff; }
SPT_HD constexpr int nheavy_n2(int nheavy) { return (nheavy >> 16) & 0xffff; }

// sflags: bit 0 = no sphere of the scene refracts, bit 2 = group costs are
// the group's longest tile (atomic max), not the sum, bits 8..14 = the flush
// threshold of the shadow-ray ring (the uncounted two-query kernel; else 0).
inline int pack_sflags(bool no_refr, bool cost_max, int sq = 0)
{
    return (no_refr ? 1 : 0) | (cost_max ? 4 : 0) | ((sq & 127) << 8);
}
SPT_HD constexpr bool sflags_no_refr(int sflags) { return sflags & 1; }
SPT_HD constexpr bool sflags_cost_max(int sflags) { return sflags & 4; }
SPT_HD constexpr int sflags_sq(int sflags) { return (sflags >> 8) & 127; }

// ---- the shadow-ray ring of the uncounted two-query kernel (render_kernel,
// DQ): per wave SQ_RING entries in LDS, a FIFO of `count` entries from `head`.
// A flush pass runs while count >= T and pops min(count, 64) entries, one per
// lane; a push follows only when count < T and adds at most one entry per
// lane, so the ring never holds more than T + 63 entries and T may be at most
// SQ_RING - 63.  Positions are in [0, SQ_RING); one conditional subtraction
// wraps a sum of two of them, or of a position and a count.
constexpr int SQ_RING = 112;
constexpr int SQ_DEFAULT = 49;
SPT_HD constexpr int sq_capacity(int T) { return T + 63; }
SPT_HD constexpr int sq_max_threshold() { return SQ_RING - 63; }
SPT_HD constexpr int sq_threshold(int T) { return T < 1 ? SQ_DEFAULT : (T > sq_max_threshold() ? sq_max_threshold() : T); }
SPT_HD constexpr int sq_wrap(int i) { return i >= SQ_RING ? i - SQ_RING : i; }
SPT_HD constexpr bool sq_flush(int count, int T) { return count >= T; }
SPT_HD constexpr int sq_pop(int count) { return count < 64 ? count : 64; }
// the ring position of the rank-th pushing lane's entry
SPT_HD constexpr int sq_push_pos(int head, int count, int rank) { return sq_wrap(sq_wrap(head + count) + rank); }
// an entry's distance from the head: it is among the m popped ones iff < m
SPT_HD constexpr int sq_rel(int pos, int head) { return pos - head < 0 ? pos - head + SQ_RING : pos - head; }

// The owners' step of a flush pass.  A lane holds up to two entries, oldest
// first, at the ring positions in pidx's bytes 0 and 1 (npend of them), of
// which the oldest npark belong to its parked sample.  The pass pops the m
// entries from head; unocc has the bit of every popped entry whose ray
// reached the light.  FIFO: the second entry resolves only if the first does
// (tests/native/owners_step_check.cpp: against the per-entry loop).
struct SqOwners {
    bool r0, r1;        // the oldest / the second entry is among the popped ones
    bool lit0, lit1;    //   ... and its ray reached the light
};
SPT_HD constexpr SqOwners sq_owners(int pidx, int npend, int head, int m, unsigned long long unocc)
{
    const int rel0 = sq_rel(pidx & 255, head), rel1 = sq_rel((pidx >> 8) & 255, head);
    const bool r0 = npend > 0 && rel0 < m, r1 = r0 && npend > 1 && rel1 < m;
    return SqOwners{r0, r1, r0 && ((unocc >> (rel0 & 63)) & 1ull) != 0, r1 && ((unocc >> (rel1 & 63)) & 1ull) != 0};
}
// the entries the lane drops from its list, how many of n dropped ones belong
// to the parked sample, and the list's positions after n are dropped
SPT_HD constexpr int sq_owners_resolved(const SqOwners &o) { return o.r1 ? 2 : (o.r0 ? 1 : 0); }
SPT_HD constexpr int sq_owners_parked(int n, int npark) { return n < npark ? n : npark; }
SPT_HD constexpr int sq_owners_shift(int pidx, int n) { return pidx >> (8 * n); }

// prio_sched: the three priority-level boundaries, 8 bits each, in 1/256 of
// the samples.
inline int pack_prio(int a, int b, int c) { return (a & 255) | ((b & 255) << 8) | ((c & 255) << 16); }
SPT_HD constexpr int prio_bound(int prio_sched, int level) { return (prio_sched >> (8 * level)) & 255; }

// ---- tuning knobs
//
// The launch policy's tuning knobs, in one place.  The defaults are the
// measured best; RT_SPT_TUNE="key=value,..." overrides any of
// them for an A/B run or a test (read at every launch, so a test may change
// it between frames).  Keys:
//   coop=N      cooperative (tier-1) tiles of an ordered 8-wide launch
//               (default: 2 x CUs at <= 5 waves of work per SIMD, 4 x CUs at
//               <= 10, else 0)
//   coop_g=G    lanes per pixel of those tiles, 8, 4 or 2 (default 8 at <= 5
//               waves of work per SIMD, 4 at <= 10, 2 at <= 20)
//   coop_waves=K waves of each block that fetch tier-1 sub-items first (16)
//   routed=N    tier-2 tiles routed one per SIMD (default 4 x blocks when
//               there is no cooperative tier, else 0)
//   walk=B/P/S  wide_walk: trip budget per call, leaf batch threshold and
//               early stop, both in 1/64 of the call's lanes (16/16/32; the
//               stop 16 in windows with a cooperative tier)
//   prio=A/B/C  priority-levelling boundaries in 1/256 of the samples
//               (64/128/192 for the 4-wave block shape, 128/192/224 for 16)
//   wpb=4|16    full-scan block shape (default: by waves of work per SIMD)
//   blocks=N    8-wide persistent grid size (default: one block per CU)
//   sq=T        flush threshold of the shadow-ray ring, 1..64, clamped to the
//               ring's largest (default SQ_DEFAULT; 1: a pass every iteration)
struct SptTune {
    int coop = -1, coop_g = 0, coop_waves = -1, routed = -1;
    int budget = 16, batch = 16, stop = -1;     // (stop -1: by window, see heavy_tiers)
    int prio[3] = {-1, -1, -1};
    int wpb = 0, blocks = 0;
    int sq = 0;                                 // (0: SQ_DEFAULT)
};
// The knobs of one RT_SPT_TUNE string (null: the defaults).
inline SptTune spt_tune_parse(const char *e)
{
    SptTune t;
    if (!e) return t;
    std::string all(e);
    size_t pos = 0;
    while (pos < all.size()) {
        size_t end = all.find(',', pos);
        if (end == std::string::npos) end = all.size();
        const std::string kv = all.substr(pos, end - pos);
        pos = end + 1;
        const size_t eq = kv.find('=');
        if (eq == std::string::npos) continue;
        const std::string k = kv.substr(0, eq);
        const char *v = kv.c_str() + eq + 1;
        if (k == "coop") t.coop = std::max(atoi(v), 0);
        else if (k == "coop_g") t.coop_g = atoi(v) == 4 ? 4 : (atoi(v) == 2 ? 2 : 8);
        else if (k == "coop_waves") t.coop_waves = std::min(std::max(atoi(v), 0), 16);
        else if (k == "routed") t.routed = std::max(atoi(v), 0);
        else if (k == "walk") sscanf(v, "%d/%d/%d", &t.budget, &t.batch, &t.stop);
        else if (k == "prio") sscanf(v, "%d/%d/%d", &t.prio[0], &t.prio[1], &t.prio[2]);
        else if (k == "wpb") t.wpb = atoi(v) == 16 ? 16 : 4;
        else if (k == "blocks") t.blocks = std::max(atoi(v), 0);
        else if (k == "sq") t.sq = std::min(std::max(atoi(v), 1), 64);
    }
    return t;
}
inline SptTune spt_tune() { return spt_tune_parse(getenv("RT_SPT_TUNE")); }

// 8-wide hierarchy launches: blocks of WIDE_WPB waves (each holds its own
// LDS copy of the nodes and its waves' stacks), one per CU at the kernel's
// occupancy of 4 waves per SIMD.
constexpr int WIDE_WPB = 16;

// Launch shape: one wave per 8x8 tile of rows [r0, r1).  256-thread blocks
// (several per CU, dispatched as CUs free up) unless the window has at most
// four tiles per SIMD (a multi-GPU row band): then 1024-thread blocks with
// more than half the CU's LDS reserved, so a CU holds exactly one and every
// SIMD gets four waves, instead of the dispatcher's uneven 3..5 per SIMD.
struct Shape {
    int tiles_x, ntiles, gstride, wpb, nblocks;
    int work = 0;                     // tiles this launch renders (ntiles, or 4 x a group list's length)
    int nslots = 0;                   // dispatch slots (tile groups of four) the order / cost arrays cover
    bool wide = false;                // the scene has an 8-wide tree: persistent waves
    const int *order = nullptr;       // adaptive schedule (render_kernel's group_order / group_cost)
    unsigned *cost = nullptr;
    bool tiers = true;                // with order: its first tiles get the heavy-tile treatment
    bool cost_max = false;            // cost: a group's longest tile (atomic max), not the sum
    SptTune tune;
};
// Rows [r0, r1), or (gstride > 1) the 8-row groups r0/8, r0/8 + gstride, ...
// below r1 (r0 a multiple of 8); or (nlist > 0) the nlist tile groups of a
// caller's list over the frame [r0, r1) = [0, h).  cus: the device's compute
// units; wide: the scene has an 8-wide tree.
inline Shape launch_shape(int cus, bool wide, int w, int r0, int r1, int gstride, int nlist, const SptTune &tune)
{
    Shape g;
    g.tune = tune;
    g.wide = wide;
    g.tiles_x = (w + 7) / 8;
    g.gstride = gstride;
    const int groups = (r1 - r0 + 7) / 8;
    g.ntiles = g.tiles_x * ((groups + gstride - 1) / gstride);
    const int work = nlist > 0 ? 4 * nlist : g.ntiles;      // tiles this launch renders
    g.work = work;
    // Waves of work per SIMD: up to 4 (an N = 8 band) run as one round of the
    // 16-wave block shape (four waves per SIMD, one block per CU); 6..8 (an
    // N = 4 band: 7.97) as two such rounds -- at occupancy 6 they run as a
    // full round of 6 and a tail of 2 (N = 4 bands 5.25-5.87 ms -> 5.44-5.47
    // ms); otherwise 256-thread blocks at the kernel's occupancy.
    const double wps = (double)work / (4.0 * cus);
    g.wpb = (wps <= 4.0 || (wps > 6.0 && wps <= 8.0)) ? 16 : 4;
    if (g.tune.wpb) g.wpb = g.tune.wpb;
    g.nblocks = (work + g.wpb - 1) / g.wpb;
    g.nslots = nlist > 0 ? nlist : g.nblocks * (g.wpb / 4);
    if (wide) {                       // persistent waves: one block per CU (fewer for a small window)
        g.wpb = WIDE_WPB;
        g.nblocks = std::min(cus, (work + g.wpb - 1) / g.wpb);
        if (g.tune.blocks) g.nblocks = g.tune.blocks;
        g.nslots = nlist > 0 ? nlist : (g.ntiles + 3) / 4;
    }
    return g;
}

// Priority levelling schedule (render_kernel's prio_sched): levels at 1/4,
// 1/2, 3/4 of the samples for the full-frame shape; for the 16-wave block
// shape (multi-GPU windows of <= 8 waves per SIMD, one or two rounds) at
// 1/2, 3/4, 7/8 -- finer where the co-resident waves drain.
inline int prio_schedule(const Shape &g)
{
    int a = 64, b = 128, c = 192;
    if (g.wpb == 16) { a = 128; b = 192; c = 224; }
    if (g.tune.prio[0] >= 0) { a = g.tune.prio[0]; b = g.tune.prio[1]; c = g.tune.prio[2]; }
    return pack_prio(a, b, c);
}

// Heavy tiles (with a learnt order, 8-wide persistent launches), in
// dispatch order: n1 cooperative tiles (cg = 8, 4 or 2 lanes per pixel,
// wide_walk_coop; cg = 0: none), fetched first by hw waves of each block,
// then n2 tiles routed one per SIMD beside lighter waves, then the rest; and
// the walk's early stop.
struct Tiers { int n1 = 0, n2 = 0, cg = 0, hw = 0, stop = 32; };
inline Tiers heavy_tiers(const Shape &g, int cus)
{
    // A window of
    // many waves of work per SIMD (a full frame: 31.6) is throughput-bound:
    // routing only.  A window of few (a multi-GPU rank's share: N = 8 is 4.0,
    // N = 4 7.9, N = 2 15.8) is bound by its heaviest tiles' sample chains,
    // which the cooperative walk shortens ~2x at ~3x their issue cost (8
    // lanes per pixel at N = 8, 4 at N = 4, 2 at N = 2).
    // configs[4], 64 spp (profiles/r03/c4_coop_*.log): N = 8 windows
    // 18.0-19.8 -> 11.4-15.1 ms, N = 4 18.7 -> 17 ms; see DESIGN.md.
    const SptTune &tu = g.tune;
    Tiers t;
    int n1 = 0, n2 = 0;
    if (g.wide && g.order && g.tiers) {
        n2 = std::min(4 * g.nblocks, 4 * g.nslots);
        const double wps = (double)g.work / (4.0 * cus);
        int hw = 0, cg = 8;
        if (wps <= 5.0) {
            n1 = 2 * cus;
            hw = 16;
        } else if (wps <= 10.0) {
            // An N = 4 share holds more ~13 ms chains than 512 tiles at
            // eight lanes per pixel cover (c4_phase_n4.log): twice the tiles
            // at four lanes per pixel, fetched by every wave of the block
            // first (one round: 4 sub-items x 1,024 tiles = 16 waves per CU).
            // N = 4 shares 16.3-16.6 -> 13.8 ms; at N = 8 four lanes lose
            // (9.9 -> 13.5 ms), c4_coop_g4_ab.log.
            n1 = 4 * cus;
            hw = 16;
            cg = 4;
        } else if (wps <= 20.0) {
            // An N = 2 share (15.8 waves of work per SIMD): still bound by its
            // heaviest chains, and too full for four- or eight-lane tiers to
            // pay (20.5 -> 19.8-23 ms); two lanes per pixel for the heaviest
            // 1,024 tiles halve their walks at the least duplicated shading:
            // 20.5 -> 19.3-19.5 ms (round 6, c4_coop_g2_ab.log; 768-1,024
            // best, 1,280+ slower; at N = 4 two lanes lose to four).
            n1 = 4 * cus;
            cg = 2;
        }
        if (tu.coop_g) cg = tu.coop_g;
        if (tu.coop >= 0) n1 = tu.coop;
        if (tu.coop_waves >= 0) hw = tu.coop_waves;
        if (n1 > 0) n2 = 0;   // routed tiles beside cooperative ones: N = 4 17 -> 24 ms (c4_coop_tiers_ab.log)
        if (tu.routed >= 0) n2 = tu.routed;
        n1 = std::min(n1, 4 * g.nslots);
        n2 = std::min(n2, 4 * g.nslots - n1);
        t.cg = n1 > 0 ? cg : 0;
        t.hw = n1 > 0 ? hw : 0;
    }
    t.n1 = n1;
    t.n2 = n2;
    // A walk call returns once <= stop/64 of the lanes that started it
    // still walk: 32 on the full frame; 16 in a window with a cooperative
    // tier, where the heaviest waves' chains bound the share (round 6,
    // with the deferred leaf sections: N = 8 9.5 -> 9.2 ms, N = 4 13.2 ->
    // 12.8 ms, profiles/r06/c4_walk_stop_sweep.log).
    t.stop = tu.stop >= 0 ? tu.stop : (n1 > 0 ? 16 : 32);
    return t;
}

// The split word of an 8-wide launch (the other kernels take 0): the tiers'
// sub-item shape and the walk options, clamped to their fields.
inline int split_word(const Shape &g, const Tiers &t)
{
    const int hs = t.cg == 8 ? 3 : t.cg == 4 ? 2 : t.cg == 2 ? 1 : 0;
    return pack_split(hs, t.cg != 0, t.hw, std::min(std::max(g.tune.budget, 1), 255),
                      std::min(std::max(g.tune.batch, 0), 64), std::min(std::max(t.stop, 0), 64));
}

}  // namespace sptpolicy

#endif
