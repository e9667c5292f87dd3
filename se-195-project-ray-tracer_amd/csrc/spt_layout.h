// spt_layout.h -- the one description of smallpt's render_kernel variants and
// of the dynamic LDS each of them carves: the kernel families, the predicates
// that tell the variants apart, the occupancy bounds, every offset and size of
// the carve, and block_lds_bytes -- the bytes a launch asks for.  Arithmetic
// only, no HIP types: render_kernel addresses its LDS by it, launch() sizes
// the launch by it, spt_bvh.h budgets the 8-wide tree by it, and the CPU check
// tests/native/layout_check.cpp sweeps it under g++ (regions disjoint, aligned,
// inside the total; DESIGN.md §3's figures).
#ifndef SPT_LAYOUT_H
#define SPT_LAYOUT_H

#include <stddef.h>
#include "spt_policy.h"

namespace sptlayout {

// ---- kernel families (rt_hip.h's SPT_GEO_*, spt_scene_info word 0) and the
// counter modes of a launch: none, all four counters, or calls and samples
// only (SPT_COUNT_RAYS: the uncounted queries).
constexpr int GEO_LDS = 0, GEO_GLOBAL = 1, GEO_BVH = 2, GEO_WIDE = 3;
enum { CNT_NONE = 0, CNT_FULL = 1, CNT_RAYS = 2 };

// Occupancy of the kernel variants (__launch_bounds__ minimum waves per
// SIMD; every bound measured against its neighbours):
//   full-scan one-query kernels: unbounded (1);
//   the uncounted two-query kernel (DUAL): 7 -- 85 -> 72 VGPRs, no VGPR
//     spills, occupancy 5 -> 7: Cornell 1080p 17.87 -> 17.3 ms.  8 measured
//     without scratch (colour, coordinates and camera terms parked: 64
//     VGPRs, private segment 0) and not kept: 8 waves cap the kernel at 80
//     SGPRs, the rest go through v_readlane in every iteration (+1.05 % VALU
//     instructions), and the eighth wave buys no rate: 16.98 ms against
//     16.57 ms for the same code at 7 (profiles/r07).  With
//     its shadow rays deferred to the per-wave ring (dq) and the lane's
//     parking address held across the loop it holds 71 VGPRs (72 reading
//     the spheres from global memory);
//   binary-hierarchy (GEO_BVH) kernels: 6 -- 93 -> 80 VGPRs (2 spilled): the
//     latency-bound walk gains more from the sixth wave than the spills cost;
//   8-wide (GEO_WIDE) kernels: 4 -- 126 VGPRs unbounded; 5 or 6 spill;
//   counted hierarchy kernels (not timed): 4, room for the counters.
constexpr int SPT_MINWAVES = 1, SPT_DUAL_MINWAVES = 7, BVH_MINWAVES = 6, WIDE_MINWAVES = 4, BVH_MINWAVES_COUNT = 4;

// One render_kernel variant: its template arguments (the counter mode stands
// for COUNT and RAYS; cg is the lanes per pixel of an 8-wide kernel's
// cooperative walk, 0: none) and everything that follows from them.
struct Variant {
    int geo;
    bool dl, dual;
    int cmode, cg;
    SPT_HD constexpr bool count() const { return cmode == CNT_FULL; }
    SPT_HD constexpr bool rays() const { return cmode == CNT_RAYS; }
    SPT_HD constexpr bool lds() const { return geo == GEO_LDS; }                   // the scene is copied into LDS
    SPT_HD constexpr bool park() const { return geo == GEO_LDS || geo == GEO_GLOBAL; }   // full scan: cold state parked in LDS
    SPT_HD constexpr bool dq() const { return dual && cmode == CNT_NONE && park(); }    // shadow rays deferred to the ring
    // the lane's parking address is held in a register across the pixel loop
    // (else: rebuilt from the thread index at every use -- the counted
    // one-query global-memory kernels, which the register would take from 80
    // VGPRs to 81 and from six waves per SIMD to five)
    SPT_HD constexpr bool held_addr() const { return park() && !(geo == GEO_GLOBAL && cmode == CNT_FULL && !dual); }
    // the one-ray queries' accept tests run on integer keys (spt_accept.h);
    // else: on floats -- the two-query global-memory kernels that keep
    // counters, where the keyed form costs the counted one two VGPRs and its
    // sixth wave per SIMD (79 -> 81) and puts two more v_readlane into the
    // RAYS one's loop; their one-ray query runs only in iterations without a
    // shadow ray
    SPT_HD constexpr bool key_accept() const { return park() && !(geo == GEO_GLOBAL && dual && cmode != CNT_NONE); }
    // pass A's and pass B's angles go through rtm::sincos_2pi_draw and pass B's
    // sqrt(1 - x2) through sqrt_nr without its range guard (both exact on a
    // draw's 2^23 values); else: rtm::sincosf and sqrt_exact -- the hierarchy
    // kernels, which sit at their register bounds (6 and 4 waves per SIMD)
    // and answer the shorter forms with more scratch, a lost wave (the RAYS
    // binary kernels, 95 -> 99 VGPRs) or up to 25 more v_readlane inside
    // their loops (profiles/r17/sincos_draw_resource_usage.txt)
    SPT_HD constexpr bool draw_trig() const { return park(); }
    SPT_HD constexpr bool persist() const { return geo == GEO_WIDE; }              // waves fetch tiles from a work counter
    SPT_HD constexpr bool sched() const { return geo == GEO_BVH || geo == GEO_WIDE; }   // group order / cost code
    SPT_HD constexpr bool gstore() const { return geo == GEO_BVH; }                // stores staged per tile group
    SPT_HD constexpr int min_waves() const
    {
        return geo == GEO_BVH    ? (cmode != CNT_NONE ? BVH_MINWAVES_COUNT : BVH_MINWAVES)
               : geo == GEO_WIDE ? (cmode != CNT_NONE ? BVH_MINWAVES_COUNT : WIDE_MINWAVES)
                                 : (dq() ? SPT_DUAL_MINWAVES : SPT_MINWAVES);
    }
};
// The variant of render_kernel's template arguments.
SPT_HD constexpr Variant variant_of(int geo, bool dl, bool dual, bool count, bool rays, int cg)
{
    return Variant{geo, dl, dual, count ? CNT_FULL : rays ? CNT_RAYS : CNT_NONE, cg};
}

// ---- the CU's LDS and the budgets taken from it
constexpr int CU_LDS_BYTES = 160 * 1024;
// A 16-wave block asks for at least this much -- more than half the CU's LDS
// -- so that a CU holds exactly one (spt_policy.h launch_shape).
constexpr int ONE_PER_CU_LDS_BYTES = CU_LDS_BYTES / 2 + 1024;
// A scene whose copy is at most this large gets the LDS family.
constexpr int MAX_LDS_BYTES = 96 * 1024;
// The 8-wide tree's nodes and stacks: leaves a CU room for that one block.
constexpr int WIDE_LDS_MAX = 144 * 1024;

// ---- GEO_LDS: the scene copy at offset 0, float4 records geo | emi | col (n
// each) | lrec (3 per light; a light-free scene has one zero record) -- a copy
// of the scene's global SoA (spt_scene_create).
constexpr int RECORD_BYTES = 16;
SPT_HD constexpr int scene_records(int n, int nlights) { return 3 * n + 3 * (nlights > 0 ? nlights : 1); }
SPT_HD constexpr int scene_bytes(int n, int nlights) { return RECORD_BYTES * scene_records(n, nlights); }

// ---- full-scan kernels: the parking area, after the scene copy (GEO_GLOBAL:
// at offset 0).  Its head holds the block's copy of the camera terms (four
// float4); then one area per wave of lane-private slots, dword slot * 64 +
// lane (conflict-free, and only the lane itself touches its dwords): the
// running-average colour and, deferred form only, the parked previous
// sample's radiance and the second pending contribution; then (deferred) the
// wave's shadow-ray ring, RING_FIELDS dwords per entry as SoA -- field f of
// entry e at RING_BASE_DW + f * RING_FIELD_DW + e.
constexpr int PARK_HEAD_BYTES = 4 * RECORD_BYTES;
constexpr int SLOT_COL = 0, SLOT_RAD = 3, SLOT_PEND = 6;     // three slots (x, y, z) each
constexpr int PARK_SLOTS = 3, DQ_SLOTS = 9;
constexpr int RING_FIELDS = 7, RING_FIELD_DW = sptpolicy::SQ_RING;   // origin, direction, maxt
constexpr int RING_BASE_DW = DQ_SLOTS * 64;
SPT_HD constexpr int wave_dwords(bool dq) { return dq ? RING_BASE_DW + RING_FIELDS * RING_FIELD_DW : PARK_SLOTS * 64; }
SPT_HD constexpr int park_offset(const Variant &v, int n, int nlights) { return v.lds() ? scene_bytes(n, nlights) : 0; }
SPT_HD constexpr size_t park_bytes(bool dq, int wpb) { return PARK_HEAD_BYTES + (size_t)wpb * 4 * wave_dwords(dq); }

// ---- GEO_BVH: per tile group (four waves) of the block a 32x8 staging strip
// -- 8 rows of 96 colour floats, of 64 seed words, of 32 pixels -- and the
// group's arrival count.
constexpr int GS_COL_OFF = 0;
constexpr int GS_SEED_OFF = GS_COL_OFF + 8 * 96 * 4;
constexpr int GS_PX_OFF = GS_SEED_OFF + 8 * 64 * 4;
constexpr int GS_COUNT_OFF = GS_PX_OFF + 8 * 32 * 4;
constexpr int GS_BYTES = (GS_COUNT_OFF + 4 + 15) & ~15;

// ---- GEO_WIDE: the nodes at offset 0 (seven 16-B reads each; counted
// kernels: then 32 B of per-slot highest indices per node, for the any-hit
// walk), then per wave its lanes' stacks, one 64-lane dword level per tree
// level below the root (at least one is reserved).
constexpr int WIDE_NODE_BYTES = 7 * 16, WIDE_MAXID_BYTES = 2 * 16;
constexpr int WIDE_LEVEL_DW = 64;
SPT_HD constexpr int wide_node_bytes(bool counted) { return WIDE_NODE_BYTES + (counted ? WIDE_MAXID_BYTES : 0); }
SPT_HD constexpr size_t wide_stack_offset(int wnodes, bool counted) { return (size_t)wide_node_bytes(counted) * wnodes; }
SPT_HD constexpr size_t wide_lds_bytes(int wnodes, int wdepth, int wpb, bool counted)
{
    return wide_stack_offset(wnodes, counted) + (size_t)wpb * 4 * WIDE_LEVEL_DW * (wdepth > 1 ? wdepth - 1 : 1);
}

// ---- a launch's total
struct SceneSizes { int n, nlights, wnodes, wdepth; };

// The dynamic LDS of a block of wpb waves of variant v: what the kernel
// addresses, and for a 16-wave block of the three non-persistent families the
// one-per-CU reservation.  (An 8-wide block is alone on its CU by its
// registers: 16 waves at four per SIMD.)
SPT_HD constexpr size_t block_lds_bytes(const Variant &v, const SceneSizes &s, int wpb)
{
    if (v.geo == GEO_WIDE) return wide_lds_bytes(s.wnodes, s.wdepth, wpb, v.count());
    size_t b = v.gstore() ? (size_t)(wpb / 4) * GS_BYTES : park_offset(v, s.n, s.nlights) + park_bytes(v.dq(), wpb);
    if (wpb == 16 && b < (size_t)ONE_PER_CU_LDS_BYTES) b = ONE_PER_CU_LDS_BYTES;
    return b;
}

// The family a launch of scene family `geo` runs: the LDS family only while
// its block fits the CU -- a large scene copy beside sixteen waves' rings does
// not -- else the global-memory full scan of the same variant, which reads the
// SoA the copy is made from and computes the same bits.
SPT_HD constexpr int launch_geo(Variant v, const SceneSizes &s, int wpb)
{
    return (v.geo == GEO_LDS && block_lds_bytes(v, s, wpb) > (size_t)CU_LDS_BYTES) ? GEO_GLOBAL : v.geo;
}

// ---- ray queries (spt_query.h's query_kernel): blocks of QUERY_WPB waves, 16
// for the 8-wide family -- the shape its tree was budgeted for (spt_bvh.h
// choose_wide), so nodes, highest-index table and stacks fit WIDE_LDS_MAX.
// LDS family: the geo records alone at offset 0; 8-wide family: GEO_WIDE's
// carve above, `counted` for the kind that seeks the highest-index occluder;
// the other two families use none.
constexpr int QUERY_WPB = 4, QUERY_WPB_WIDE = sptpolicy::WIDE_WPB;
SPT_HD constexpr int query_wpb(int geo) { return geo == GEO_WIDE ? QUERY_WPB_WIDE : QUERY_WPB; }
SPT_HD constexpr size_t query_lds_bytes(int geo, const SceneSizes &s, bool counted)
{
    return geo == GEO_WIDE  ? wide_lds_bytes(s.wnodes, s.wdepth, QUERY_WPB_WIDE, counted)
           : geo == GEO_LDS ? (size_t)RECORD_BYTES * s.n
                            : 0;
}

// ---- radiance queries (spt_radiance.h's radiance_kernel): query_kernel's
// blocks.  LDS family: the whole scene copy -- geo | emi | col | lrec, as
// render_kernel stages it -- at offset 0; 8-wide family: the uncounted
// GEO_WIDE carve (nodes and stacks; the materials stay in global memory); the
// other two families use none.
SPT_HD constexpr size_t radiance_lds_bytes(int geo, const SceneSizes &s)
{
    return geo == GEO_WIDE  ? wide_lds_bytes(s.wnodes, s.wdepth, QUERY_WPB_WIDE, false)
           : geo == GEO_LDS ? (size_t)scene_bytes(s.n, s.nlights)
                            : 0;
}

}  // namespace sptlayout

#endif
