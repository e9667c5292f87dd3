// spt_walk.h -- device code of smallpt's sphere hierarchies: the binary walk
// (bvh_begin, bvh_walk), the 8-wide walk in LDS (wide_begin, wide_walk) and
// its cooperative form (wide_walk_coop).  Not a stand-alone header: smallpt.hip
// includes it inside namespace rt::smallpt, after ray3 / sphere_hit / EPS /
// MISS and spt_policy.h (the packed walk options), before render_kernel.
#ifndef SPT_WALK_H
#define SPT_WALK_H

// ---------------------------------------------------------------------------
// Bounding-volume hierarchy for large scenes (BASELINE configs[4]: 10k
// spheres).  The reference tests every sphere for every ray (geomfunc.h:71-
// 110); the result is the minimum over spheres of the float distance d_i of
// SphereIntersect, ties to the highest index (Intersect), or "some d_i <
// maxt" (IntersectP).  Both are order-independent, so a traversal that
// computes d_i with the reference's exact float formula for every sphere it
// visits, and skips a sphere only when d_i provably cannot matter, returns
// identical bits.
//
// Skipping rule.  For a sphere (radius r, |c - o| = |op|) inside box B
// (centre C, half-diagonal R), a float distance t* puts the point o + t*.d
// within  m = 1.04e-3 * (|op| + r) + sqrt(e) * t*  of the sphere, hence of B:
//   * the float root b -+ sqrt(det) differs from the geometric one by at most
//     sqrt(|det error|) + |b error|, with |det error| <= ~18u max(|op|, r)^2
//     (u = 2^-24; det = b*b - op.op + rad^2 cancels in float) -> 1.04e-3 *
//     max(|op|, r);
//   * a direction with |d|^2 = 1 + e puts the formula's roots on a sphere of
//     radius sqrt(r^2 + e t*^2), i.e. sqrt(e) * t* further out.
// With |op| <= |o - C| + R, r <= R and t* <= |o - C| + 2R this is below
// (1.04e-3 + sqrt(e)) |o - C| + (1.04e-3 + 2 sqrt(e)) R.  The margin is
// alpha * |o - C| + BVH_ALPHA_R * R + BETA with a per-ray alpha = 2 x
// (1.04e-3 + sqrt(e' + 2^-22)) (e' the float-computed e, whose rounding the
// 2^-22 covers): twice the bound's first coefficient; BVH_ALPHA_R = 1/64 is
// 1.7 .. 7x the second for e < 2^-16, and beyond that nothing is culled
// (rays here are normalised or built from unit vectors: e ~ 1e-7, alpha ~
// 1/270).  tests/test_bvh_margin.py measures the float roots of grazing rays
// at ~0.57 of the bound.  So a node whose box, grown by m on every side, is not
// crossed by the ray between 0 and lim (the current nearest distance, or
// maxt) holds no sphere that could be taken; its spheres are skipped.  BETA
// and the same slack absorb the slab test's own rounding (approximate
// reciprocals and square root, relative ~1e-6) and the box corners'.
// Spheres whose radius dwarfs the rest (the ground) are tested first, for
// every ray, outside the hierarchy.
struct BvhView {
    const float4 *node;   // 8 octant layouts x 2 per node: (centre.xyz, link) (half-extent.xyz, ALPHA*R + BETA)
    const float4 *geo;    // spheres in hierarchy order: centre, rad^2
    const int *id;        // their reference indices
    const float4 *ageo;   // "always" spheres (tested first)
    const int *aid;
    int nalways, nnodes;
    const uint4 *wnode;   // the 8-wide layout (spt_bvh.h WideBuild: 7 x 16 B per node), staged in LDS
    const uint4 *wmax;    //   per node and slot the highest reference index below (2 x 16 B per node;
                          //   staged by the counted kernels only)
    int wnodes, wdepth;   //   its node count and depth (levels of wide nodes)
};
// (BVH_ALPHA_R = spt_bvh.h's ALPHA_R: applied on the host, in the node records' margin terms)
#ifndef RT_BVH_K
#define RT_BVH_K 2.f
#endif

#ifndef RT_BVH_BUDGET
#define RT_BVH_BUDGET 32    // walk steps per render-loop iteration before a lane's query is suspended
#endif
constexpr float BVH_K = RT_BVH_K;           // per-ray alpha: K x the bound's |o - C| coefficient
constexpr int BVH_LEAF_MAX = 4;             // spheres per leaf (host build: BVH_LEAF)

// One ray query through the hierarchy.  Nearest hit (shadow = false): t in
// = 1e20f, out = nearest distance, returns its index (highest on ties) or
// -1.  Any hit (shadow = true): t = maxt, returns an occluder index or -1;
// with COUNT the highest one (IntersectP's early-exit position, for the test
// counter), without COUNT the traversal stops at the first.
//
// The walk is latency-bound (one dependent node load per step, L1/L2 hits):
// every step loads both halves of the node record together and runs the slab
// test before branching on the node kind -- leaves are tested against their
// own grown box too -- and a leaf issues the loads of all its spheres and
// indices before the first test, so a step costs one memory latency (a first
// form that branched on the link word first and loaded per sphere paid two
// to five: configs[4] 11.1 -> 8.5 ms per 4 spp).

// A query's walk state, kept across loop iterations of render_kernel: the
// walk is resumable, so a lane whose walk is long does not hold up the
// other lanes of its wave (they shade and start their next queries while it
// continues).  t = nearest distance so far (any hit: maxt, unchanged), id =
// the result so far, node = next node in the ray's octant layout (nnodes:
// finished), pend = a crossed leaf not yet tested (first | count << 24).
// Leaf postponement: a lane may hold two crossed leaves and keeps stepping
// while it holds one; the wave tests pending leaves once >= BVH_BATCH/64 of
// its lanes in the walk cannot step (hold two, or reached the end with one).
constexpr int BVH_BATCH = 16;
struct BvhWalk {
    float t;
    int id, node, pend;
    unsigned m;             // 8-wide walk: node = the current node (-1: root not yet visited), m = its
    int sp, bpos;           //   children still to visit (visit order), sp = stacked (node, mask) entries,
                            //   bpos = hierarchy position of the best leaf hit so far (-1: none)
    int pend2;              // a second crossed leaf (only while pend holds one)
#ifdef RT_SPT_TRACE
    unsigned tr_leaf, tr_trips, tr_leafruns;   // tools-only phase stamps (s_memtime cycles, counts)
#endif
#ifdef RT_SPT_PROF
    unsigned pf_l[3], pf_w[3];   // tools-only: lanes / wave-executions of wide_walk calls, node steps, leaf passes
#endif
};
#ifdef RT_SPT_PROF
#define WALK_PROF(W, b)                                                                    \
    do {                                                                                   \
        (W).pf_l[b]++;                                                                     \
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(__builtin_amdgcn_read_exec())) (W).pf_w[b]++; \
    } while (0)
#define SPT_PROF_ONLY(...) __VA_ARGS__
#else
#define WALK_PROF(W, b) do {} while (0)
#define SPT_PROF_ONLY(...)
#endif
// Tools-only statements and declarations: SPT_TRACE(...) stands as written in
// the -DRT_SPT_TRACE build, SPT_PROF_ONLY(...) in the -DRT_SPT_PROF build, and
// each vanishes from every other build.
#ifdef RT_SPT_TRACE
#define SPT_TRACE(...) __VA_ARGS__
#else
#define SPT_TRACE(...)
#endif

// Starts a query: the "always" spheres, then the walk from the root.
// Nearest hit (shadow = false): t = 1e20f on entry; any hit: t = maxt.
template <bool COUNT>
__device__ __forceinline__ void bvh_begin(const BvhView &B, const ray3 &r, bool shadow, float t, BvhWalk &W)
{
    const float maxt = t;
    int id = -1;
    for (int k = 0; k < B.nalways; k++) {
        const float d = sphere_hit(B.ageo[k], r);
        const int i = B.aid[k];
        if (shadow) {
            if (d < maxt && i > id) id = i;
        } else if (d < t || (d == t && i > id)) {
            t = d;
            id = i;
        }
    }
    W.t = t;
    W.id = id;
    W.node = (!COUNT && shadow && id >= 0) ? B.nnodes : 0;
    W.pend = 0;
    W.pend2 = 0;
}

// A ray's terms of the slab tests (culling only: their rounding is inside the
// margin; fused ops are fine here and nowhere else): the direction with zero
// components made +-1e-30 so no 0 * inf appears, its reciprocals, the per-ray
// margin coefficient alpha and the direction octant.
struct WalkRay {
    float dx, dy, dz, ix, iy, iz, alpha;
    int oct;
};
__device__ __forceinline__ WalkRay walk_ray(const ray3 &r)
{
    WalkRay q;
    q.dx = fabsf(r.d.x) < 1e-30f ? copysignf(1e-30f, r.d.x) : r.d.x;
    q.dy = fabsf(r.d.y) < 1e-30f ? copysignf(1e-30f, r.d.y) : r.d.y;
    q.dz = fabsf(r.d.z) < 1e-30f ? copysignf(1e-30f, r.d.z) : r.d.z;
    q.ix = __builtin_amdgcn_rcpf(q.dx), q.iy = __builtin_amdgcn_rcpf(q.dy), q.iz = __builtin_amdgcn_rcpf(q.dz);
    const float e = fabsf(r.d.x * r.d.x + r.d.y * r.d.y + r.d.z * r.d.z - 1.f);
    q.alpha = e < 0x1p-16f ? BVH_K * (1.04e-3f + __builtin_amdgcn_sqrtf(e + 0x1p-22f)) : 1e30f;
    q.oct = (q.dx < 0.f ? 1 : 0) | (q.dy < 0.f ? 2 : 0) | (q.dz < 0.f ? 4 : 0);
    return q;
}

// The SphereIntersect distances dq (MISS: none) of spheres f .. f + c4 - 1
// (c4 <= BVH_LEAF_MAX; entries past c4 are not used) of the hierarchy order:
// all loads first (one latency per leaf), then branch-free sphere tests (as
// query_bf): sqrt_nr is exact for det in [2^-96, inf) and NaN below 0 (a
// miss); a wave with a lane meeting 0 <= |det| < 2^-96 redoes the leaf with
// sphere_hit.
__device__ __forceinline__ void leaf_dist4(const BvhView &B, const ray3 &r, int f, int c4, float (&dq)[BVH_LEAF_MAX])
{
    float4 g[BVH_LEAF_MAX];
#pragma unroll
    for (int q = 0; q < BVH_LEAF_MAX; q++) g[q] = B.geo[f + (q < c4 ? q : 0)];
    bool bad = false;
#pragma unroll
    for (int q = 0; q < BVH_LEAF_MAX; q++) {
        const float opx = g[q].x - r.o.x, opy = g[q].y - r.o.y, opz = g[q].z - r.o.z;
        const float bb = opx * r.d.x + opy * r.d.y + opz * r.d.z;
        const float det = bb * bb - (opx * opx + opy * opy + opz * opz) + g[q].w;
        bad = bad || (q < c4 && fabsf(det) < 0x1p-96f);
        const float sd = sqrt_nr(det);
        const float t1 = bb - sd, t2 = bb + sd;
        dq[q] = t1 > EPS ? t1 : (t2 > EPS ? t2 : MISS);
    }
    if (wave_any(bad)) {
#pragma unroll
        for (int q = 0; q < BVH_LEAF_MAX; q++) dq[q] = sphere_hit(g[q], r);
    }
}

// Advances the walks of the wave's lanes by up to RT_BVH_BUDGET steps
// (node visits); returns true for a lane whose query is complete: W.id is
// then the nearest sphere (highest index on ties) with W.t its distance, or
// for any hit an occluder index (COUNT: the highest one, IntersectP's
// early-exit position, for the test counter; without COUNT the walk stops
// at the first) or -1.
template <bool COUNT>
__device__ bool bvh_walk(const BvhView &B, const ray3 &r, bool shadow, BvhWalk &W)
{
    const float maxt = W.t;
    float t = W.t;
    int id = W.id, node = W.node, pend = W.pend, pend2 = W.pend2;
    const WalkRay wr = walk_ray(r);
    const float ix = wr.ix, iy = wr.iy, iz = wr.iz, alpha = wr.alpha;
    // Layout of this ray's direction octant: near children first.  A 32-bit
    // element offset from the uniform base (one VGPR, not a 64-bit pointer).
    const unsigned lay = 2u * (unsigned)B.nnodes * (unsigned)wr.oct;
    // Crossed leaves are postponed: a lane that reaches one keeps it pending
    // and steps on until it holds a second; the wave tests one pending leaf
    // per lane together once at least BVH_BATCH/64 of its lanes still in the
    // walk cannot step (or
    // none can), instead of running the leaf block for the one or two lanes
    // that reach a leaf in a given step.  The result does not depend on the
    // order spheres are tested in (minimum, ties to the highest index; or
    // "some occluder"); a leaf tested later than it was crossed only makes
    // the culling limit t of the steps in between looser, never wrong.
    int trips = 0;
    while (true) {
        if (node < B.nnodes && pend2 == 0) {
            const float4 a = B.node[lay + 2u * (unsigned)node], b = B.node[lay + 2u * (unsigned)node + 1u];
            const int link = __float_as_int(a.w);
            const float lim = shadow ? maxt : t;
            const float cx = a.x - r.o.x, cy = a.y - r.o.y, cz = a.z - r.o.z;
            const float dist = __builtin_amdgcn_sqrtf(__builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz)));
            const float m = __builtin_fmaf(alpha, dist, b.w);
            const float tcx = cx * ix, tcy = cy * iy, tcz = cz * iz;                // slab centres
            const float hx = (b.x + m) * fabsf(ix), hy = (b.y + m) * fabsf(iy), hz = (b.z + m) * fabsf(iz);  // slab half-widths
            const float tn = fmaxf(fmaxf(tcx - hx, tcy - hy), tcz - hz);
            const float tf = fminf(fminf(tcx + hx, tcy + hy), tcz + hz);
            const bool cross = tn <= tf && tf >= 0.f && tn <= lim;
            int next = cross ? node + 1 : link;
            if (link < 0) {                              // leaf ~(first | count << 24); escape = next node
                next = node + 1;
                if (cross) {
                    if (pend == 0) pend = ~link;
                    else pend2 = ~link;
                }
            }
            node = next;
        }
        trips++;
        const unsigned long long pm = __builtin_amdgcn_ballot_w64(pend != 0);
        const unsigned long long sm = __builtin_amdgcn_ballot_w64(node < B.nnodes && pend2 == 0);
        if (pm == 0) {
            if (sm == 0 || trips >= RT_BVH_BUDGET) break;
            continue;
        }
        if (sm != 0 && trips < RT_BVH_BUDGET &&
            64 * __builtin_popcountll(pm & ~sm) < BVH_BATCH * __builtin_popcountll(pm | sm))
            continue;
        SPT_TRACE(const unsigned long long tr_l0 = __builtin_amdgcn_s_memtime(); W.tr_leafruns++;)
        if (pend != 0) {
            const int f = pend & 0xffffff, c = pend >> 24;
            float dq[BVH_LEAF_MAX];
            leaf_dist4(B, r, f, c, dq);
            // The spheres' reference indices are not loaded with the leaf
            // (four VGPRs less across the walk): the leaf's new best is kept
            // as its hierarchy position and its index loaded once, after the
            // tests; only ties (and the counted any-hit's highest occluder)
            // load an index on the spot.
            int bpos = -1;
#pragma unroll
            for (int q = 0; q < BVH_LEAF_MAX; q++) {
                if (q < c) {
                    const float d = dq[q];
                    if (shadow) {
                        if (d < maxt) {
                            if (COUNT) {
                                const int i = B.id[f + q];
                                if (i > id) id = i;
                            } else {
                                bpos = f + q;
                            }
                        }
                    } else if (d < t) {
                        t = d;
                        bpos = f + q;
                    } else if (d == t) {
                        const int cur = bpos >= 0 ? B.id[bpos] : id;
                        if (B.id[f + q] > cur) bpos = f + q;
                    }
                }
            }
            if (bpos >= 0) id = B.id[bpos];
            if (!COUNT && shadow && id >= 0) {
                node = B.nnodes;
                pend2 = 0;
            }
            pend = pend2;
            pend2 = 0;
        }
        SPT_TRACE(W.tr_leaf += (unsigned)(__builtin_amdgcn_s_memtime() - tr_l0);)
        if (trips >= RT_BVH_BUDGET) break;
    }
    SPT_TRACE(W.tr_trips += trips;)
    W.t = t;
    W.id = id;
    W.node = node;
    W.pend = pend;
    W.pend2 = pend2;
    return node >= B.nnodes && pend == 0;
}

// ---------------------------------------------------------------------------
// 8-wide hierarchy in LDS (GEO_WIDE; spt_bvh.h WideBuild).  The binary tree
// above collapsed to 8 children per node with the child boxes quantised to 8
// bits per plane (rounded outward on the host): configs[4]'s 10k spheres,
// leaves of <= 8, make 528 nodes = 59 KB, which every block stages in LDS.
// A query visits ~7 wide nodes instead of ~15 binary ones, and each visit is
// an LDS read instead of a dependent L2 access: the binary walk's trip cost
// ~1,300 cycles even with its wave alone on the chip (tools/c5_phase.py), its
// latency, not contention, set configs[4]'s critical path.
//
// Culling is the binary walk's rule with the margin taken over the node: a
// child box is skipped when the ray misses it grown by m = alpha * (|o - p| +
// D0) + K, where |o - p| + D0 >= |o - C| for every child centre C and K is the
// largest child's ALPHA_R * R + BETA -- m is at least each child's own binary
// margin.  The slab test in the node's quantisation frame rounds within
// ~2^-22 (|o - p| + D0) of the exact box planes, far inside alpha's factor-2
// slack.  Visit order: the child in slot p ^ octant at position p (the host
// put each octant's front child in the slot of that octant); the per-lane
// stack holds (node << 8 | remaining mask) entries in LDS, one per level.
// idmin >= 0 (the counted any-hit): only children holding a reference index
// above idmin (hid: the node's eight highest-index words) are crossed.
__device__ __forceinline__ unsigned wide_visit(const uint4 *__restrict__ N, const ray3 &r, const WalkRay &wr, float lim,
                                               const unsigned *__restrict__ hid = nullptr, int idmin = -1)
{
    const float ix = wr.ix, iy = wr.iy, iz = wr.iz, alpha = wr.alpha;
    const int oct = wr.oct;
    const uint4 h0 = N[0];
    const float2 h1 = *(const float2 *)(N + 1);
    const float cx = __uint_as_float(h0.x) - r.o.x, cy = __uint_as_float(h0.y) - r.o.y,
                cz = __uint_as_float(h0.z) - r.o.z;
    const float dist = __builtin_amdgcn_sqrtf(__builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz)));
    const float m = __builtin_fmaf(alpha, dist + h1.x, h1.y);
    const float ax = __uint_as_float((h0.w & 255u) << 23) * ix;
    const float ay = __uint_as_float(((h0.w >> 8) & 255u) << 23) * iy;
    const float az = __uint_as_float(((h0.w >> 16) & 255u) << 23) * iz;
    const float bx = cx * ix, by = cy * iy, bz = cz * iz;
    const float mx = m * fabsf(ix), my = m * fabsf(iy), mz = m * fabsf(iz);
    const float bnx = bx - mx, bfx = bx + mx, bny = by - my, bfy = by + my, bnz = bz - mz, bfz = bz + mz;
    unsigned valid = h0.w >> 24;
    if (hid && idmin >= 0) {
#pragma unroll
        for (int sl = 0; sl < 8; sl++) valid &= ((int)hid[sl] > idmin ? 1u : 0u) << sl | ~(1u << sl);
    }
    // The child boxes, a half (four slots) at a time: words 16 + 6 h ..
    // 21 + 6 h hold lo_x, lo_y, lo_z, hi_x, hi_y, hi_z of slots 4h .. 4h+3.
    // The near plane of an axis is the low byte for a positive direction.
    const unsigned *W = (const unsigned *)N;
    unsigned hm = 0;
#pragma unroll
    for (int hf = 0; hf < 2; hf++) {
        const unsigned *q = W + 16 + 6 * hf;
        const unsigned lx = q[0], ly = q[1], lz = q[2], ux = q[3], uy = q[4], uz = q[5];
        const unsigned nxw = (oct & 1) ? ux : lx, fxw = (oct & 1) ? lx : ux;
        const unsigned nyw = (oct & 2) ? uy : ly, fyw = (oct & 2) ? ly : uy;
        const unsigned nzw = (oct & 4) ? uz : lz, fzw = (oct & 4) ? lz : uz;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int sh = 8 * j, sl = 4 * hf + j;
            const float tnx = __builtin_fmaf((float)((nxw >> sh) & 255u), ax, bnx);
            const float tfx = __builtin_fmaf((float)((fxw >> sh) & 255u), ax, bfx);
            const float tny = __builtin_fmaf((float)((nyw >> sh) & 255u), ay, bny);
            const float tfy = __builtin_fmaf((float)((fyw >> sh) & 255u), ay, bfy);
            const float tnz = __builtin_fmaf((float)((nzw >> sh) & 255u), az, bnz);
            const float tfz = __builtin_fmaf((float)((fzw >> sh) & 255u), az, bfz);
            const float tn = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, 0.f));
            const float tf = fminf(fminf(tfx, tfy), fminf(tfz, lim));
            hm |= ((tn <= tf && ((valid >> sl) & 1u)) ? 1u : 0u) << (sl ^ oct);
        }
    }
    return hm;
}

#ifndef RT_SPT_COOP_NL
#define RT_SPT_COOP_NL 2    // cooperative walk: leaves tested per pass (loads in flight together)
#endif
// (wide_walk's trip budget per call (16), leaf batch threshold (16/64) and
// early stop (end the call once <= 32/64 of its lanes still walk: configs[4]
// 36.3 -> 29.0 ms) come from the host, SptTune.)
constexpr int WIDE_WORDS = 28;   // per node (spt_bvh.h)

template <bool COUNT>
__device__ __forceinline__ void wide_begin(const BvhView &B, const ray3 &r, bool shadow, float t, BvhWalk &W)
{
    bvh_begin<COUNT>(B, r, shadow, t, W);
    W.node = -1;                                        // the root is visited by the first trip
    W.bpos = -1;
    W.m = (!COUNT && shadow && W.id >= 0) ? 0u : 1u;
    W.sp = 0;
}

// Advances the wave's wide walks by up to `budget` trips; returns true
// for a lane whose query is complete (results as bvh_walk).  L: the block's
// LDS copy of the nodes; stk: this wave's LDS stack (entry k of lane l at
// stk[64 k + l]).  Crossed leaves are postponed and tested together as in
// bvh_walk (two pending per lane); a leaf of more than four spheres is tested
// four at a time.
// opts (render_kernel's split word, spt_policy.h): trip budget per call, leaf
// batch threshold in 1/64 of the walking lanes, early stop: the call ends once
// at most stop/64 of the lanes that entered it are still walking (64: never).
template <bool COUNT>
__device__ bool wide_walk(const BvhView &B, const uint4 *__restrict__ L, unsigned *__restrict__ stk, const ray3 &r,
                          bool shadow, BvhWalk &W, int opts)
{
    const int budget = sptpolicy::split_budget(opts), batch = sptpolicy::split_batch(opts),
              stop = sptpolicy::split_stop(opts);
    const float maxt = W.t;
    float t = W.t;
    // The best leaf hit so far is kept as its hierarchy position (bpos) and
    // its reference index loaded once, when the query completes -- not after
    // every leaf pass (a dependent global load: ~1/3 of a lone wave's leaf
    // pass, tools/c5_phase.py).  Ties and the counted any-hit's highest
    // occluder still load indices on the spot.
    int id = W.id, cur = W.node, pend = W.pend, pend2 = W.pend2, sp = W.sp, bpos = W.bpos;
    unsigned m = W.m;
    const WalkRay wr = walk_ray(r);
    const int oct = wr.oct;
    const unsigned *Lw = (const unsigned *)L;
    const unsigned *Lmax = COUNT ? (const unsigned *)(L + 7 * B.wnodes) : nullptr;   // (counted kernels)
    unsigned *my = stk + (threadIdx.x & 63);
    const int n0 = __builtin_popcountll(__builtin_amdgcn_ballot_w64(true));   // lanes in this call
    int trips = 0;
    WALK_PROF(W, 0);
    while (true) {
        if (m != 0 && pend2 == 0) {
            WALK_PROF(W, 1);
            int cw;
            if (cur < 0) {
                cw = 0;                                  // the root
                m = 0;
            } else {
                const int p = __builtin_ctz(m);
                m &= m - 1;
                cw = (int)Lw[cur * WIDE_WORDS + 8 + (p ^ oct)];
            }
            if (cw < 0) {
                if (pend == 0) pend = ~cw;
                else pend2 = ~cw;
            } else {
                const unsigned hm =
                    COUNT ? wide_visit(L + 7 * cw, r, wr, shadow ? maxt : t, Lmax + 8 * cw, shadow ? id : -1)
                          : wide_visit(L + 7 * cw, r, wr, shadow ? maxt : t);
                if (hm) {
                    if (m) {
                        my[64 * sp] = ((unsigned)cur << 8) | m;
                        sp++;
                    }
                    cur = cw;
                    m = hm;
                }
            }
            if (m == 0 && sp > 0) {
                sp--;
                const unsigned e2 = my[64 * sp];
                cur = (int)(e2 >> 8);
                m = e2 & 255u;
            }
        }
        trips++;
        const unsigned long long pm = __builtin_amdgcn_ballot_w64(pend != 0);
        const unsigned long long sm = __builtin_amdgcn_ballot_w64(m != 0 && pend2 == 0);
        const bool out = trips >= budget || 64 * __builtin_popcountll(pm | sm) <= stop * n0;
        if (pm == 0) {
            if (sm == 0 || out) break;
            continue;
        }
        if (sm != 0 && !out && 64 * __builtin_popcountll(pm & ~sm) < batch * __builtin_popcountll(pm | sm))
            continue;
        SPT_TRACE(const unsigned long long tr_l0 = __builtin_amdgcn_s_memtime(); W.tr_leafruns++;)
        if (pend != 0) {
            WALK_PROF(W, 2);
            const int f = pend & 0xffffff, c = pend >> 24, c4 = c < BVH_LEAF_MAX ? c : BVH_LEAF_MAX;
            float dq[BVH_LEAF_MAX];
            leaf_dist4(B, r, f, c4, dq);
#pragma unroll
            for (int q = 0; q < BVH_LEAF_MAX; q++) {
                if (q < c4) {
                    const float d = dq[q];
                    if (shadow) {
                        if (d < maxt) {
                            if (COUNT) {
                                const int i = B.id[f + q];
                                if (i > id) id = i;
                            } else {
                                bpos = f + q;
                            }
                        }
                    } else if (d < t) {
                        t = d;
                        bpos = f + q;
                    } else if (d == t) {
                        const int cur_id = bpos >= 0 ? B.id[bpos] : id;
                        if (B.id[f + q] > cur_id) bpos = f + q;
                    }
                }
            }
            if (c > BVH_LEAF_MAX) {
                pend = (f + BVH_LEAF_MAX) | ((c - BVH_LEAF_MAX) << 24);
            } else {
                pend = pend2;
                pend2 = 0;
            }
            if (!COUNT && shadow && (id >= 0 || bpos >= 0)) {
                m = 0;
                sp = 0;
                pend = pend2 = 0;
            }
        }
        SPT_TRACE(W.tr_leaf += (unsigned)(__builtin_amdgcn_s_memtime() - tr_l0);)
        if (out) break;
    }
    SPT_TRACE(W.tr_trips += trips;)
    const bool done = m == 0 && pend == 0;
    // (an uncounted any-hit only needs "some occluder": no index load)
    if (done && bpos >= 0) id = (!COUNT && shadow) ? 0x7fffffff : B.id[bpos];
    W.t = t;
    W.id = id;
    W.bpos = bpos;
    W.node = cur;
    W.m = m;
    W.sp = sp;
    W.pend = pend;
    W.pend2 = pend2;
    return done;
}

// ---------------------------------------------------------------------------
// Cooperative 8-wide walk: EIGHT lanes per ray (the heaviest tiles).
//
// A heavy tile's critical path is one pixel's 64-sample RNG chain of ~900
// loop iterations, each ~24 dependent walk trips; a lone wave issues one VALU
// instruction per ~4 cycles, and a per-lane trip (eight child slab tests, the
// stack, the pending-leaf bookkeeping) costs it ~250 of them.  Here the eight
// lanes of a lane group (lanes 8g .. 8g+7) hold the same pixel -- the same
// ray, RNG words and path state, computed redundantly and identically -- and
// split each trip: lane k tests child slot k ^ oct of the node (its bit of the
// visit mask, gathered with one ballot), or sphere k of a leaf (the group's
// nearest / any hit by a 3-step DPP reduction).  A trip is ~40 VALU
// instructions instead of ~250, a leaf is one pass instead of up to four, and
// the wave walks the maximum over 8 rays instead of 64.  Group-uniform state
// (node, mask, stack, t, bpos, id) is held identically by the 8 lanes; each
// lane keeps its own copy of the stack column, as in wide_walk.  Results are
// the reference's: every sphere a per-lane walk would test is tested with
// the same float formula, and the nearest hit is the minimum distance with
// the highest reference index on ties, an order-independent choice.
// G = 4 (COOP4): four lanes per pixel, two child slots / spheres per lane --
// half the waves per heavy tile for a somewhat longer trip.
// Minimum over the group of non-negative floats (leaf distances: > EPS or
// +inf), compared as integers: the same order, and no NaN canonicalisation.
template <int G>
__device__ __forceinline__ float grp_min(float v)
{
    // (the identity as the DPP's old value lets the compiler fold each move
    // into its v_min_i32)
    constexpr int ID = 0x7fffffff;
    int i = __float_as_int(v);
    i = min(i, __builtin_amdgcn_update_dpp(ID, i, 0xB1, 0xF, 0xF, false));
    if (G >= 4) i = min(i, __builtin_amdgcn_update_dpp(ID, i, 0x4E, 0xF, 0xF, false));
    if (G == 8) i = min(i, __builtin_amdgcn_update_dpp(ID, i, 0x141, 0xF, 0xF, false));
    return __int_as_float(i);
}
template <int G>
__device__ __forceinline__ int grp_max(int v)
{
    constexpr int ID = (int)0x80000000;
    v = max(v, __builtin_amdgcn_update_dpp(ID, v, 0xB1, 0xF, 0xF, false));
    if (G >= 4) v = max(v, __builtin_amdgcn_update_dpp(ID, v, 0x4E, 0xF, 0xF, false));
    if (G == 8) v = max(v, __builtin_amdgcn_update_dpp(ID, v, 0x141, 0xF, 0xF, false));
    return v;
}
// The group's G bits of a predicate (bit k = lane gbase + k).
template <int G>
__device__ __forceinline__ unsigned grp_bits(bool p, int gbase)
{
    return (unsigned)(__builtin_amdgcn_ballot_w64(p) >> gbase) & ((1u << G) - 1u);
}

// wide_visit split over the group: lane k tests the child at visit
// positions k, k + G, ... (slot position ^ oct) and the group's visit mask
// comes back from ballots.  The float operations are wide_visit's, so the
// culling decisions are its own.
template <int G>
__device__ __forceinline__ unsigned wide_visit_coop(const uint4 *__restrict__ N, const ray3 &r, const WalkRay &wr,
                                                    float lim, int pos, int gbase, unsigned &lm,
                                                    const unsigned *__restrict__ hid = nullptr, int idmin = -1)
{
    const float ix = wr.ix, iy = wr.iy, iz = wr.iz, alpha = wr.alpha;
    const int oct = wr.oct;
    const uint4 h0 = N[0];
    const float2 h1 = *(const float2 *)(N + 1);
    uint2 w[8 / G][3];
    int cwk[8 / G];                       // this lane's children's words (< 0: a leaf)
#pragma unroll
    for (int j = 0; j < 8 / G; j++) cwk[j] = (int)((const unsigned *)N)[8 + ((pos + j * G) ^ oct)];
#pragma unroll
    for (int j = 0; j < 8 / G; j++) {
        const unsigned *q = (const unsigned *)N + 16 + 6 * (((pos + j * G) ^ oct) >> 2);
        w[j][0] = *(const uint2 *)q;
        w[j][1] = *(const uint2 *)(q + 2);
        w[j][2] = *(const uint2 *)(q + 4);
    }
    const float cx = __uint_as_float(h0.x) - r.o.x, cy = __uint_as_float(h0.y) - r.o.y,
                cz = __uint_as_float(h0.z) - r.o.z;
    const float dist = __builtin_amdgcn_sqrtf(__builtin_fmaf(cx, cx, __builtin_fmaf(cy, cy, cz * cz)));
    const float m = __builtin_fmaf(alpha, dist + h1.x, h1.y);
    const float ax = __uint_as_float((h0.w & 255u) << 23) * ix;
    const float ay = __uint_as_float(((h0.w >> 8) & 255u) << 23) * iy;
    const float az = __uint_as_float(((h0.w >> 16) & 255u) << 23) * iz;
    const float bx = cx * ix, by = cy * iy, bz = cz * iz;
    const float mx = m * fabsf(ix), my = m * fabsf(iy), mz = m * fabsf(iz);
    const float bnx = bx - mx, bfx = bx + mx, bny = by - my, bfy = by + my, bnz = bz - mz, bfz = bz + mz;
    unsigned hm = 0;
    lm = 0;
#pragma unroll
    for (int j = 0; j < 8 / G; j++) {
        const int sl = (pos + j * G) ^ oct;
        const unsigned lx = w[j][0].x, ly = w[j][0].y, lz = w[j][1].x, ux = w[j][1].y, uy = w[j][2].x,
                       uz = w[j][2].y;
        const unsigned nxw = (oct & 1) ? ux : lx, fxw = (oct & 1) ? lx : ux;
        const unsigned nyw = (oct & 2) ? uy : ly, fyw = (oct & 2) ? ly : uy;
        const unsigned nzw = (oct & 4) ? uz : lz, fzw = (oct & 4) ? lz : uz;
        const int sh = 8 * (sl & 3);
        const float tnx = __builtin_fmaf((float)((nxw >> sh) & 255u), ax, bnx);
        const float tfx = __builtin_fmaf((float)((fxw >> sh) & 255u), ax, bfx);
        const float tny = __builtin_fmaf((float)((nyw >> sh) & 255u), ay, bny);
        const float tfy = __builtin_fmaf((float)((fyw >> sh) & 255u), ay, bfy);
        const float tnz = __builtin_fmaf((float)((nzw >> sh) & 255u), az, bnz);
        const float tfz = __builtin_fmaf((float)((fzw >> sh) & 255u), az, bfz);
        const float tn = fmaxf(fmaxf(tnx, tny), fmaxf(tnz, 0.f));
        const float tf = fminf(fminf(tfx, tfy), fminf(tfz, lim));
        bool hit = tn <= tf && ((h0.w >> (24 + sl)) & 1u);
        if (hid && idmin >= 0) hit = hit && (int)hid[sl] > idmin;
        hm |= grp_bits<G>(hit, gbase) << (j * G);
        lm |= grp_bits<G>(hit && cwk[j] < 0, gbase) << (j * G);
    }
    return hm;
}

// Applies one leaf pass's distances d[j] (sphere b + pos + j G of the leaf
// at f; MISS past its end) to the group's query.  Nearest hit: t / bpos
// updated to the minimum distance, highest reference index on ties (ids
// loaded only then).  Any hit: COUNT -- id = the highest occluder index so
// far; otherwise returns true (occluded: bpos = f) and the caller ends the walk.
template <bool COUNT, int G>
__device__ __forceinline__ bool leaf_apply(const BvhView &B, bool shadow, float maxt, int f, int b, int pos,
                                           int gbase, const float (&d)[8 / G], float &t, int &bpos, int &id)
{
    constexpr int S = 8 / G;
    if (shadow) {
        bool occ[S];
        unsigned any = 0;
#pragma unroll
        for (int j = 0; j < S; j++) {
            occ[j] = d[j] < maxt;
            any |= grp_bits<G>(occ[j], gbase);
        }
        if (COUNT) {
            if (any) {
                int i = -1;
#pragma unroll
                for (int j = 0; j < S; j++)
                    if (occ[j]) i = max(i, B.id[f + b + pos + j * G]);
                i = grp_max<G>(i);
                if (i > id) id = i;
            }
        } else if (any) {
            bpos = f;
            return true;
        }
        return false;
    }
    float dl = d[0];
#pragma unroll
    for (int j = 1; j < S; j++) dl = fminf(dl, d[j]);
    const float dm = grp_min<G>(dl);
    if (dm <= t) {                              // (dm finite: t < +inf)
        unsigned cm[S];
        int nc = 0;
#pragma unroll
        for (int j = 0; j < S; j++) {
            cm[j] = grp_bits<G>(d[j] == dm, gbase);
            nc += __builtin_popcount(cm[j]);
        }
        if (dm < t && nc == 1) {
            int k = 0;
#pragma unroll
            for (int j = 0; j < S; j++)
                if (cm[j]) k = j * G + __builtin_ctz(cm[j]);
            t = dm;
            bpos = f + b + k;
        } else {                                // a tie: within the leaf, or with the best so far
            int il[S], i = -1;
#pragma unroll
            for (int j = 0; j < S; j++) {
                il[j] = d[j] == dm ? B.id[f + b + pos + j * G] : -1;
                i = max(i, il[j]);
            }
            const int im = grp_max<G>(i);
            const int cur_id = dm == t ? (bpos >= 0 ? B.id[bpos] : id) : -1;
            if (im > cur_id) {
                int k = 0;
#pragma unroll
                for (int j = 0; j < S; j++) {
                    const unsigned wm = grp_bits<G>(il[j] == im, gbase);
                    if (wm) k = j * G + __builtin_ctz(wm);
                }
                t = dm;
                bpos = f + b + k;
            }
        }
    }
    return false;
}

// Up to NL leaves (first sphere f[l], c[l] spheres; c = 0: none) for the
// group, sphere b + k + j G of each on lane k: the sphere loads of all of
// them are issued before the first test (one memory latency per pass), the
// leaves then applied in order.  Returns true when an uncounted any-hit
// found an occluder.
// LOCAL (nearest hit): each lane keeps its own best (t, bpos) over the
// spheres it tests -- no group reduction per leaf; wide_walk_coop reduces the
// lanes' bests to the group's culling limit once per leaf section and to the
// result once per query (the minimum with ties to the highest index: the
// same choice, made once).
template <bool COUNT, int G, int NL, bool LOCAL = false>
__device__ __forceinline__ bool leaf_coop(const BvhView &B, const ray3 &r, bool shadow, float maxt,
                                          const int (&f)[NL], const int (&c)[NL], int pos, int gbase, float &t,
                                          int &bpos, int &id)
{
    constexpr int S = 8 / G;
    int cmax = c[0];
#pragma unroll
    for (int l = 1; l < NL; l++) cmax = max(cmax, c[l]);
    for (int b = 0; b < cmax; b += 8) {
        float4 g[NL][S];
#pragma unroll
        for (int l = 0; l < NL; l++)
#pragma unroll
            for (int j = 0; j < S; j++) {
                const int q = b + pos + j * G;
                g[l][j] = B.geo[f[l] + (q < c[l] ? q : 0)];
            }
#pragma unroll
        for (int l = 0; l < NL; l++) {
            if (b >= c[l]) continue;
            float d[S];
            bool bad = false;
#pragma unroll
            for (int j = 0; j < S; j++) {
                const float opx = g[l][j].x - r.o.x, opy = g[l][j].y - r.o.y, opz = g[l][j].z - r.o.z;
                const float bb = opx * r.d.x + opy * r.d.y + opz * r.d.z;
                const float det = bb * bb - (opx * opx + opy * opy + opz * opz) + g[l][j].w;
                bad = bad || (b + pos + j * G < c[l] && fabsf(det) < 0x1p-96f);
                const float sd = sqrt_nr(det);
                const float t1 = bb - sd, t2 = bb + sd;
                d[j] = t1 > EPS ? t1 : (t2 > EPS ? t2 : MISS);
            }
            if (wave_any(bad)) {
#pragma unroll
                for (int j = 0; j < S; j++) d[j] = sphere_hit(g[l][j], r);
            }
#pragma unroll
            for (int j = 0; j < S; j++)
                if (b + pos + j * G >= c[l]) d[j] = MISS;
            if (LOCAL && !shadow) {
#pragma unroll
                for (int j = 0; j < S; j++) {
                    const int q = f[l] + b + pos + j * G;
                    if (d[j] < t) {
                        t = d[j];
                        bpos = q;
                    } else if (d[j] == t) {             // (d finite: a tie)
                        const int cur_id = bpos >= 0 ? B.id[bpos] : id;
                        if (B.id[q] > cur_id) bpos = q;
                    }
                }
            } else if (leaf_apply<COUNT, G>(B, shadow, maxt, f[l], b, pos, gbase, d, t, bpos, id)) {
                return true;
            }
        }
    }
    return false;
}

// The crossed leaves l1 of node n1 and l2 of node n2, RT_SPT_COOP_NL per
// pass; true when an uncounted any-hit found an occluder.
template <bool COUNT, int G, bool LOC>
__device__ __forceinline__ bool coop_leaves(const BvhView &B, const ray3 &r, bool shadow, float maxt,
                                            const unsigned *Lw, int oct, int n1, unsigned l1, int n2, unsigned l2,
                                            int pos, int gbase, float &t, int &bpos, int &id)
{
    constexpr int NL = G == 2 ? 1 : RT_SPT_COOP_NL;   // (two lanes: four spheres a lane per leaf already)
    while (l1 | l2) {
        int fa[NL], ca[NL];
#pragma unroll
        for (int q = 0; q < NL; q++) {
            fa[q] = ca[q] = 0;
            if (l1 | l2) {
                const bool first = l1 != 0;
                const unsigned lq = first ? l1 : l2;
                const int iq = __builtin_ctz(lq);
                l1 = first ? (l1 & (l1 - 1u)) : l1;
                l2 = first ? l2 : (l2 & (l2 - 1u));
                const int wq = ~(int)Lw[(first ? n1 : n2) * WIDE_WORDS + 8 + (iq ^ oct)];
                fa[q] = wq & 0xffffff;
                ca[q] = wq >> 24;
            }
        }
        if (leaf_coop<COUNT, G, NL, LOC>(B, r, shadow, maxt, fa, ca, pos, gbase, t, bpos, id))
            return true;
    }
    return false;
}

template <bool COUNT, int G>
__device__ bool wide_walk_coop(const BvhView &B, const uint4 *__restrict__ L, unsigned *__restrict__ stk,
                               const ray3 &r, bool shadow, BvhWalk &W, int opts)
{
    const int budget = sptpolicy::split_budget(opts), stop = sptpolicy::split_stop(opts);
    const float maxt = W.t;
    float t = W.t;
    int id = W.id, cur = W.node, sp = W.sp, bpos = W.bpos;
    unsigned m = W.m;
    const WalkRay wr = walk_ray(r);
    const int oct = wr.oct;
    const unsigned *Lw = (const unsigned *)L;
    const unsigned *Lmax = COUNT ? (const unsigned *)(L + 7 * B.wnodes) : nullptr;
    unsigned *my = stk + (threadIdx.x & 63);
    const int pos = threadIdx.x & (G - 1), gbase = threadIdx.x & (64 - G);
    const int n0 = __builtin_popcountll(__builtin_amdgcn_ballot_w64(true));
    int trips = 0;
    // One trip as straight-line selects: the next child's word and the
    // stack top are read together at the trip's start (the pop can only
    // need the entry below the current top: a trip that descends does not
    // pop), every group's lanes run the visit (a group with nothing to visit
    // masks its result), and only the leaf passes sit behind a wave-uniform
    // branch.  The old form's per-group branches cost the lone heavy wave
    // ~40 exec-mask and branch instructions per trip (c4_coop_phase_n8_spread.log).
    // (G = 8, nearest hits: t / bpos are the lane's own best -- reduced to
    // the group's culling limit tg once per leaf section and to the result
    // once per query instead of per leaf: N = 8 / 4 shares -2 to -3 %)
    constexpr bool LOC = G == 8;
    float tg = LOC ? grp_min<G>(t) : t;
    unsigned pl = 0u;                           // the previous trip's crossed leaves (of node pn), pending
    int pn = 0;
    while (true) {
        const bool has = m != 0;
        const int p = __builtin_ctz(m | 256u);
        const unsigned mr = cur < 0 ? 0u : (m & (m - 1u));
        const int cwl = (int)Lw[max(cur, 0) * WIDE_WORDS + 8 + ((p & 7) ^ oct)];
        const unsigned e2 = my[64 * max(sp - 1, 0)];
        const int cw = cur < 0 ? 0 : cwl;
        bool occl = false;
        const bool rootleaf = has && cw < 0;    // (a root leaf: child leaves are tested at their parent)
        if (wave_any(rootleaf)) {
            if (rootleaf) {
                const int lf = ~cw;
                const int fa[1] = {lf & 0xffffff}, ca[1] = {lf >> 24};
                occl = leaf_coop<COUNT, G, 1, LOC>(B, r, shadow, maxt, fa, ca, pos, gbase, t, bpos, id);
            }
            if (LOC) tg = grp_min<G>(t);
        }
        const bool vis = has && cw >= 0;
        const int cv = vis ? cw : 0;
        unsigned lm;
        unsigned hm = COUNT ? wide_visit_coop<G>(L + 7 * cv, r, wr, shadow ? maxt : (LOC ? tg : t), pos, gbase, lm,
                                                 Lmax + 8 * cv, shadow ? id : -1)
                            : wide_visit_coop<G>(L + 7 * cv, r, wr, shadow ? maxt : (LOC ? tg : t), pos, gbase, lm);
        hm = vis ? hm : 0u;
        lm = vis ? lm : 0u;
        // A trip's crossed leaves wait one trip, so one leaf section serves
        // two trips' leaves of every group: the lone heavy wave of an N = 8
        // share runs half as many leaf sections (~50 % of its chain).  Exact:
        // the nearest hit is order-independent; the culling limit tg lags
        // one trip.  N = 8 shares 9.8-10.1 -> 9.3-9.65 ms, N = 4 13.6-14.2
        // -> 13.0-13.5 ms (profiles/r06/c4_coop_defer_ab.log).
        bool run = wave_any(pl != 0);
        if (!run && wave_any(lm != 0)) {
            pl = lm;
            pn = cv;
        } else if (run) {
            SPT_TRACE(const unsigned long long tr_l0 = __builtin_amdgcn_s_memtime(); W.tr_leafruns++;)
            occl = coop_leaves<COUNT, G, LOC>(B, r, shadow, maxt, Lw, oct, pn, pl, cv, lm, pos, gbase, t, bpos, id) || occl;
            pl = 0u;
            if (LOC) tg = grp_min<G>(t);
            SPT_TRACE(W.tr_leaf += (unsigned)(__builtin_amdgcn_s_memtime() - tr_l0);)
        }
        const unsigned nm = hm & ~lm;
        const bool desc = vis && nm != 0 && !occl;
        if (desc && mr != 0) my[64 * sp] = ((unsigned)cur << 8) | mr;
        sp = occl ? 0 : sp + ((desc && mr != 0) ? 1 : 0);
        cur = desc ? cw : cur;
        m = occl ? 0u : (desc ? nm : mr);
        const bool pop = m == 0 && sp > 0;      // (then no push this trip: e2 is the top)
        sp -= pop ? 1 : 0;
        cur = pop ? (int)(e2 >> 8) : cur;
        m = pop ? (e2 & 255u) : m;
        trips++;
        const unsigned long long am = __builtin_amdgcn_ballot_w64(m != 0);
        if (am == 0 || trips >= budget || 64 * __builtin_popcountll(am) <= stop * n0) {
            if (wave_any(pl != 0)) {                    // (no leaf is left pending past the call)
                if (coop_leaves<COUNT, G, LOC>(B, r, shadow, maxt, Lw, oct, pn, pl, 0, 0u, pos, gbase, t, bpos, id)) {
                    m = 0u;
                    sp = 0;
                }
            }
            break;
        }
    }
    if (LOC && m == 0 && !shadow) {
        // the group's result from its lanes' bests: the minimum distance,
        // ties to the highest reference index (bpos -1: the query's first id)
        const float tf = grp_min<G>(t);
        const bool cand = t == tf;
        int wb;
        if (__builtin_popcount(grp_bits<G>(cand, gbase)) <= 1) {
            wb = grp_max<G>(cand ? bpos : -1);
        } else {
            const int cid = cand ? (bpos >= 0 ? B.id[bpos] : id) : (int)0x80000000;
            const int im = grp_max<G>(cid);
            wb = grp_max<G>((cand && cid == im) ? bpos : -1);
        }
        t = tf;
        bpos = wb;
    }
    SPT_TRACE(W.tr_trips += trips;)
    const bool done = m == 0;
    if (done && bpos >= 0) id = (!COUNT && shadow) ? 0x7fffffff : B.id[bpos];
    W.t = t;
    W.id = id;
    W.bpos = bpos;
    W.node = cur;
    W.m = m;
    W.sp = sp;
    return done;
}

#endif  // SPT_WALK_H
