// smallpt.hip -- gfx950 kernel for the Monte-Carlo hot path of smallptgpu-v1.6.
//
// Computes what nsamples successive UpdateRenderingCPU passes
// (smallptCPU.cpp:77-132) compute: per pixel a camera ray from the pixel's
// own MWC RNG (simplernd.h:34-48), RadiancePathTracing (geomfunc.h:167-338)
// or RadianceDirectLighting (:340-483), the running average into the
// flipped colour slot (smallptCPU.cpp:110-118) and the toInt pack
// (vec.h:62, smallptCPU.cpp:120-122).  Results match the CPU path bit for bit
// (the float ops are the reference's, in its order; glibc sinf/cosf/powf are
// reproduced by rt_glibc_math.h), well inside the 1e-4 HDR tolerance.
//
// Mapping (MI355X-first, not a port of rendering_kernel.cl):
//   * one lane per pixel, a wave per 8x8 tile (launch_shape: 4 or 16 waves
//     per block, a block's waves spread over the row window);
//   * ALL samples of a launch run in-lane with path regeneration: the per-
//     lane loop advances one bounce per iteration and a lane whose path ended
//     immediately starts its next sample, so a wave's cost is the max over
//     lanes of the total bounces of nsamples paths (~ the mean for spp >> 1),
//     not the sum over samples of the per-sample max;
//   * RNG state and the path state stay in VGPRs for the whole launch, the
//     colour accumulator (touched once per sample) in a lane-private LDS
//     area: HBM traffic is 32 B per pixel per launch, whatever nsamples is;
//   * spheres are staged once per block into LDS as SoA float4 (centre,
//     rad^2) + material records and read with wave-uniform indices (LDS
//     broadcast); scenes larger than the LDS budget are read from global
//     memory through the same wave-uniform loop (L2/scalar-cache resident).
#include "rt_common.h"
#include "rt_glibc_math.h"
#include "spt_policy.h"
#include "spt_layout.h"
#include "spt_accept.h"
#include "spt_rng.h"

namespace rt {
namespace smallpt {

using namespace sptlayout;               // the kernel families, variant predicates and LDS layout
namespace acc = sptaccept;               // the integer accept tests of query_bf / shadow_bf
constexpr float EPS = acc::EPS;          // geom.h:29
constexpr float PI_F = 3.14159265358979323846f;
constexpr int DIFF = 0, SPEC = 1;   // REFR = 2 is the remaining case
#ifndef RT_SPT_QUNROLL
#define RT_SPT_QUNROLL 3
#endif

struct SphereGeo { float4 g; };          // centre.xyz, rad*rad (same float product as :42)

// GetRandom, simplernd.h:34-48, returning f = the float in [2, 4) that the
// reference maps to (f - 2) / 2.  Callers finish with fma(f, .5, c): for
// c = -1 that is (f - 2) / 2 and for c = -1.5 it is (f - 2) / 2 - .5f, exact
// (f / 2 - 1 and f / 2 - 1.5 are representable, as are the reference's two
// steps each), in one op instead of two or three.
// (the two stream updates: spt_rng.h, two VALU each)
__device__ __forceinline__ float get_random_f(uint32_t &s0, uint32_t &s1)
{
    return __uint_as_float(sptrng::draw<true>(s0, s1));
}
__device__ __forceinline__ float get_random(uint32_t &s0, uint32_t &s1)
{
    return __builtin_fmaf(get_random_f(s0, s1), .5f, -1.f);
}

__device__ __forceinline__ float vdot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ v3 vsmul(float k, v3 b) { return mk(k * b.x, k * b.y, k * b.z); }
__device__ __forceinline__ v3 vadd(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 vsub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 vmul(v3 a, v3 b) { return mk(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ v3 vnorm(v3 v) { const float l = inv_len(vdot(v, v)); return vsmul(l, v); }
__device__ __forceinline__ v3 vxcross(v3 a, v3 b)
{
    return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x);
}

// SphereIntersect, geomfunc.h:32-59 (g = centre.xyz, rad*rad), except that a
// miss returns +inf instead of 0: every caller tests "d != 0 && d < t" with a
// finite t, which for +inf is the single test "d < t".  The early return on
// det < 0 is kept as a branch: when no lane of the wave reaches the sphere's
// line the square root is skipped (measured +8 % over a branch-free select
// form).  NaN det is a miss, as in the reference.
constexpr float MISS = __builtin_inff();
__device__ __forceinline__ float sphere_hit(float4 g, const ray3 &r)
{
    const float opx = g.x - r.o.x, opy = g.y - r.o.y, opz = g.z - r.o.z;
    const float b = opx * r.d.x + opy * r.d.y + opz * r.d.z;
    const float det = b * b - (opx * opx + opy * opy + opz * opz) + g.w;
    if (det < 0.f) return MISS;
    const float sd = sqrt_exact(det);
    const float t1 = b - sd, t2 = b + sd;
    return t1 > EPS ? t1 : (t2 > EPS ? t2 : MISS);
}

// Sphere geometry for the nearest-hit / any-hit loops: LDS (per-block copy)
// or global-memory float4 array (scenes above MAX_LDS_BYTES), runtime count.
struct DynGeo {
    const float4 *g;
    int n;
    __device__ __forceinline__ int count() const { return n; }
    __device__ __forceinline__ float4 at(int i) const { return g[i]; }
};

struct Scene {                // per-block LDS copy (or global view for big scenes)
    const float4 *geo;        // centre, rad^2 (per-lane lookups of the hit sphere)
    const float4 *emi;        // emission.xyz, refl (as int bits)
    const float4 *col;        // colour.xyz, rad
    const float4 *lrec;       // per light (!viszero(e), ascending index): geo, col, emi
    int n, nlights;
};

// One ray query over the spheres, i descending, update iff d != 0 && d < t.
// With t = 1e20f on entry this is Intersect (geomfunc.h:71-92: nearest hit,
// highest index wins ties); with t = maxt on entry "some update happened" is
// IntersectP (:94-110: any d != 0 && d < maxt), and the first update is at
// the index where IntersectP's early exit stops (kept for the test counter).
// Returns the last updated index, -1 if none.
template <bool COUNT, class G>
__device__ __forceinline__ int query(const G &geo, const ray3 &r, float &t, int &first)
{
    int id = -1;
#pragma unroll 1
    for (int i = geo.count() - 1; i >= 0; i--) {
        const float d = sphere_hit(geo.at(i), r);
        const bool take = d < t;                           // d != 0 && d < t (miss = +inf)
        t = take ? d : t;
        id = take ? i : id;
        if (COUNT) first = (first < 0 && take) ? i : first;
    }
    return id;
}

// The same query with a branch-free sphere test and the next sphere's record
// loaded while the current one is tested (one LDS / scalar-load latency per
// query instead of one per sphere).  sqrt_nr is exact for det in [2^-96,
// inf); for det < 0 or NaN it returns NaN, and NaN roots are no candidates --
// the reference's miss; for det = +inf it returns NaN where sqrtf returns
// +inf, whose root b + inf is never "< t" for the finite t of every caller --
// a miss either way.  Only |det| < 2^-96 (where sqrt_nr is not sqrtf, e.g.
// det = +-0) is unsafe: any lane that meets one in the whole query has the
// wave redo the query with the exact per-sphere test.
//
// The accept tests run on integer keys (spt_accept.h): the bound is kept as a
// limit key, a sphere's two roots and the bound fold into one unsigned three-
// way minimum, "taken" is "the bound moved" (strict: a tie keeps the earlier,
// higher index), and the distance is rebuilt from the bound once, after the
// loop.  A t_in <= EPS or NaN accepts nothing and comes back unchanged.
//
// The loops are unrolled by hand -- trips of RT_SPT_QUNROLL spheres, then the
// rest one by one -- because the compiler does not unroll a loop of unknown
// length around the three-way minimum's instruction.  The |det| guard is one
// minimum over the trip's spheres and one compare per trip.
constexpr float DET_SAFE = 0x1p-96f;
template <class G, class F, class T>
__device__ __forceinline__ bool for_spheres_bf(const G &geo, const ray3 &r, F &&accept, T &&trip)
{
    // trip(k) before each run of k spheres, then accept(i, after, t1, t2) for
    // i descending, `after` = the run's spheres still to come behind i (a
    // constant once unrolled); true iff some |det| < DET_SAFE
    const auto roots = [&](int i, float &t1, float &t2) {
        const float4 g = geo.at(i);
        const float opx = g.x - r.o.x, opy = g.y - r.o.y, opz = g.z - r.o.z;
        const float b = opx * r.d.x + opy * r.d.y + opz * r.d.z;
        const float det = b * b - (opx * opx + opy * opy + opz * opz) + g.w;
        const float sd = sqrt_nr(det);
        t1 = b - sd;
        t2 = b + sd;
        return fabsf(det);
    };
    bool bad = false;
    int i = geo.count() - 1;
#pragma unroll 1
    for (; i >= RT_SPT_QUNROLL - 1; i -= RT_SPT_QUNROLL) {
        float t1[RT_SPT_QUNROLL], t2[RT_SPT_QUNROLL];
        float m = roots(i, t1[0], t2[0]);
#pragma unroll
        for (int j = 1; j < RT_SPT_QUNROLL; j++) m = __builtin_fminf(m, roots(i - j, t1[j], t2[j]));
        trip(RT_SPT_QUNROLL);
#pragma unroll
        for (int j = 0; j < RT_SPT_QUNROLL; j++) accept(i - j, RT_SPT_QUNROLL - 1 - j, t1[j], t2[j]);
        bad = bad || m < DET_SAFE;
    }
#pragma unroll 1
    for (; i >= 0; i--) {
        float t1, t2;
        bad = bad || roots(i, t1, t2) < DET_SAFE;
        trip(1);
        accept(i, 0, t1, t2);
    }
    return bad;
}

// Returns the last updated index, negative if none.  KEYED (spt_layout.h
// key_accept): false keeps the float form of the accept tests for the two
// variants that the keyed form costs registers.
// Uncounted, the keyed form does not select the loop's index (a scalar: one
// v_mov per sphere to make it selectable) but counts the spheres that follow
// the taken one: `since` grows by a trip's length before the trip and is set
// to the constant `after` by the sphere that is taken.  The loop ends at
// index 0, so the count is the index; untaken, it stays negative.
template <bool COUNT, bool KEYED, class G>
__device__ __forceinline__ int query_bf(const G &geo, const ray3 &r, float &t, int &first)
{
    const float t_in = t;
    int id = -1;
    bool bad = false;
    if constexpr (KEYED && COUNT) {
        uint32_t tb = acc::limit_key(t_in);
        bad = for_spheres_bf(geo, r, [&](int i, int, float t1, float t2) {
            const bool take = acc::nearest_accept(tb, t1, t2);
            id = take ? i : id;
            first = (first < 0 && take) ? i : first;
        }, [](int) {});
        t = acc::nearest_result(tb, t_in);
    } else if constexpr (KEYED) {
        uint32_t tb = acc::limit_key(t_in);
        int since = -(1 << 30);
        bad = for_spheres_bf(geo, r, [&](int, int after, float t1, float t2) {
            since = acc::nearest_accept(tb, t1, t2) ? after : since;
        }, [&](int k) { since += k; });
        id = since;
        t = acc::nearest_result(tb, t_in);
    } else {
#pragma unroll RT_SPT_QUNROLL
        for (int i = geo.count() - 1; i >= 0; i--) {
            const float4 g = geo.at(i);
            const float opx = g.x - r.o.x, opy = g.y - r.o.y, opz = g.z - r.o.z;
            const float b = opx * r.d.x + opy * r.d.y + opz * r.d.z;
            const float det = b * b - (opx * opx + opy * opy + opz * opz) + g.w;
            bad = bad || fabsf(det) < DET_SAFE;
            const float sd = sqrt_nr(det);
            const float t1 = b - sd, t2 = b + sd;
            // SphereIntersect's distance is t1 if t1 > EPS, else t2 if t2 > EPS,
            // else a miss: d = t1 > EPS ? t1 : t2, taken iff d > EPS && d < t
            // (false for NaN) -- one select fewer than materialising the miss.
            const float d = t1 > EPS ? t1 : t2;
            const bool take = d > EPS && d < t;
            t = take ? d : t;
            id = take ? i : id;
            if (COUNT) first = (first < 0 && take) ? i : first;
        }
    }
    if (wave_any(bad)) {
        t = t_in;
        first = -1;
        id = query<COUNT>(geo, r, t, first);
    }
    return id;
}

// Two queries in one pass over the spheres (single-light scenes, see
// render_kernel<..., DUAL>): the path ray's nearest hit (t = 1e20f on entry,
// as query_bf) and, for lanes with sh set, the pending shadow ray's any hit
// (ts = maxt on entry; "some update happened" = IntersectP true, the first
// update = its early-exit index for the test counter).  Each sphere record
// is loaded once for both rays, and the two dependency chains interleave.
// Uncounted, the shadow ray only needs "some distance in (EPS, maxt)"
// (geomfunc.h:94-110 with a fixed maxt): an occluded flag, not a running
// minimum and index -- three VALU operations fewer per sphere.
template <bool COUNT, class G>
__device__ __forceinline__ void query2_bf(const G &geo, const ray3 &r, float &t, int &id, const ray3 &rs, bool sh,
                                          float &ts, int &ids, int &firsts)
{
    const float t_in = t, ts_in = ts;
    int first = -1;
    id = -1;
    ids = -1;
    bool bad = false, occ = false;
#pragma unroll RT_SPT_QUNROLL
    for (int i = geo.count() - 1; i >= 0; i--) {
        const float4 g = geo.at(i);
        {
            const float opx = g.x - r.o.x, opy = g.y - r.o.y, opz = g.z - r.o.z;
            const float b = opx * r.d.x + opy * r.d.y + opz * r.d.z;
            const float det = b * b - (opx * opx + opy * opy + opz * opz) + g.w;
            bad = bad || fabsf(det) < 0x1p-96f;
            const float sd = sqrt_nr(det);
            const float t1 = b - sd, t2 = b + sd;
            const float d = t1 > EPS ? t1 : t2;          // (query_bf: taken iff d > EPS && d < t)
            const bool take = d > EPS && d < t;
            t = take ? d : t;
            id = take ? i : id;
        }
        {
            const float opx = g.x - rs.o.x, opy = g.y - rs.o.y, opz = g.z - rs.o.z;
            const float b = opx * rs.d.x + opy * rs.d.y + opz * rs.d.z;
            const float det = b * b - (opx * opx + opy * opy + opz * opz) + g.w;
            bad = bad || (sh && fabsf(det) < 0x1p-96f);
            const float sd = sqrt_nr(det);
            const float t1 = b - sd, t2 = b + sd;
            const float d = t1 > EPS ? t1 : t2;
            const bool take = d > EPS && d < ts;
            if (COUNT) {
                ts = take ? d : ts;
                ids = take ? i : ids;
                firsts = (firsts < 0 && take) ? i : firsts;
            } else {
                occ = occ || take;
            }
        }
    }
    if (!COUNT) ids = occ ? 0 : -1;
    if (wave_any(bad)) {
        t = t_in;
        id = query<COUNT>(geo, r, t, first);
        ts = ts_in;
        firsts = -1;
        ids = query<COUNT>(geo, rs, ts, firsts);
    }
}

// One shadow ray's any-hit query (IntersectP, geomfunc.h:94-110) for lanes
// with `have` set: query2_bf's uncounted shadow half on its own -- the same
// test, an occluded flag, and the wave's redo with the exact query when a lane
// that holds a ray meets |det| < 2^-96.  (Lanes without a ray run the loop on
// whatever their registers hold; their result is discarded.)
template <class G>
__device__ __forceinline__ bool shadow_bf(const G &geo, const ray3 &rs, float maxt, bool have)
{
    // (spt_accept.h: the minimum key over every sphere's roots, then one
    // compare against maxt's limit key -- 0, nothing passes, for maxt <= EPS)
    uint32_t near = acc::KEY_NONE;
    const bool bad = for_spheres_bf(geo, rs, [&](int, int, float t1, float t2) { acc::any_accept(near, t1, t2); }, [](int) {});
    bool occ = acc::any_result(near, maxt);
    if (wave_any(have && bad)) {
        float ts = maxt;
        int first = -1;
        occ = query<false>(geo, rs, ts, first) >= 0;
    }
    return occ;
}

// shadow_bf for a flush pass: the lane mask of the rays that reached the
// light (have && !occluded).  The two ballots are of compares, so the mask
// stays in scalar registers; ballot(have && !occ) of the merged flags went
// through a VGPR and back.
template <class G>
__device__ __forceinline__ unsigned long long shadow_bf_unocc(const G &geo, const ray3 &rs, float maxt, bool have)
{
    uint32_t near = acc::KEY_NONE;
    const bool bad = for_spheres_bf(geo, rs, [&](int, int, float t1, float t2) { acc::any_accept(near, t1, t2); }, [](int) {});
    const unsigned long long hm = __builtin_amdgcn_ballot_w64(have);
    // (the limit key behind an opaque copy: folded into the compare, its
    // select becomes an AND of two compares, which is no compare to a ballot)
    uint32_t lim = acc::limit_key(maxt);
    asm volatile("" : "+v"(lim));
    unsigned long long un = hm & ~__builtin_amdgcn_ballot_w64(near < lim);
    if (wave_any(have && bad)) {
        float ts = maxt;
        int first = -1;
        un = hm & __builtin_amdgcn_ballot_w64(query<false>(geo, rs, ts, first) < 0);
    }
    return un;
}

// ---------------------------------------------------------------------------
// The sphere hierarchy's device code for large scenes -- BvhView, the binary
// walk, the 8-wide walk in LDS and its cooperative form -- stands here, inside
// this namespace: it uses the helpers above and render_kernel below uses it.
#include "spt_walk.h"

// Per-lane work counters: calls and samples in 32 bits (a lane adds a few per
// sample; render_kernel flushes a lane's calls with an atomic before they
// could wrap), sphere tests in 64.  Four VGPRs fewer than four u64 words.
struct Counts { unsigned isect, isectp, samples; unsigned long long tests; };

// Tools-only block profile (build with -DRT_SPT_PROF; tools/ab.py PROF=1):
// per code block, the lanes that executed it and the wave-executions
// (iterations in which at least one lane of the wave did).  Never in the
// product build.
#ifdef RT_SPT_PROF
enum { PB_ITER, PB_SHADOW, PB_NEAREST, PB_DIFF, PB_SPEC, PB_REFR, PB_LIGHT, PB_BOUNCE, PB_DONE,
       PB_WCALL, PB_WSTEP, PB_WLEAF, PB_WSHADE, PB_FLUSH,
       // flush passes by what started them (the first that holds, in this order):
       // the threshold, a DIFF hit with no free slot, a sample ending behind a
       // parked one, an emitter term behind an unresolved entry, the drain
       PB_FL_THRESH, PB_FL_SLOT, PB_FL_ENDS, PB_FL_EMIT, PB_FL_DRAIN,
       // the owners' step of a flush pass: entries resolved / passes with one,
       // lanes and passes that fold a parked sample, lanes that resolve one entry / two
       PB_OW_ROUND, PB_OW_FOLD, PB_OW_ONE, PB_OW_TWO, PB_N };
__device__ unsigned long long g_spt_prof[2 * PB_N];
#define SPT_PROF(b)                                                                        \
    do {                                                                                   \
        prof_l[b]++;                                                                       \
        if ((int)(threadIdx.x & 63) == __builtin_ctzll(__builtin_amdgcn_read_exec())) prof_w[b]++; \
    } while (0)
#else
#define SPT_PROF(b) do {} while (0)
#endif

// Tools-only wave timeline (build with -DRT_SPT_TRACE): per wave of the grid
// {start, end} (s_memrealtime, 100 MHz), HW_ID, XCC_ID and {sum, max} over
// its lanes of the loop iterations, at g_spt_trace[4 * (linear block * 4 +
// wave) + 0/1].  Never in the product build.
// Phase stamps (s_memtime, shader clock), hierarchy kernels: per wave, the
// max over its lanes of the cycles spent in the walk (bvh_begin + bvh_walk),
// of those in leaf blocks, walk trips, leaf-block passes and queries; at
// g_spt_trace[4 * wave + 2/3].  g_spt_only_group >= 0 renders only that tile
// group (the other waves exit at once): the group's waves run alone on the
// chip, which splits contention from latency.
#ifdef RT_SPT_TRACE
__device__ uint4 *g_spt_trace;
__device__ int g_spt_only_group = -1;
#endif

// toInt, vec.h:62 (clamp macro keeps -0.0; glibc powf via rt_glibc_math.h).
// A NaN accumulator (an inf emitter channel times a zero throughput) passes
// the clamp and powf: the reference's x86 conversion makes it INT_MIN.
__device__ __forceinline__ int to_int(float x)
{
    const float c = (x < 0.f) ? 0.f : ((x > 1.f) ? 1.f : x);
    return rt::cvt_i32_x86(rtm::powf(c, 1.f / 2.2f) * 255.f + .5f);
}
// A pixel, smallptCPU.cpp:120-122 (the shifts in 32 bits, as x86 shifts INT_MIN).
__device__ __forceinline__ uint32_t pack_rgb(float r, float g, float b)
{
    return (uint32_t)to_int(r) | ((uint32_t)to_int(g) << 8) | ((uint32_t)to_int(b) << 16);
}

// DUAL (path tracing, full-scan geometry, scenes with exactly one light): a
// DIFF vertex builds its light sample's shadow ray AND its bounce ray in the
// same iteration -- SampleLights' draws do not depend on the shadow test, so
// the bounce's draws follow them in the reference's order either way -- and
// the next iteration queries both (query2_bf) and applies the shadow result
// (rad += thr * Ld, geomfunc.h:229-230) before it shades the bounce's hit.
// One iteration per path vertex instead of two for a lit DIFF vertex.
// The uncounted form (no COUNT, no RAYS) goes further: the shadow ray is not
// traced by the lane that built it nor in the next iteration, but from a
// per-wave ring by whichever lane pops it (DQ, in the kernel).
// COUNT: all four counters (the sphere-test count needs IntersectP's early-
// exit position, so a counted shadow query finds the highest-index
// occluder).  RAYS (SPT_COUNT_RAYS): Intersect / IntersectP calls and samples
// only, with the uncounted queries (any occluder ends a shadow query).
// CG (8-wide kernels): lanes per pixel of the cooperative walk this kernel
// carries (8 or 4), or 0 -- no cooperative code (windows without a
// cooperative tier: the full frame, N = 2 shares).
template <bool DL, bool COUNT, int GEO, bool DUAL = false, bool RAYS = false, int CG = 0>
__global__ void __launch_bounds__(1024, variant_of(GEO, DL, DUAL, COUNT, RAYS, CG).min_waves())
render_kernel(const rt_sphere *__restrict__ spheres, int nspheres, rt_camera cam,
              float *__restrict__ colors, const uint32_t *seeds_in,
              uint32_t *seeds_out, uint32_t *__restrict__ pixels, int w, int h,
              int row_begin, int row_end, int tiles_x, int ntiles, int nslots, int gstride, int first_sample,
              int nsamples, int prio_sched, const int *__restrict__ group_order, unsigned *__restrict__ group_cost,
              const float4 *__restrict__ g_geo, const float4 *__restrict__ g_emi,
              const float4 *__restrict__ g_col, const float4 *__restrict__ g_lrec, int nlights,
              BvhView bvh, unsigned long long *__restrict__ counters, int *__restrict__ work, int split,
              int nheavy, int sflags)
{
    // The variant (spt_layout.h): its predicates here are the ones launch()
    // sizes the dynamic LDS by, and every LDS offset below is that header's.
    constexpr Variant V = variant_of(GEO, DL, DUAL, COUNT, RAYS, CG);
    constexpr bool LDS = V.lds();
    // GEO_WIDE: persistent waves -- each wave takes 8x8 tiles from a work
    // counter (in the adaptive order's slot sequence, heaviest groups first)
    // until the window is done, so a block's LDS copy of the hierarchy is
    // made once and a CU never idles behind one block's slowest wave.
    constexpr bool PERSIST = V.persist();
    // PARK (full-scan kernels): state that is touched once per sample or
    // once per pass B, not in the sphere loop, lives in LDS after the scene
    // copy instead of in registers.  The running-average colour sits in the
    // wave's lane-private slots (only the lane itself ever reads or writes
    // its dwords, so no barrier is needed); the camera terms sit once per
    // block before them.  Arithmetic, draws and stores are unchanged.
    constexpr bool PARK = V.park();
    // DQ (the uncounted two-query kernels): the shadow rays are deferred.  A
    // lit DIFF vertex pushes its shadow ray (origin, direction, maxt) into a
    // wave-private FIFO ring in LDS and keeps the contribution c = thr * (e *
    // s) it would add -- the same two products on the same thr that the lock-
    // step form computes one iteration later -- and the path query is the one-
    // ray query_bf.  A flush pass (all 64 lanes pop the oldest min(count, 64)
    // entries, one each, and run the any-hit loop; the result is one ballot,
    // an owner reads the bit at its entry's distance from the head) runs when
    // the ring holds the threshold T (spt_policy.h, sq=T) or an order demands
    // it.  Exactness is the order of the float additions: a sample's rad
    // receives its terms in vertex order, and the running average receives
    // samples in sample order.  A lane's entries resolve in push order (FIFO),
    // so its shadow terms stay ordered among themselves; a flush is forced
    // (wave_any, before the dependent operation) when a lane
    //   * is about to add an emitter term to a sample with a pending term,
    //   * is about to end a sample while its previous sample is unfolded (a
    //     sample that ends with terms pending parks its rad in LDS and is
    //     folded into the average when the last of them resolves),
    //   * is about to push with both its pending slots taken (one in
    //     registers, one in LDS), or
    //   * when no lane has a sample left: the drain that ends the wave's loop.
    // Every lane of the wave stays in the loop until then (a lane out of
    // samples, or past the frame's edge, idles but still pops entries).
    constexpr bool DQ = V.dq();
    constexpr int WAVE_DW = wave_dwords(DQ);
    constexpr int SQ_RING = RING_FIELD_DW;
    // Dynamic LDS (spt_layout.h): LDS: the scene copy; PARK: then the parking
    // area -- its head, and WAVE_DW dwords per wave of the block.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int park_off = park_offset(V, nspheres, nlights);
    // The lane's parking address -- head, wave x WAVE_DW, lane -- and its
    // wave's ring base do not change during a launch.  HELD variants state
    // them as plain expressions of the thread index: the compiler computes
    // them once per wave, before the pixel loop, and keeps the lane's address
    // in a register for the whole launch, the ring base derived from it (at
    // occupancy 7 the two-query kernel has that register: 70 -> 71 of 72
    // VGPRs).  Rebuilt at every use they cost six VALU instructions a time in
    // blocks that run with few lanes active.  (Stated this way, not through
    // a variable of their own, the hierarchy kernels -- which have no parked
    // state -- compile to the instructions they had; a wave-uniform ring base
    // in a scalar register cost nine more scalar spills.)
    // Not HELD (spt_layout.h names the variants that have no register to
    // spare): the thread index is re-read behind an empty asm at every use,
    // which keeps the address from being hoisted out of the loop.
    constexpr bool HELD = V.held_addr();
    const auto park_ptr = [&]() {
        int t = (int)threadIdx.x;
        if constexpr (!HELD) asm volatile("" : "+v"(t));
        return (float *)(smem + park_off + PARK_HEAD_BYTES) + (t >> 6) * WAVE_DW + (t & 63);
    };
    // DQ (always HELD): the wave's ring, field f of entry e at [f * SQ_RING + e]
    const auto ring_ptr = [&]() {
        const int t = (int)threadIdx.x;
        return (float *)(smem + park_off + PARK_HEAD_BYTES) + (t >> 6) * WAVE_DW + RING_BASE_DW;
    };
    // The camera terms of pass B (twelve floats, with 1 / w and 1 / h) head
    // the parking area: read there by every lane at one address (broadcast)
    // instead of being held in fourteen scalar registers for the whole loop.
    if (PARK && threadIdx.x == 0) {
        float4 *pc = (float4 *)(smem + park_off);
        pc[0] = make_float4(cam.x.x, cam.x.y, cam.x.z, 1.f / w);           // smallptCPU.cpp:80-81
        pc[1] = make_float4(cam.y.x, cam.y.y, cam.y.z, 1.f / h);
        pc[2] = make_float4(cam.dir.x, cam.dir.y, cam.dir.z, 0.f);
        pc[3] = make_float4(cam.orig.x, cam.orig.y, cam.orig.z, 0.f);
    }
    if (PARK && !LDS) __syncthreads();
    Scene S;
    if (LDS) {
        float4 *s = (float4 *)smem;
        const int nrec = scene_records(nspheres, nlights);
        for (int i = threadIdx.x; i < nrec; i += blockDim.x) s[i] = g_geo[i];
        __syncthreads();
        S.geo = s; S.emi = s + nspheres; S.col = s + 2 * nspheres; S.lrec = s + 3 * nspheres;
    } else {
        S.geo = g_geo; S.emi = g_emi; S.col = g_col; S.lrec = g_lrec;
    }
    S.nlights = nlights;
    S.n = nspheres;
    const DynGeo geo{S.geo, S.n};
    // GEO_WIDE (spt_layout.h): the wide nodes, then per wave of the block its
    // lanes' stacks.
    const uint4 *wL = (const uint4 *)smem;
    unsigned *wstk = nullptr;
    if (GEO == GEO_WIDE) {
        uint4 *d = (uint4 *)smem;
        for (int i = threadIdx.x; i < 7 * bvh.wnodes; i += blockDim.x) d[i] = bvh.wnode[i];
        if (COUNT)
            for (int i = threadIdx.x; i < 2 * bvh.wnodes; i += blockDim.x) d[7 * bvh.wnodes + i] = bvh.wmax[i];
        wstk = (unsigned *)(smem + wide_stack_offset(bvh.wnodes, COUNT)) +
               (size_t)(threadIdx.x >> 6) * WIDE_LEVEL_DW * (bvh.wdepth - 1);
        __syncthreads();
    }

    // 8x8 pixel tiles of the row window, one per wave, in groups of four
    // side by side (a 32x8 strip: whole 128-B lines of the seed, colour and
    // pixel rows, so no line is fetched by two XCDs); group j of block b is
    // j * gridDim.x + b, so the groups of a 16-wave block sample the whole
    // window (per-CU work evens out when one block fills a CU).
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // group_order (optional): dispatch slot -> group, heaviest groups of the
    // previous launch first (host: adaptive schedule); results do not depend
    // on it.
    // Compiled into the hierarchy kernels only: in the full-scan kernels
    // (Cornell) the order/cost plumbing cost 1.4 % of the frame and 8 % of an
    // N = 8 band (measured A/B) although it is never used there.
    constexpr bool SCHED = V.sched();
    constexpr bool CALLS = COUNT || RAYS;           // the call / sample counters are kept
    Counts cnt = {0, 0, 0, 0};
    SPT_PROF_ONLY(unsigned prof_l[PB_N] = {}, prof_w[PB_N] = {};)
    // Work item: tile (item & 3) of dispatch slot item >> 2.  Static launches:
    // one item per wave, slot (wave >> 2) * gridDim.x + blockIdx.x.
    // Persistent launches fetch work indices f: the first nheavy items in
    // dispatch order (the heaviest, with a learnt order) as 2^hs sub-items of
    // 64 >> hs pixels each (lanes beyond them idle: a heavy tile's pixels run
    // on several SIMDs), f = (nheavy << hs) + ... the rest whole.
    // (the packed words split, nheavy, sflags and prio_sched: spt_policy.h)
    const int hs = PERSIST ? sptpolicy::split_hs(split) : 0;
    // waves of a block that take tier-1 sub-items first (0: 4 << hs)
    const int hw = sptpolicy::split_hw(split) ? sptpolicy::split_hw(split) : (4 << hs);
    const int nitems = 4 * nslots;
    // Three tiers, in dispatch order (heaviest first with a learnt order):
    // n1 tiles split into 2^hs sub-items each (the cooperative walk with
    // split's coop bit), n2 tiles routed one per SIMD, then the rest.
    const int n1 = PERSIST ? min(sptpolicy::nheavy_n1(nheavy), nitems) : 0;
    const int n2 = PERSIST ? min(sptpolicy::nheavy_n2(nheavy), nitems - n1) : 0;
    const int nwork = (n1 << hs) + (nitems - n1);
    // Persistent fetch: waves 0..hw - 1 of a block take tier-1 sub-items
    // first (work[2]); waves 0..3 -- one per SIMD -- then take tier-2 tiles
    // (work[1]): a heavy tile's SIMD shares its issue slots with lighter,
    // lower-priority waves instead of with three other heavy tiles; every
    // wave then takes the rest in order (work[0]).
    // (by the wave's first active lane: refill claims fetch from inside the
    // pixel loop, where lanes that ran out of work have left)
    // (below: the first min(hw, waves per block) x #blocks tier-1 sub-items are assigned statically)
    const int nstatic = PERSIST ? min(min(hw, (int)(blockDim.x >> 6)) * (int)gridDim.x, n1 << hs) : 0;
    const auto fetch = [&]() {
        int v = 0;
        if (lane == __builtin_ctzll(__builtin_amdgcn_read_exec())) {
            v = -1;
            if (wave < hw && n1 > 0) {
                const int hv = atomicAdd(work + 2, 1) + nstatic;
                if (hv < (n1 << hs)) v = hv;
            }
            if (v < 0 && wave < 4 && n2 > 0) {
                const int hv = atomicAdd(work + 1, 1);
                if (hv < n2) v = (n1 << hs) + hv;
            }
            if (v < 0) v = (n1 << hs) + n2 + atomicAdd(work, 1);
        }
        return __builtin_amdgcn_readfirstlane(v);
    };
    int f = ((wave >> 2) * (int)gridDim.x + (int)blockIdx.x) * 4 + (wave & 3);
    if (PERSIST) {
        // The first tier-1 sub-item of wave w of block b is
        // w * #blocks + b, not the next one a shared counter hands out: the
        // heaviest tiles' sub-items (dispatch order) land one per CU, beside
        // lighter ones on their SIMD, where the counter gave a whole heavy
        // tile's rows to the waves of the first block to start.
        const int fs = wave * (int)gridDim.x + (int)blockIdx.x;
        f = (wave < hw && fs < (n1 << hs)) ? fs : __builtin_amdgcn_readfirstlane(fetch());
    }
    while (!PERSIST || f < nwork) {
    const bool heavy_ = f < (n1 << hs);
    // Tier-1 (heavy) items are cooperative (the host sends them only to a
    // kernel carrying the walk, CG != 0, with hs = log2(CG)): hs = 3 (G = 8):
    // a heavy tile's 8 sub-items are 8 rows of 8 pixels with eight lanes per
    // pixel (lane group g = pixel g of the row), walking the hierarchy
    // cooperatively (wide_walk_coop); hs = 2 (G = 4): 4 sub-items of 16
    // pixels, four lanes per pixel.
    const bool coop = GEO == GEO_WIDE && CG != 0 && heavy_;
    const int cg = coop ? CG : 0;
    const int item = heavy_ ? f >> hs : f - (n1 << hs) + n1;
    const int sub = heavy_ ? f & ((1 << hs) - 1) : 0;
    const int slot = item >> 2;
    // group_order: the learnt order (hierarchy kernels) or the caller's
    // group list (spt_scene_render_list_async, every kernel) of nslots
    // entries; a slot past it or an entry outside the frame renders nothing.
    const int grp = group_order ? (slot < nslots ? group_order[slot] : -1) : slot;
    const bool gvalid = (unsigned)grp < (unsigned)((ntiles + 3) >> 2);
    const int tile = grp * 4 + (item & 3);
    const int li = coop ? (sub << (6 - hs)) + (lane >> hs) : lane;   // pixel of the 8x8 tile
    const bool lead = !coop || (lane & (cg - 1)) == 0;  // the lane that stores the pixel and counts
    unsigned long long t_start = 0;
    if (SCHED) t_start = __builtin_amdgcn_s_memrealtime();
    // GSTORE (hierarchy kernels): per group of the block a 32x8 staging
    // strip in LDS -- colours, seeds, pixels -- and an arrival count.
    // (Addresses recomputed where used: held across the loop they spilled.)
    constexpr bool GSTORE = V.gstore();
#define GS_BASE() (smem + (size_t)((threadIdx.x >> 6) >> 2) * GS_BYTES)
    if (GSTORE) {
        if ((threadIdx.x & 255) == 0) *(int *)(GS_BASE() + GS_COUNT_OFF) = 0;
        __syncthreads();
    }
    int x = (tile % tiles_x) * 8 + (li & 7);
    // gstride > 1: the window is every gstride-th 8-row group from row_begin
    // (spt_scene_render_groups_async, multi-GPU load balance).
    int y = row_begin + (tile / tiles_x) * 8 * gstride + (li >> 3);
    // Refill (full-counter 8-wide kernels, items past the cooperative
    // tier): the wave starts on this item's 64 pixels, and from then on a
    // lane whose pixel has taken all its samples stores it and takes the next
    // pixel of the dispatch sequence (the rest of the wave's current item,
    // then further items), until the window's work is gone.  A tile of
    // configs[4] mixes pixels whose sample chains differ several-fold (sky
    // beside the fractal): waiting for the tile's slowest pixel left 28 % of
    // the lanes idle (tools/c4_lanes.py).  Every pixel's computation is
    // unchanged -- only which lane runs it, and when.
    // Counted kernels only: there the tile tail, not the levelling,
    // dominates -- 28 of 64 lanes per iteration without refill, 52 with,
    // profiles/r05/c4_counted_refill.log; on the uncounted frame refill
    // measured +7 % (its waves lose the levelled priority).
    const bool refill = COUNT && PERSIST && !heavy_;
    bool active = gvalid && tile < ntiles && x < w && y < row_end
                  SPT_TRACE(&& (g_spt_only_group < 0 || grp == g_spt_only_group));
    SPT_TRACE(unsigned tr_walk = 0, tr_leaf = 0, tr_trips = 0, tr_leafruns = 0, tr_queries = 0;
              const unsigned long long tr_c0 = __builtin_amdgcn_s_memtime();
              const unsigned long long tr_t0 = __builtin_amdgcn_s_memrealtime();
              unsigned tr_iters = 0;)
    if (active || refill || DQ) {       // (DQ: lanes without a pixel idle in the loop and pop ring entries)
        int i = (h - y - 1) * w + x;                            // smallptCPU.cpp:86
        uint32_t s0 = 0, s1 = 0;
        v3 col = mk(0.f, 0.f, 0.f);
        if (active) {
            s0 = seeds_in[2 * (size_t)i];
            s1 = seeds_in[2 * (size_t)i + 1];
            if (first_sample > 0)
                col = mk(colors[3 * (size_t)i], colors[3 * (size_t)i + 1], colors[3 * (size_t)i + 2]);
        }
        if (PARK && first_sample > 0) {         // (first_sample == 0: the first sample overwrites it)
            float *p = park_ptr();
            p[64 * SLOT_COL] = col.x;
            p[64 * (SLOT_COL + 1)] = col.y;
            p[64 * (SLOT_COL + 2)] = col.z;
        }
        const float invW = 1.f / w, invH = 1.f / h;             // :80-81
        // Refill state: the lane's pixel is px_ok (its group pgrp, started at
        // pix_t0), exhausted once the window has no pixel left for it; the
        // wave's dispatch cursor is item rf_f, pixel rf_p (wave-uniform: only
        // updated at the loop top, where every lane still looping is active).
        bool px_ok = active, exhausted = false;
        int pgrp = grp;
        unsigned pix_t0 = (unsigned)__builtin_amdgcn_s_memrealtime();
        int rf_f = f, rf_p = 64;

        // Per-lane path state.  Every loop iteration issues exactly ONE ray
        // query for every live lane -- the path ray (nearest hit) or, while a
        // DIFF vertex is sampling its lights, that light's shadow ray (any hit)
        // -- so the sphere loop runs with all lanes of the wave active.  The
        // shading after it is organised by the operations it needs rather than
        // by material, so that lanes in different situations share one pass of
        // the expensive code (RNG draws, square root, sincos, normalisation,
        // division) instead of each situation running its own divergent block:
        //   * pass A builds a light sample's shadow ray (SampleLights) or a
        //     REFR hit's Fresnel-chosen ray;
        //   * pass B builds a DIFF bounce ray or the next sample's camera ray.
        // A lane that needs both in one iteration (a light sample that yields
        // no shadow ray, then the bounce; a refraction that ends the path,
        // then the camera ray) runs A before B, so per lane the operations and
        // RNG draws are the reference's, in its order.
        ray3 ray;              // the ray queried next
        v3 rad = mk(0.f, 0.f, 0.f), thr = mk(1.f, 1.f, 1.f);
        int depth = 0;
        bool specular = true;
        bool shadow = false;   // ray is the shadow ray of light li (DUAL: a shadow ray (hit, sdir) is pending)
        v3 sdir = mk(0.f, 0.f, 0.f);   // DUAL: the pending shadow ray's direction (origin: hit)
        bool fin = false;      // DUAL: the sample ends once its pending shadow ray is resolved
        // The last hit point IS the next ray's origin: every ray after a hit
        // (bounce, mirror, refraction, shadow) starts there, and a camera
        // ray's origin is written into it when the old hit is dead.  One
        // register triple instead of copying hit into ray.o on four paths.
        v3 &hit = ray.o;
        v3 nl;                 // the last hit's oriented normal (SampleLights' args)
        v3 lsum;               // SampleLights' running result
        float lmax = 0.f;      // shadow ray maxt (len - EPSILON)
        float lw = 0.f;        // that light's weight s (geomfunc.h:159)
        int li = 0;
        int k = active ? 0 : nsamples;      // (refill: a lane without a pixel takes one first)
        bool need_cam = active && nsamples > 0, need_bounce = false;
        BvhWalk walk;          // GEO_BVH: the current query's walk state
        SPT_TRACE(walk.tr_leaf = walk.tr_trips = walk.tr_leafruns = 0;)
        SPT_PROF_ONLY(for (int b = 0; b < 3; b++) walk.pf_l[b] = walk.pf_w[b] = 0;)
        bool walking = false;  //   and whether it is suspended mid-walk
        // DQ: the lane's pending contributions, oldest first (npend of them:
        // pc0 in registers, the second in the SLOT_PEND slots; their ring positions
        // in pidx's bytes 0 and 1), of which the oldest npark belong to the
        // parked previous sample (the SLOT_RAD slots); and the wave's ring, q_count
        // entries from q_head (wave-uniform), flushed at q_T.
        v3 pc0 = mk(0.f, 0.f, 0.f);
        int pidx = 0, npend = 0, npark = 0;
        int q_head = 0, q_count = 0;
        const int q_T = sptpolicy::sq_threshold(sptpolicy::sflags_sq(sflags));
        // PARK: sample number `current`'s radiance r into the parked running
        // average (:110-118, the arithmetic of the register form below)
        const auto fold = [&](const v3 r, const int current) {
            float *p = park_ptr();
            v3 c = r;
            if (current != 0) {
                const float k1 = (float)current;
                const float k2 = rcp_nr(k1 + 1.f);
                c.x = (p[64 * SLOT_COL] * k1 + r.x) * k2;
                c.y = (p[64 * (SLOT_COL + 1)] * k1 + r.y) * k2;
                c.z = (p[64 * (SLOT_COL + 2)] * k1 + r.z) * k2;
            }
            p[64 * SLOT_COL] = c.x;
            p[64 * (SLOT_COL + 1)] = c.y;
            p[64 * (SLOT_COL + 2)] = c.z;
        };
        constexpr float nc = 1.f, nt = 1.5f;
        // prio_sched: the three level boundaries as fractions of the samples
        // (8 bits each, in 1/256; host: prio_schedule).  Every wave starts at
        // the top priority and levels down (no group is held at the top: the
        // round-2 rule, measured best for the binary walk, cost configs[4]
        // 2-8 % with the 8-wide one, profiles/r05/c4_heavy_prio_sweep.log).
        int prio_level = 0, prio_next = (nsamples * sptpolicy::prio_bound(prio_sched, 0)) >> 8;
        __builtin_amdgcn_s_setprio(3);
        while (true) {
            if (refill) {
                // ---- refill: lanes whose pixel is done store it, then take
                // the next pixels of the wave's dispatch sequence
                const bool want = k >= nsamples && !exhausted;
                const unsigned long long wm = __builtin_amdgcn_ballot_w64(want);
                if (wm) {
                    if (want && px_ok) {
                        if (nsamples > 0) {
                            colors[3 * (size_t)i] = col.x;
                            colors[3 * (size_t)i + 1] = col.y;
                            colors[3 * (size_t)i + 2] = col.z;
                            pixels[(size_t)y * w + x] = pack_rgb(col.x, col.y, col.z);
                        }
                        seeds_out[2 * (size_t)i] = s0;
                        seeds_out[2 * (size_t)i + 1] = s1;
                        if (SCHED && group_cost) {      // the pixel's duration: per group the sum, or
                            const unsigned dur = (unsigned)__builtin_amdgcn_s_memrealtime() - pix_t0;
                            if (sptpolicy::sflags_cost_max(sflags)) atomicMax(&group_cost[pgrp], dur);   //   the longest
                            else atomicAdd(&group_cost[pgrp], dur);
                        }
                    }
                    const unsigned long long need = __builtin_amdgcn_ballot_w64(want);
                    const int ncl = __builtin_popcountll(need);
                    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
                    const bool more = rf_p + ncl > 64;
                    const int f2 = more ? fetch() : nwork;
                    if (want) {
                        const int pos = rf_p + rank;
                        const int mf = pos < 64 ? rf_f : f2, mp = pos < 64 ? pos : pos - 64;
                        px_ok = false;
                        if (mf >= nwork) {
                            exhausted = true;
                        } else {
                            const int it = mf - (n1 << hs) + n1, sl = it >> 2;
                            const int g = group_order ? (sl < nslots ? group_order[sl] : -1) : sl;
                            const int tl = g * 4 + (it & 3);
                            x = (tl % tiles_x) * 8 + (mp & 7);
                            y = row_begin + (tl / tiles_x) * 8 * gstride + (mp >> 3);
                            if ((unsigned)g < (unsigned)((ntiles + 3) >> 2) && tl < ntiles && x < w && y < row_end) {
                                i = (h - y - 1) * w + x;
                                s0 = seeds_in[2 * (size_t)i];
                                s1 = seeds_in[2 * (size_t)i + 1];
                                col = mk(0.f, 0.f, 0.f);
                                if (first_sample > 0)
                                    col = mk(colors[3 * (size_t)i], colors[3 * (size_t)i + 1], colors[3 * (size_t)i + 2]);
                                k = 0;
                                need_cam = nsamples > 0;
                                px_ok = true;
                                pgrp = g;
                                pix_t0 = (unsigned)__builtin_amdgcn_s_memrealtime();
                            }
                        }
                    }
                    if (more) {
                        rf_f = f2;
                        rf_p += ncl - 64;
                    } else {
                        rf_p += ncl;
                    }
                }
            }
            // ---- pass B: DIFF bounce (geomfunc.h:229-269) or camera ray
            // (smallptCPU.cpp:89-105).  Both draw two randoms and normalise
            // one vector.
            if (need_bounce || need_cam) {
                SPT_PROF(PB_BOUNCE);
                const float f1 = get_random_f(s0, s1), f2 = get_random_f(s0, s1);
                const float x1 = __builtin_fmaf(f1, .5f, -1.f), x2 = __builtin_fmaf(f2, .5f, -1.f);
                // bounce: r1 = 2 PI x1, r2 = x2, u = norm(a x w)
                const v3 wv = nl;
                const v3 a = (fabsf(wv.x) > .1f) ? mk(0.f, 1.f, 0.f) : mk(1.f, 0.f, 0.f);
                const v3 cu = vxcross(a, wv);
                // camera: r1 = x1 - .5, r2 = x2 - .5
                // (PARK: the camera terms from the parking area's head)
                float4 cmx = make_float4(cam.x.x, cam.x.y, cam.x.z, invW), cmy = make_float4(cam.y.x, cam.y.y, cam.y.z, invH);
                float4 cmd = make_float4(cam.dir.x, cam.dir.y, cam.dir.z, 0.f);
                float4 cmo = make_float4(cam.orig.x, cam.orig.y, cam.orig.z, 0.f);
                if constexpr (PARK) {
                    int o = park_off;
                    asm volatile("" : "+s"(o));
                    const float4 *pc = (const float4 *)(smem + o);
                    cmx = pc[0]; cmy = pc[1]; cmd = pc[2]; cmo = pc[3];
                }
                const float kcx = (x + __builtin_fmaf(f1, .5f, -1.5f)) * cmx.w - .5f;   // r1 = GetRandom() - .5f
                const float kcy = (y + __builtin_fmaf(f2, .5f, -1.5f)) * cmy.w - .5f;
                const v3 rdir = mk(cmx.x * kcx + cmy.x * kcy + cmd.x,
                                   cmx.y * kcx + cmy.y * kcy + cmd.y,
                                   cmx.z * kcx + cmy.z * kcy + cmd.z);
                const v3 vn = vnorm(need_bounce ? cu : rdir);
                if (need_bounce) {
                    const float r2s = sqrt_exact(x2);
                    const v3 v = vxcross(wv, vn);
                    // sinf / cosf of r1 = 2 PI x1 and sqrtf(1 - x2).  draw_trig: the
                    // quadrant from f1's mantissa; 1 - x2 lies in [2^-23, 1] for every
                    // draw, inside sqrt_nr's range (x2 itself can be 0: r2s keeps the guard)
                    float sn1, cs1, r2c;
                    if constexpr (V.draw_trig()) {
                        rtm::sincos_2pi_draw_bits(__float_as_uint(f1), x1, sn1, cs1);
                        r2c = sqrt_nr(1 - x2);
                    } else {
                        rtm::sincosf(2.f * PI_F * x1, sn1, cs1);
                        r2c = sqrt_exact(1 - x2);
                    }
                    const v3 u = vsmul(cs1 * r2s, vn);
                    v3 nd = vadd(u, vsmul(sn1 * r2s, v));
                    nd = vadd(nd, vsmul(r2c, wv));
                    ray.d = nd;                          // origin: hit
                } else {
                    v3 rorig = vsmul(0.1f, rdir);
                    rorig = vadd(rorig, mk(cmo.x, cmo.y, cmo.z));
                    ray.o = rorig;
                    ray.d = vn;
                    // (rad, thr, depth, specular were reset when the previous
                    // sample finished: writing them only on this side made the
                    // compiler copy all six accumulators out and back around
                    // the branch every pass)
                }
                need_bounce = need_cam = false;
            }
            // DQ: a lane out of samples stays (live = false) until the wave
            // has none left and the ring is empty.
            const bool live = !DQ || k < nsamples;
            bool drain = false;
            if constexpr (DQ) {
                drain = !wave_any(live);
                if (drain && q_count == 0) break;
            } else if (k >= nsamples) {
                if (!refill || exhausted) break;
                continue;                       // (a pixel past the frame's edge: claim again)
            }
            // Progress-levelled issue priority.  The SIMD arbitrates VALU issue
            // by priority, then age, so waves that start together finish one
            // after another and the last one runs alone at a fraction of the
            // SIMD's rate.  A wave whose every lane has passed another quarter
            // of its samples drops one priority level, letting the waves
            // behind it catch up: co-resident waves stay level and finish
            // together.  (s_setprio only reorders issue; results unchanged.)
            if (!refill && !wave_any(k < prio_next)) {
                prio_level++;
                prio_next = prio_level < 3 ? (nsamples * sptpolicy::prio_bound(prio_sched, prio_level)) >> 8 : nsamples;
                if (prio_level == 1) __builtin_amdgcn_s_setprio(2);
                else if (prio_level == 2) __builtin_amdgcn_s_setprio(1);
                else __builtin_amdgcn_s_setprio(0);
            }

            SPT_PROF(PB_ITER);
            SPT_TRACE(tr_iters++;)
            float t = (shadow && !DUAL) ? lmax : 1e20f;
            int first = -1;
            int id;
            bool done = false, lights = false, a_R = false;
            bool pushed = false;            // DQ: the lane pushed a shadow ray in this iteration
            if constexpr (DQ) {
                id = -1;
                if (live) id = query_bf<COUNT, V.key_accept()>(geo, ray, t, first);
                // What this lane's shading is about to do that an unresolved
                // entry must precede: add an emitter term, end its sample, push.
                bool f_emit = false, f_ends = false, f_diff = false;
                if (live && npend > 0) {
                    bool emit = false;
                    if (id >= 0) {
                        const float4 oe = S.emi[id];
                        emit = !((oe.x == 0.f) && (oe.x == 0.f) && (oe.z == 0.f));
                        f_diff = !emit && __float_as_int(oe.w) == DIFF;
                    }
                    f_emit = emit && specular;
                    f_ends = id < 0 || emit || depth >= 6;
                }
                while (true) {
                    const bool force = (f_emit && npend > npark) || (f_ends && npark > 0) || (f_diff && npend == 2);
                    // (a forcing lane has an entry in the ring, so q_count > 0 then)
                    if (q_count == 0 || !(sptpolicy::sq_flush(q_count, q_T) || drain || wave_any(force))) break;
                    // ---- flush pass: lane j takes entry head + j
                    const int m = sptpolicy::sq_pop(q_count);
                    const int e = sptpolicy::sq_wrap(q_head + lane);
                    const float *rg = ring_ptr();
                    ray3 rs;
                    rs.o = mk(rg[e], rg[SQ_RING + e], rg[2 * SQ_RING + e]);
                    rs.d = mk(rg[3 * SQ_RING + e], rg[4 * SQ_RING + e], rg[5 * SQ_RING + e]);
                    const float maxt = rg[6 * SQ_RING + e];
                    const bool have = lane < m;
                    SPT_PROF_ONLY(if (have) prof_l[PB_FLUSH]++; if (lane == 0) prof_w[PB_FLUSH]++;)
                    SPT_PROF_ONLY({
                        const int why = sptpolicy::sq_flush(q_count, q_T)        ? PB_FL_THRESH
                                        : wave_any(f_diff && npend == 2)         ? PB_FL_SLOT
                                        : wave_any(f_ends && npark > 0)          ? PB_FL_ENDS
                                        : wave_any(f_emit && npend > npark)      ? PB_FL_EMIT
                                                                                 : PB_FL_DRAIN;
                        _Pragma("unroll") for (int b = PB_FL_THRESH; b <= PB_FL_DRAIN; b++) {
                            if (have && b == why) prof_l[b]++;
                            if (lane == 0 && b == why) prof_w[b]++;
                        }
                    })
                    const unsigned long long unocc = shadow_bf_unocc(geo, rs, maxt, have);
                    // owners (:154-161, then :229-230): a lane's popped entries, at most
                    // two, resolved in straight-line code, oldest first -- parked terms
                    // onto the parked rad (one load and one store of SLOT_RAD), the
                    // fold at most once, the other terms onto rad, then the shift.
                    // (The per-entry loop this replaces ran 2.0 rounds a pass, each with
                    // its own exec-mask bookkeeping, and folded in 1.6 of them.)
                    const sptpolicy::SqOwners ow = sptpolicy::sq_owners(pidx, npend, q_head, m, unocc);
                    if (ow.r0) {
                        SPT_PROF(PB_OW_ROUND);
                        SPT_PROF_ONLY(if (ow.r1) prof_l[PB_OW_ROUND]++;)
                        SPT_PROF_ONLY(if (ow.r1) SPT_PROF(PB_OW_TWO); else SPT_PROF(PB_OW_ONE);)
                        const int nres = sptpolicy::sq_owners_resolved(ow);
                        const int nparked = sptpolicy::sq_owners_parked(nres, npark);
                        float *p = park_ptr();
                        v3 pc1 = pc0;           // the second term: resolved now, or the oldest from here on
                        if (npend == 2) pc1 = mk(p[64 * SLOT_PEND], p[64 * (SLOT_PEND + 1)], p[64 * (SLOT_PEND + 2)]);
                        if (nparked > 0) {
                            v3 pr = mk(p[64 * SLOT_RAD], p[64 * (SLOT_RAD + 1)], p[64 * (SLOT_RAD + 2)]);
                            const bool add0 = ow.lit0, add1 = nparked == 2 && ow.lit1;
                            if (add0) pr = vadd(pr, pc0);
                            if (add1) pr = vadd(pr, pc1);
                            if (add0 || add1) {
                                p[64 * SLOT_RAD] = pr.x;
                                p[64 * (SLOT_RAD + 1)] = pr.y;
                                p[64 * (SLOT_RAD + 2)] = pr.z;
                            }
                            if (nparked == npark) {
                                SPT_PROF(PB_OW_FOLD);
                                // (an opaque copy: the compiler otherwise hoists the fold's
                                // int-to-float and rcp_nr in front of the flush loop, into
                                // every iteration -- seven VALU operations and two registers)
                                int prev = first_sample + k - 1;
                                asm volatile("" : "+v"(prev));
                                fold(pr, prev);
                            }
                        } else if (ow.lit0) {
                            rad = vadd(rad, pc0);
                        }
                        if (ow.lit1 && nparked < 2) rad = vadd(rad, pc1);
                        npark -= nparked;
                        npend -= nres;
                        pidx = sptpolicy::sq_owners_shift(pidx, nres);
                        pc0 = pc1;
                    }
                    q_head = __builtin_amdgcn_readfirstlane(sptpolicy::sq_wrap(q_head + m));
                    q_count = __builtin_amdgcn_readfirstlane(q_count - m);
                }
            } else if constexpr (DUAL) {
                // Both rays at once when any lane holds a shadow ray; its
                // result is applied first (the light sample precedes the
                // bounce's hit in the reference's order).
                if (wave_any(shadow)) {
                    float ts = lmax;
                    int ids, firsts = -1;
                    ray3 rs;
                    rs.o = hit;
                    rs.d = sdir;
                    query2_bf<COUNT>(geo, ray, t, id, rs, shadow, ts, ids, firsts);
                    if (shadow) {                               // :154-161, then :229-230
                        SPT_PROF(PB_SHADOW);
                        cnt.isectp++;
                        cnt.tests += firsts >= 0 ? (unsigned)(S.n - firsts) : (unsigned)S.n;
                        if (ids < 0) {
                            const float4 le = S.lrec[2];
                            const v3 ld = vsmul(lw, mk(le.x, le.y, le.z));   // 0 + e * s
                            rad = vadd(rad, vmul(thr, ld));
                        }
                        shadow = false;
                        done = fin;
                    }
                } else {
                    id = query_bf<COUNT, V.key_accept()>(geo, ray, t, first);
                }
            } else if constexpr (GEO == GEO_BVH) {
                // Resumable walk: a lane whose query needs more than this
                // iteration's step budget sits out the rest of the iteration
                // and continues its walk in the next one.
                SPT_TRACE(const unsigned long long tr_w0 = __builtin_amdgcn_s_memtime(); tr_queries += !walking;)
                if (!walking) bvh_begin<COUNT>(bvh, ray, shadow, t, walk);
                walking = !bvh_walk<COUNT>(bvh, ray, shadow, walk);
                SPT_TRACE(tr_walk += (unsigned)(__builtin_amdgcn_s_memtime() - tr_w0);)
                if (walking) continue;
                t = walk.t;
                id = walk.id;
                first = id;                 // any hit: the highest occluder (COUNT)
            } else if constexpr (GEO == GEO_WIDE) {
                SPT_TRACE(const unsigned long long tr_w0 = __builtin_amdgcn_s_memtime(); tr_queries += !walking;)
                if (!walking) wide_begin<COUNT>(bvh, ray, shadow, t, walk);
                if constexpr (CG != 0)
                    walking = coop ? !wide_walk_coop<COUNT, (CG ? CG : 8)>(bvh, wL, wstk, ray, shadow, walk, split)
                                   : !wide_walk<COUNT>(bvh, wL, wstk, ray, shadow, walk, split);
                else
                    walking = !wide_walk<COUNT>(bvh, wL, wstk, ray, shadow, walk, split);
                SPT_TRACE(tr_walk += (unsigned)(__builtin_amdgcn_s_memtime() - tr_w0);)
                if (walking) continue;
                SPT_PROF(PB_WSHADE);
                t = walk.t;
                id = walk.id;
                first = id;                 // any hit: the highest occluder (COUNT)
            } else {
                id = query_bf<COUNT, V.key_accept()>(geo, ray, t, first);
            }
            float dp = 0.f, inv_sign = 1.f;  // REFR (pass A): vdot(normal, ray.d), -1 * sign(dp); and id
            if (DQ && !live) {
                // no sample left: the lane only takes part in the flush passes
            } else if (DUAL && fin) {
                // the path ended at the last DIFF vertex: no path ray this iteration
            } else if (shadow && !DUAL) {                       // :154-161
                SPT_PROF(PB_SHADOW);
                cnt.isectp++;
                cnt.tests += first >= 0 ? (unsigned)(S.n - first) : (unsigned)S.n;
                if (id < 0) {
                    const float4 le = S.lrec[3 * li + 2];
                    lsum = vadd(lsum, vsmul(lw, mk(le.x, le.y, le.z)));
                }
                li++;
                lights = true;
                shadow = false;
            } else {                                            // one bounce of :182-337
                cnt.isect++;
                cnt.tests += S.n;
                if (id < 0) {
                    done = true;
                } else {
                    SPT_PROF(PB_NEAREST);
                    const float4 og = S.geo[id], oe = S.emi[id], oc = S.col[id];
                    hit = vadd(ray.o, vsmul(t, ray.d)); // ray.o + ray.d * t (hit aliases ray.o)
                    v3 normal = vsub(hit, mk(og.x, og.y, og.z));
                    normal = vnorm(normal);
                    dp = vdot(normal, ray.d);
                    inv_sign = -1.f * (dp > 0 ? 1.f : -1.f);
                    nl = vsmul(inv_sign, normal);
                    const int refl = __float_as_int(oe.w);
                    if (!((oe.x == 0.f) && (oe.x == 0.f) && (oe.z == 0.f))) {
                        if (specular) {
                            v3 e = vsmul(fabsf(dp), mk(oe.x, oe.y, oe.z));
                            e = vmul(thr, e);
                            rad = vadd(rad, e);
                        }
                        done = true;
                    } else if (refl == DIFF) {
                        SPT_PROF(PB_DIFF);
                        specular = false;
                        thr = vmul(thr, mk(oc.x, oc.y, oc.z));
                        lsum = mk(0.f, 0.f, 0.f);
                        if constexpr (!DUAL) li = 0;            // (DUAL: the only light, no index)
                        lights = true;
                    } else if (refl == SPEC) {
                        SPT_PROF(PB_SPEC);
                        specular = true;
                        v3 nd = vsmul(2.f * vdot(normal, ray.d), normal);
                        nd = vsub(ray.d, nd);
                        thr = vmul(thr, mk(oc.x, oc.y, oc.z));
                        ray.d = nd;                             // origin: hit
                    } else {
                        SPT_PROF(PB_REFR);
                        specular = true;
                        a_R = true;                             // ray, hit, nl, dp, inv_sign, id -> pass A
                    }
                    depth++;
                    // :184 at the next bounce.  (A REFR lane's test follows its pass A
                    // below; DUAL: taken here -- done is false on that side, pass A does
                    // not read it, and the merge behind pass A cost five VALU operations.)
                    done = done || (!lights && (DUAL || !a_R) && depth > 6);
                }
            }

            // ---- pass A: SampleLights (:112-165) from light li on, stopping at
            // the next light that needs a shadow test, and/or the REFR branch
            // (:281-336).  Repeats only while some lane skips a light (several
            // lights).  UniformSampleSphere's two GetRandom() arguments are
            // drawn second-first, as the g++-built oracle does (:138); the
            // Russian-roulette draw of REFR is taken before its Fresnel terms
            // (no other draw of the lane lies between).
            // (DUAL: one light, so every lane at a DIFF hit samples it.)
            bool a_L = DUAL ? lights : lights && li < S.nlights;
            bool lights_done = lights && !a_L;
            const bool was_R = a_R;
            // One pass for every lane that needs A, then further light-only
            // passes while some lane skipped a light (scenes with several
            // lights).  The body is one lambda instantiated twice so the
            // common single pass is straight-line code (a loop around both
            // made the compiler shuffle all loop-carried state every pass).
            const auto pass_a = [&](const bool with_r) {
                {
                    SPT_PROF(PB_LIGHT);
                    // Loaded by every lane (an R-only lane's light terms are
                    // discarded by the selects below; li is clamped into the
                    // light list) -- a conditional load left five zeroing
                    // moves and a branch in every pass.
                    // (DUAL: the only light's record, at its fixed address.)
                    const int lj = DUAL ? 0 : (li < S.nlights ? li : 0);
                    const float4 lg = S.lrec[3 * lj];           // centre
                    const float4 lc = S.lrec[3 * lj + 1];       // colour.xyz, rad
                    // REFR terms (:281-296), rebuilt here from the few values
                    // kept since the hit: normal = inv_sign * nl exactly
                    // (inv_sign = +-1), and, rounding being sign-symmetric,
                    // vdot(normal, nl) = inv_sign * |n|^2 and vdot(ray.d, nl) =
                    // inv_sign * dp exactly: into is dp <= 0 (false for NaN, as
                    // the reference's NaN dot) and ddn is dp signed.
                    const v3 normal = vsmul(inv_sign, nl);
                    const bool into = dp <= 0.f;
                    const float nnt = into ? nc / nt : nt / nc;
                    const float ddn = inv_sign * dp;
                    const float cos2t = 1.f - nnt * nnt * (1.f - ddn * ddn);
                    const bool tir = cos2t < 0.f;
                    // (g1: the [2, 4) float x1 is made from, whose mantissa gives
                    // the angle's quadrant; no draw: 2, x1 = 0)
                    float g1 = 2.f, x2 = 0.f;
                    if (a_L || (with_r && !tir)) g1 = get_random_f(s0, s1);   // L: u2; R: the roulette draw
                    const float x1 = __builtin_fmaf(g1, .5f, -1.f);
                    if (a_L) x2 = get_random(s0, s1);           // L: u1
                    const float zz = 1.f - 2.f * x2;            // UniformSampleSphere, :61-69
                    const float q = 1.f - zz * zz;
                    const float sq = sqrt_exact((!with_r || a_L) ? ((0.f > q) ? 0.f : q) : (tir ? 1.f : cos2t));
                    float sp_sin, sp_cos;                       // of phi = 2 PI x1 (no draw: x1 = 0)
                    if constexpr (V.draw_trig()) rtm::sincos_2pi_draw_bits(__float_as_uint(g1), x1, sp_sin, sp_cos);
                    else rtm::sincosf(2.f * PI_F * x1, sp_sin, sp_cos);
                    const v3 unit = mk(sq * sp_cos, sq * sp_sin, zz);
                    v3 sp = vsmul(lc.w, unit);
                    sp = vadd(sp, mk(lg.x, lg.y, lg.z));
                    const v3 vl = vsub(sp, hit);                // shadow ray direction
                    const float kk = (into ? 1.f : -1.f) * (ddn * nnt + sq);
                    const v3 vr = vsub(vsmul(nnt, ray.d), vsmul(kk, normal));   // refracted direction
                    const v3 vv = (!with_r || a_L) ? vl : vr;
                    const float dd = vdot(vv, vv);
                    float len, ilen;                            // sqrtf(dd), 1.f / len
                    // (DUAL: the short forms fall through; the other kernels' layout is
                    // left as it was -- the hint costs them four to six scalar instructions)
                    const bool in_range = !wave_any(!sqrt_nr_ok(dd));
                    if (DUAL ? __builtin_expect(in_range, 1) : in_range) {
                        len = sqrt_nr(dd);
                        ilen = rcp_nr(len);
                    } else {
                        len = sqrt_rn(dd);
                        ilen = 1.f / len;
                    }
                    const v3 vn = vsmul(ilen, vv);
                    const float dv = vdot(vn, (!with_r || a_L) ? unit : normal);   // L: wo; R: vdot(td, normal)
                    // L: weight (4 PI rad^2) wi wo / len^2; R: RP = Re / P or TP = Tr / (1 - P)
                    const float wo = -dv;
                    const float wi = vdot(vn, nl);
                    const bool lit = a_L && !(dv > 0.f) && wi > 0.f;
                    const float a = nt - nc, b = nt + nc;
                    const float R0 = a * a / (b * b);
                    const float c = 1 - (into ? -ddn : dv);
                    const float Re = R0 + (1 - R0) * c * c * c * c * c;
                    const float Tr = 1.f - Re;
                    const float P = .25f + .5f * Re;
                    const bool refl_pick = x1 < P;
                    const bool l_lane = !with_r || a_L;
                    const float num = l_lane ? (4.f * PI_F * lc.w * lc.w) * wi * wo : (refl_pick ? Re : Tr);
                    const float den = l_lane ? len * len : (refl_pick ? P : 1.f - P);
                    const float quo = num / den;
                    // DQ: the pushing lanes' ranks (lit is false for an R lane)
                    unsigned long long pm = 0;
                    if constexpr (DQ) pm = __builtin_amdgcn_ballot_w64(lit);
                    if (!with_r || a_L) {
                        if (DQ && lit) {
                            // the shadow ray into the ring, its term c = thr * (e * s) kept
                            const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(pm >> 32),
                                                                       __builtin_amdgcn_mbcnt_lo((unsigned)pm, 0u));
                            const int pos = sptpolicy::sq_push_pos(q_head, q_count, rank);
                            float *rg = ring_ptr();
                            rg[pos] = hit.x;
                            rg[SQ_RING + pos] = hit.y;
                            rg[2 * SQ_RING + pos] = hit.z;
                            rg[3 * SQ_RING + pos] = vn.x;
                            rg[4 * SQ_RING + pos] = vn.y;
                            rg[5 * SQ_RING + pos] = vn.z;
                            rg[6 * SQ_RING + pos] = len - EPS;
                            const float4 le = S.lrec[2];
                            const v3 c = vmul(thr, vsmul(quo, mk(le.x, le.y, le.z)));   // 0 + e * s, then thr * Ld
                            // (Selects and an unconditional store, not two branch
                            // sides: the sides met in seven register copies on every
                            // push.  A lane with nothing pending writes the second
                            // entry's slot too; nothing reads it before the next push
                            // with one entry pending rewrites it.)
                            const bool first_term = npend == 0;
                            float *p = park_ptr();
                            p[64 * SLOT_PEND] = c.x;
                            p[64 * (SLOT_PEND + 1)] = c.y;
                            p[64 * (SLOT_PEND + 2)] = c.z;
                            pc0 = mk(first_term ? c.x : pc0.x, first_term ? c.y : pc0.y, first_term ? c.z : pc0.z);
                            pidx = first_term ? pos : (pidx | pos << 8);
                            npend++;
                            pushed = true;
                            a_L = false;
                            lights_done = true;                 // the only light
                        } else if (lit) {
                            if (DUAL) {
                                sdir = vn;                      // queried next iteration, with the bounce ray
                            } else {
                                ray.d = vn;                     // origin: hit
                            }
                            lmax = len - EPS;
                            lw = quo;
                            shadow = true;
                            a_L = false;
                            if (DUAL) lights_done = true;       // the only light
                        } else if constexpr (DUAL) {
                            a_L = false;
                            lights_done = true;                 // the only light
                        } else {
                            li++;
                            a_L = li < S.nlights;
                            lights_done = !a_L;
                        }
                    } else {
                        const float4 oc = S.col[id];
                        v3 nd = vsmul(2.f * dp, normal);         // vdot(normal, ray.d) = dp
                        nd = vsub(ray.d, nd);
                        if (tir) {                              // origin: hit
                            thr = vmul(thr, mk(oc.x, oc.y, oc.z));
                            ray.d = nd;
                        } else {
                            thr = vsmul(quo, thr);
                            thr = vmul(thr, mk(oc.x, oc.y, oc.z));
                            ray.d = refl_pick ? nd : vn;
                        }
                        a_R = false;
                    }
                }
            };
            // A scene without REFR spheres (sflags' no_refr: configs[4]'s 10k
            // spheres are all DIFF) never sets a_R: its lanes take the
            // light-only body, whose operations and draws for an a_L lane are
            // pass_a(true)'s without the Fresnel / refraction terms it would
            // compute and discard (~45 VALU per pass).  Hierarchy kernels only.
            if ((GEO == GEO_BVH || GEO == GEO_WIDE) && sptpolicy::sflags_no_refr(sflags)) {
                if (a_L) pass_a(false);
            } else if (a_L || a_R) {
                pass_a(true);
            }
            // With one light the pass above always leaves a_L false (lit, or
            // li = 1 = nlights); the scalar test keeps the light-only loop --
            // and the copies of the loop-carried state the compiler puts at
            // its header, 12 VALU ops per iteration -- out of such scenes.
            // A DUAL kernel runs only such scenes and has no such loop.
            if constexpr (!DUAL) {
                if (S.nlights > 1) {
                    while (wave_any(a_L)) {
                        if (a_L) pass_a(false);
                    }
                }
            }
            if constexpr (DQ)      // this iteration's pushes (one pass A: every lane is back here)
                q_count = __builtin_amdgcn_readfirstlane(
                    q_count + __builtin_popcountll(__builtin_amdgcn_ballot_w64(pushed)));
            if constexpr (!DUAL) {
                if (was_R) done = depth > 6;
            }
            if (lights_done) {                                 // :229-230, then the bounce
                // (DUAL: Ld is 0 + e * s once the pending shadow ray is
                // resolved, or 0 -- and rad + thr * 0 == rad -- if none.)
                if (!DUAL) rad = vadd(rad, vmul(thr, lsum));
                if (DL) {
                    done = true;                                // :413-414
                } else if (depth > 6) {                         // the bounce's two draws, then :184
                    (void)get_random(s0, s1);
                    (void)get_random(s0, s1);
                    if (DUAL && shadow) fin = true;             // ends after the shadow result
                    else done = true;
                } else {
                    need_bounce = true;
                }
            }
            if (done) {                                         // :110-118 running average
                SPT_PROF(PB_DONE);
                const int current = first_sample + k;
                if constexpr (DQ) {
                    // terms still pending: rad waits in LDS for the last of
                    // them (the previous sample is folded by now: f_ends)
                    if (npend > 0) {
                        float *p = park_ptr();
                        p[64 * SLOT_RAD] = rad.x;
                        p[64 * (SLOT_RAD + 1)] = rad.y;
                        p[64 * (SLOT_RAD + 2)] = rad.z;
                        npark = npend;
                    } else {
                        fold(rad, current);
                    }
                } else if constexpr (PARK) {
                    fold(rad, current);         // the parked colour: loaded, updated and written back
                } else if (current == 0) {
                    col = rad;
                } else {
                    const float k1 = (float)current;
                    const float k2 = rcp_nr(k1 + 1.f);      // 2 <= k1 + 1 <= 2^31: rcp_nr range
                    col.x = (col.x * k1 + rad.x) * k2;
                    col.y = (col.y * k1 + rad.y) * k2;
                    col.z = (col.z * k1 + rad.z) * k2;
                }
                cnt.samples++;
                if (CALLS && (cnt.isect | cnt.isectp) >= 0x80000000u) {   // (long launches: before 32 bits wrap)
                    atomicAdd(counters, (unsigned long long)cnt.isect);
                    atomicAdd(counters + 1, (unsigned long long)cnt.isectp);
                    cnt.isect = cnt.isectp = 0;
                }
                k++;
                need_cam = k < nsamples;
                fin = false;
                rad = mk(0.f, 0.f, 0.f);                        // the next sample's path state
                thr = mk(1.f, 1.f, 1.f);                        // (smallptCPU.cpp:89-105 via pass B)
                depth = 0;
                specular = true;
            }
        }
        if (GSTORE) {                                   // staged: the group's last wave stores it
            float *gs_col = (float *)GS_BASE();
            uint32_t *gs_seed = (uint32_t *)(GS_BASE() + GS_SEED_OFF), *gs_px = (uint32_t *)(GS_BASE() + GS_PX_OFF);
            const int c = (wave & 3) * 8 + (lane & 7), r = lane >> 3;
            if (nsamples > 0) {
                gs_col[r * 96 + 3 * c] = col.x;
                gs_col[r * 96 + 3 * c + 1] = col.y;
                gs_col[r * 96 + 3 * c + 2] = col.z;
                gs_px[r * 32 + c] = pack_rgb(col.x, col.y, col.z);
            }
            gs_seed[r * 64 + 2 * c] = s0;
            gs_seed[r * 64 + 2 * c + 1] = s1;
        } else if (lead && !refill && (!DQ || active)) {   // (refill: stored as each pixel finished)
            if (PARK && nsamples > 0) {          // the parked colour back
                const float *p = park_ptr();
                col = mk(p[64 * SLOT_COL], p[64 * (SLOT_COL + 1)], p[64 * (SLOT_COL + 2)]);
            }
            if (nsamples > 0) {
                colors[3 * (size_t)i] = col.x;
                colors[3 * (size_t)i + 1] = col.y;
                colors[3 * (size_t)i + 2] = col.z;
                pixels[(size_t)y * w + x] = pack_rgb(col.x, col.y, col.z);
            }
            seeds_out[2 * (size_t)i] = s0;
            seeds_out[2 * (size_t)i + 1] = s1;
        }
        SPT_PROF_ONLY(for (int b = 0; b < 3; b++) {
            prof_l[PB_WCALL + b] += walk.pf_l[b];
            prof_w[PB_WCALL + b] += walk.pf_w[b];
        })
        SPT_TRACE(if (GEO == GEO_BVH || GEO == GEO_WIDE) {
            tr_leaf = walk.tr_leaf;
            tr_trips = walk.tr_trips;
            tr_leafruns = walk.tr_leafruns;
        })
    }
    if (GSTORE) {
        // The group's four waves finish at different times (configs[4]: per-
        // wave work varies 6x); each leaves its 8x8 tile in LDS and the last
        // one stores the whole 32x8 strip, so every 128-B line of the colour,
        // seed and pixel rows is written once, whole.  (Stored per wave, the
        // 96-B colour and 32-B pixel row segments of a tile share lines with
        // the neighbouring tiles' and reach HBM as partial lines when the
        // neighbours finish much later: 71 MB written per frame for 50 MB.)
        const float *gs_col = (const float *)GS_BASE();
        const uint32_t *gs_seed = (const uint32_t *)(GS_BASE() + GS_SEED_OFF);
        const uint32_t *gs_px = (const uint32_t *)(GS_BASE() + GS_PX_OFF);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        int old = 0;
        if (lane == 0) old = atomicAdd((int *)(GS_BASE() + GS_COUNT_OFF), 1);
        old = __shfl(old, 0, 64);
        if (old == 3) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            // entry (row r, group column c) -> its pixel, or invalid
            const auto pix = [&](int r, int c, int &xx, int &yy) {
                const int tl = grp * 4 + (c >> 3);
                xx = (tl % tiles_x) * 8 + (c & 7);
                yy = row_begin + (tl / tiles_x) * 8 * gstride + r;
                return gvalid && tl < ntiles && xx < w && yy < row_end;
            };
            int xx, yy;
            if (nsamples > 0) {
#pragma unroll 4
                for (int k = 0; k < 12; k++) {
                    const int j = k * 64 + lane, r = j / 96, c3 = j % 96, c = c3 / 3;
                    if (pix(r, c, xx, yy)) colors[3 * ((size_t)(h - yy - 1) * w + xx) + (c3 - 3 * c)] = gs_col[j];
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int j = k * 64 + lane, r = j >> 5, c = j & 31;
                    if (pix(r, c, xx, yy)) pixels[(size_t)yy * w + xx] = gs_px[j];
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int j = k * 64 + lane, r = j >> 6, c2 = j & 63, c = c2 >> 1;
                if (pix(r, c, xx, yy)) seeds_out[2 * ((size_t)(h - yy - 1) * w + xx) + (c2 & 1)] = gs_seed[j];
            }
        }
    }
#undef GS_BASE
    if (SCHED && group_cost && gvalid && lane == 0 && !refill) {  // this tile's duration (100 MHz ticks), summed per group
        const unsigned dur = (unsigned)(__builtin_amdgcn_s_memrealtime() - t_start);
        if (sptpolicy::sflags_cost_max(sflags)) atomicMax(&group_cost[grp], dur);   // (Shape::cost_max: the group's longest tile)
        else atomicAdd(&group_cost[grp], dur);
    }
    SPT_TRACE({
        const unsigned long long t1 = __builtin_amdgcn_s_memrealtime();
        unsigned mx = tr_iters;
        _Pragma("unroll")
        for (int off = 32; off > 0; off >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, off, 64));
        const unsigned sum = (unsigned)wave_sum_u64(tr_iters);
        const size_t wv = (size_t)f;                       // one record per work item (tile)
        const unsigned tr_tot = (unsigned)(__builtin_amdgcn_s_memtime() - tr_c0);
        unsigned ph[6] = {tr_walk, tr_leaf, tr_trips, tr_leafruns, tr_queries, tr_tot};
        _Pragma("unroll")
        for (int q = 0; q < 6; q++)
            _Pragma("unroll")
            for (int off = 32; off > 0; off >>= 1) ph[q] = max(ph[q], (unsigned)__shfl_xor((int)ph[q], off, 64));
        if (lane == 0 && g_spt_trace) {
            g_spt_trace[4 * wv] = make_uint4((unsigned)tr_t0, (unsigned)t1, __builtin_amdgcn_s_getreg(0xF804),
                                             __builtin_amdgcn_s_getreg(0xF814));
            g_spt_trace[4 * wv + 1] = make_uint4(sum, mx, (unsigned)grp, ph[5]);
            g_spt_trace[4 * wv + 2] = make_uint4(ph[0], ph[1], ph[2], ph[3]);
            g_spt_trace[4 * wv + 3] = make_uint4(ph[4], 0u, 0u, 0u);
        }
    })
    if (CALLS && PERSIST && sptpolicy::split_coop(split)) {   // a cooperative group counts its pixel once:
        if (!lead) cnt = Counts{0, 0, 0, 0};            //   flushed per work item
        const unsigned long long c[4] = {cnt.isect, cnt.isectp, COUNT ? cnt.tests : 0ull, cnt.samples};
        flush_counters<4>(counters, c);
        cnt = Counts{0, 0, 0, 0};
    }
    if (!PERSIST || refill) break;          // (refill: the wave took pixels until the window ran out)
    f = __builtin_amdgcn_readfirstlane(fetch());
    }   // work items
    if (CALLS) {
        const unsigned long long c[4] = {cnt.isect, cnt.isectp, COUNT ? cnt.tests : 0ull, cnt.samples};
        flush_counters<4>(counters, c);
    }
    SPT_PROF_ONLY(_Pragma("unroll") for (int b = 0; b < PB_N; b++) {
        const unsigned long long l = wave_sum_u64(prof_l[b]), v = wave_sum_u64(prof_w[b]);
        if (lane == 0) { atomicAdd(&g_spt_prof[2 * b], l); atomicAdd(&g_spt_prof[2 * b + 1], v); }
    })
}

// toInt pack of rows [row_begin, row_end) from the accumulator: the pixels
// render_kernel writes at the end of a launch (smallptCPU.cpp:120-122), for a
// frame whose colour bands came from other ranks.
__global__ void __launch_bounds__(256) pack_kernel(const float *__restrict__ colors, uint32_t *__restrict__ pixels,
                                                   int w, int h, int row_begin, int row_end)
{
    const size_t n = (size_t)(row_end - row_begin) * w;
    for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
        const int y = row_begin + (int)(p / w), x = (int)(p % w);
        const size_t i = (size_t)(h - y - 1) * w + x;
        pixels[(size_t)y * w + x] = pack_rgb(colors[3 * i], colors[3 * i + 1], colors[3 * i + 2]);
    }
}

// Tile groups <-> a packed buffer (a multi-GPU frame split by explicit group
// lists, spt_groups_pack_async): group g is the 8x8 tiles 4g .. 4g+3 of the
// frame in row-major tile order; its 768 packed floats are tile by tile, row
// by row, pixel by pixel, (r, g, b) -- the accumulator slots (h-y-1)*w+x.
// Pixels outside the frame (and entries outside [0, ngroups_total)) pack as
// 0 and are skipped when unpacking.  Exact copies.
constexpr int GROUP_FLOATS = 4 * 64 * 3;
template <bool PACK>
__global__ void __launch_bounds__(256) groups_copy_kernel(float *__restrict__ colors, int w, int h,
                                                          const int *__restrict__ groups, int n,
                                                          float *__restrict__ buf)
{
    const int tiles_x = (w + 7) / 8, ntiles = tiles_x * ((h + 7) / 8), total = (ntiles + 3) / 4;
    const size_t ne = (size_t)n * GROUP_FLOATS;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < ne; e += (size_t)gridDim.x * blockDim.x) {
        const int k = (int)(e / GROUP_FLOATS), q = (int)(e % GROUP_FLOATS);
        const int g = groups[k];
        const int tile = g * 4 + q / 192, p = (q % 192) / 3, comp = q % 3;
        const int x = (tile % tiles_x) * 8 + (p & 7), y = (tile / tiles_x) * 8 + (p >> 3);
        const bool in = (unsigned)g < (unsigned)total && tile < ntiles && x < w && y < h;
        const size_t i = 3 * ((size_t)(h - 1 - y) * w + x) + comp;
        if (PACK) buf[e] = in ? colors[i] : 0.f;
        else if (in) colors[i] = buf[e];
    }
}

// A caller's group list made a set (spt_scene_render_list_async): one entry
// per listed group survives into `out` -- the one whose claim on the group's
// bit of `claimed` (zeroed) came first -- and every repeat or out-of-range
// entry becomes -1, which render_kernel skips.  Two waves can then never
// render the same pixels (their accumulator and seed slots) in one launch, and
// a group's wave time is added to its cost entry once.  Which copy of a repeat
// survives moves only its dispatch slot, never a result.
__global__ void __launch_bounds__(256) list_dedup_kernel(const int *__restrict__ groups, int n, int total,
                                                         unsigned *__restrict__ claimed, int *__restrict__ out)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        const int g = groups[k];
        int v = -1;
        if ((unsigned)g < (unsigned)total) {
            const unsigned bit = 1u << (g & 31);
            if (!(atomicOr(&claimed[g >> 5], bit) & bit)) v = g;
        }
        out[k] = v;
    }
}

// Ray queries on a prepared scene (spt_scene_query_async): kernels of their
// own over the sphere loops and the walks of spt_walk.h; render_kernel does
// not use them.
#include "spt_query.h"

// Radiance queries (spt_scene_radiance_async): the estimator along the
// caller's rays, one path per lane over the same loops and walks.
#include "spt_radiance.h"

// Pixel lists (spt_scene_render_pixels_async): the camera's rays through the
// same estimator for the pixels the caller lists, a sample count per entry.
#include "spt_pixels.h"

// The sample plan (spt_frame_plan_async): colours, second moments and sample
// counts into the next pixel list, in three stream-ordered launches.
#include "spt_plan.h"

}  // namespace smallpt
}  // namespace rt

// ------------------------------------------------------------------ host side
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <mutex>
#include <string>
#include <vector>
#include "rt_runtime.h"
#include <memory>
#include "spt_bvh.h"
#include "spt_refit.h"
#include "spt_move.h"
#include "spt_regroup.h"
#include "spt_sched.h"

using sptpolicy::Shape;

// What spt_scene_regroup_async adds, built at the first regroup: the launch
// plan (sptregroup::Plan), Topo's and the plan's ints on the device, and the
// sort's scratch (a key and an id per tree entry).
struct SceneRegroup {
    sptregroup::Plan plan;
    int *d_ints = nullptr;             // left | right | axis | wpos | sub | desc
    uint32_t *d_scratch = nullptr;     // nb keys, then nb ids
    uint64_t regroups = 0, bytes = 0;
    ~SceneRegroup()
    {
        if (d_ints) (void)hipFree(d_ints);
        if (d_scratch) (void)hipFree(d_scratch);
    }
};

// What spt_scene_update_async keeps with a scene, built at the first update (a
// scene that is never updated has none): the frozen topology of the hierarchy
// on the host and on the device (sptrefit::Meta), the refit kernels' scratch,
// the light indices, and two page-locked staging slots, so that the caller's
// array is free when the call returns and no update waits for the one before it.
struct SceneRefit {
    static constexpr int SLOTS = 2;
    sptrefit::Meta meta;
    sptregroup::Topo topo;             // the children and axes beside meta (host only until a regroup)
    std::unique_ptr<SceneRegroup> regroup;   // null until the first regroup
    int *d_meta = nullptr;             // range | pos | order | wslot
    float *d_scratch = nullptr;        // entry boxes (six planes of nb floats, padded to 16 B), then two float4 per node
    int *d_lights = nullptr;           // light indices, ascending (n ints)
    char *h_stage[SLOTS] = {};         // the changed spheres, then (at 44 n) the light indices
    hipEvent_t done[SLOTS] = {};       // recorded behind the copies out of a slot
    bool used[SLOTS] = {};
    int next = 0;
    int light_cap = 1;                 // light records d_soa has room for
    bool boxes_valid = false;          // the entry boxes hold the whole scene (after the first refit)
    bool lights_valid = false;         // d_lights holds the light list (an update that touched an emitter, or move_prepare)
    uint64_t updates = 0, refits = 0, light_rebuilds = 0, reallocs = 0, meta_bytes = 0;
    uint64_t moves = 0, moves_captured = 0, move_refits = 0;   // spt_scene_move_async's (spt_scene_move_info)
    ~SceneRefit()
    {
        if (d_meta) (void)hipFree(d_meta);
        if (d_scratch) (void)hipFree(d_scratch);
        if (d_lights) (void)hipFree(d_lights);
        for (int k = 0; k < SLOTS; k++) {
            if (h_stage[k]) (void)hipHostFree(h_stage[k]);
            if (done[k]) (void)hipEventDestroy(done[k]);
        }
    }
};

// A prepared scene (spt_scene_create): device AoS copy for the per-block LDS
// staging, device SoA + light list for scenes above the LDS budget.
struct spt_scene {
    int device = -1;
    int cus = 256;
    int n = 0;
    rt_sphere *d_spheres = nullptr;   // n x 44 B
    float4 *d_soa = nullptr;          // geo | emi | col (n each) | light records (3 per light)
    int nlights = 0;
    void *d_bvh = nullptr;            // nodes | geo | id | always geo | always id | wide nodes (large scenes)
    rt::smallpt::BvhView bvh = {};
    // The spheres as the host last gave them (spt_scene_create, then every
    // spt_scene_update_async).  After a spt_scene_move_async the centres and
    // radii of the moved spheres are stale here -- the device's AoS array is
    // the scene (spt_scene_read_spheres) -- while e, c and refl stay exact:
    // only the host edits them.  Readers: refit_prepare runs the builders on
    // it, and runs before the first move is enqueued (a move prepares the
    // scene first), while this still is the scene as created; the update's
    // light list and no_refr read e and refl alone.  Nothing else reads it
    // (the scene caches of spt_render_async and spt_render_multi compare the
    // caller's array with copies of their own, and their scenes are never moved).
    std::vector<rt_sphere> host;
    bool force_global = false;        // RT_SPT_GEO=global: scalar-load path at any size (A/B)
    mutable sptsched::SptSched sched;       // adaptive group order (hierarchy scenes)
    mutable sptsched::SptSched sched_cnt;   //   ... of the full-counter launches (their own tile costs)
    mutable sptsched::WorkRing work;  // work counters of the persistent (8-wide hierarchy) launches
    bool no_refr = false;             // no sphere has refl == REFR (render_kernel's sflags)
    int leaf_max = 0;                 // the 8-wide tree's leaf size (sptbvh::choose_wide; 0: no wide tree)
    // The most recent launch (written on the host by launch(), read by spt_scene_info).
    struct LastLaunch { int count = 0, wpb = 0, nblocks = 0, cg = 0, n1 = 0, n2 = 0, dual = 0, lds = 0; };
    mutable LastLaunch last;
    std::unique_ptr<SceneRefit> refit; // the edits' state (null until the first update, regroup or move_prepare)
};

namespace {
using namespace sptlayout;

// One render call, as the entry points receive it: rows [r0, r1) (every
// gstride-th 8-row group), or (list) the caller's nlist tile groups over the
// whole frame, with their costs recorded into `cost` if given.
struct RenderCall {
    const rt_camera *cam;
    float *colors;
    const uint32_t *seeds_in;
    uint32_t *seeds_out, *pixels;
    int w, h, r0, r1, gstride, first_sample, nsamples, mode;
    unsigned long long *counters;
    hipStream_t stream;
    const int *list = nullptr;
    int nlist = 0;
    unsigned *cost = nullptr;
};

// The counter mode of a call (spt_layout.h: none, all four, calls and samples).
int counter_mode(const RenderCall &c)
{
    return !c.counters ? CNT_NONE : (c.mode & SPT_COUNT_RAYS) ? CNT_RAYS : CNT_FULL;
}

// The kernel family of a scene: the 8-wide tree, the binary one, the
// per-block LDS copy if the scene fits, else global memory.
int scene_geo(const spt_scene &sc)
{
    static_assert(GEO_LDS == SPT_GEO_LDS && GEO_GLOBAL == SPT_GEO_GLOBAL && GEO_BVH == SPT_GEO_BVH &&
                  GEO_WIDE == SPT_GEO_WIDE, "rt_hip.h's family codes (spt_scene_info)");
    if (sc.bvh.wnode) return GEO_WIDE;
    if (sc.bvh.node) return GEO_BVH;
    return (scene_bytes(sc.n, sc.nlights) <= MAX_LDS_BYTES && !sc.force_global) ? GEO_LDS : GEO_GLOBAL;
}

// Whether a launch runs the two-query iteration (one_light: the scene has
// exactly one light).
bool two_query_form(int geo, bool dl, bool one_light)
{
    // The two-query iteration for path tracing in single-light scenes, at
    // every launch shape: one iteration per lit DIFF vertex instead of two.
    // Once the one-query kernel's copies were gone (hit aliasing ray.o, path
    // state reset at sample end) it fits 72 VGPRs at occupancy 7 and beats
    // the one-query form both where per-wave ILP is short (N = 8 band) and on
    // the full frame (17.98 -> 17.3 ms).  RT_SPT_DUAL=0 / 1 forces it off / on (A/B).
    // (The hierarchy walks keep the one-query form: their two resumable
    // walks in one loop spill)
    const int dual_env = getenv("RT_SPT_DUAL") ? atoi(getenv("RT_SPT_DUAL")) : -1;
    return one_light && dual_env != 0 && !dl && (geo == GEO_LDS || geo == GEO_GLOBAL);
}

// The variant of a launch of call c in blocks of wpb waves: the scene's
// family (the LDS family only while the block fits a CU's LDS: launch_geo),
// the estimator, the counter mode, two_query_form's answer, and cg, the lanes
// per pixel of the launch's cooperative tier (8-wide kernels; 0: none -- the
// kernel carries the cooperative walk only when the launch has such a tier,
// and only the group size it uses).
Variant launch_variant(const spt_scene &sc, const RenderCall &c, const SceneSizes &sizes, int wpb, int cg)
{
    const bool dl = (c.mode & ~(SPT_COUNT_RAYS | SPT_COST_MAX)) == SPT_DIRECT_LIGHTING;
    Variant v{scene_geo(sc), dl, false, counter_mode(c), cg};
    v.dual = two_query_form(v.geo, dl, sc.nlights == 1);
    v.geo = launch_geo(v, sizes, wpb);
    return v;
}

// The render_kernel instantiation of a variant: every one has the same
// signature, so the variant's fields become template arguments here and
// nowhere else.
using Kernel = decltype(&rt::smallpt::render_kernel<false, false, 0>);

template <bool DL, bool COUNT, int GEO, bool DUAL, bool RAYS>
Kernel pick_cg(const Variant &v)
{
    Kernel kern = rt::smallpt::render_kernel<DL, COUNT, GEO, DUAL, RAYS, 0>;
    if constexpr (GEO == GEO_WIDE) {
        if (v.cg == 8) kern = rt::smallpt::render_kernel<DL, COUNT, GEO, DUAL, RAYS, 8>;
        else if (v.cg == 4) kern = rt::smallpt::render_kernel<DL, COUNT, GEO, DUAL, RAYS, 4>;
        else if (v.cg == 2) kern = rt::smallpt::render_kernel<DL, COUNT, GEO, DUAL, RAYS, 2>;
    }
    return kern;
}

template <int GEO, bool DL, bool DUAL>
Kernel pick_counted(const Variant &v)
{
    if (v.count()) return pick_cg<DL, true, GEO, DUAL, false>(v);
    if (v.rays()) return pick_cg<DL, false, GEO, DUAL, true>(v);
    return pick_cg<DL, false, GEO, DUAL, false>(v);
}

template <int GEO>
Kernel pick_mode(const Variant &v)
{
    if (v.dl) return pick_counted<GEO, true, false>(v);
    if constexpr (GEO != GEO_BVH && GEO != GEO_WIDE) {
        if (v.dual) return pick_counted<GEO, false, true>(v);
    }
    return pick_counted<GEO, false, false>(v);
}

Kernel pick_kernel(const Variant &v)
{
    if (v.geo == GEO_WIDE) return pick_mode<GEO_WIDE>(v);
    if (v.geo == GEO_BVH) return pick_mode<GEO_BVH>(v);
    if (v.geo == GEO_LDS) return pick_mode<GEO_LDS>(v);
    return pick_mode<GEO_GLOBAL>(v);
}

// Launches render_kernel for call c in shape g: the variant and its LDS size
// (spt_layout.h), the work counters of a persistent launch and the packed
// words of spt_policy.h.
int launch(const spt_scene &sc, const RenderCall &c, const Shape &g)
{
    const int n = sc.n;
    const float4 *gg = sc.d_soa, *ge = gg + n, *gc = ge + n, *gl = gc + n;
    const sptpolicy::Tiers t = sptpolicy::heavy_tiers(g, sc.cus);
    const SceneSizes sizes{n, sc.nlights, sc.bvh.wnodes, sc.bvh.wdepth};
    const Variant v = launch_variant(sc, c, sizes, g.wpb, t.cg);
    const size_t lds = block_lds_bytes(v, sizes, g.wpb);
    int *work = nullptr;
    if (v.persist() && !(work = sptsched::work_entry(sc.work, c.stream)))
        return rtrt::check_launch("spt work counters") ? RT_ERR_HIP : RT_ERR_INVALID;
    sc.last = {sc.last.count + 1, g.wpb, g.nblocks, t.cg, t.n1, t.n2, v.dual ? 1 : 0, (int)lds};
    hipLaunchKernelGGL(pick_kernel(v), dim3(g.nblocks), dim3(64 * g.wpb), lds, c.stream, sc.d_spheres, n, *c.cam,
                       c.colors, c.seeds_in, c.seeds_out, c.pixels, c.w, c.h, c.r0, c.r1, g.tiles_x, g.ntiles, g.nslots,
                       g.gstride, c.first_sample, c.nsamples, sptpolicy::prio_schedule(g), g.order, g.cost, gg, ge, gc,
                       gl, sc.nlights, sc.bvh, c.counters, work, v.persist() ? sptpolicy::split_word(g, t) : 0,
                       sptpolicy::pack_nheavy(t.n1, t.n2),
                       sptpolicy::pack_sflags(sc.no_refr, g.cost_max, v.dq() ? sptpolicy::sq_threshold(g.tune.sq) : 0));
    if (work) sptsched::work_launched(sc.work, work, c.stream);
    return RT_OK;
}

// ---- hierarchy build (host, spt_bvh.h) for scenes of >= sptbvh::MIN_SPHERES spheres
// Builds the hierarchy into sc->d_bvh / sc->bvh (nothing for small scenes):
// the binary tree's eight octant layouts and, when a block's LDS can hold it
// (two blocks of WIDE_WPB waves per CU), the 8-wide layout -- with the
// smallest leaf size in {8, 12, 16} whose tree fits.
int build_scene_bvh(spt_scene *sc, const rt_sphere *spheres)
{
    const int n = sc->n;
    if (n < sptbvh::MIN_SPHERES || getenv("RT_SPT_NO_BVH")) return RT_OK;
    std::vector<int> always;
    sptbvh::BvhBuild b;
    sptbvh::partition_and_build(spheres, n, always, b);
    const int nn = (int)b.nodes.size(), nb = (int)b.idx.size(), na = (int)always.size();
    // Eight layouts (one per direction octant), each with layout-local links.
    std::vector<sptbvh::f4> nodes;
    nodes.reserve(2 * (size_t)nn * 8);
    for (int oct = 0; oct < 8; oct++) {
        std::vector<sptbvh::f4> lay;
        lay.reserve(2 * (size_t)nn);
        if (nn) b.emit(0, oct, lay);
        nodes.insert(nodes.end(), lay.begin(), lay.end());
    }
    sptbvh::WideBuild wb;
    const char *we = getenv("RT_SPT_WIDE");             // 0: the binary walk only (A/B, tests)
    if (!(we && atoi(we) == 0)) sc->leaf_max = sptbvh::choose_wide(b, wb, sptpolicy::WIDE_WPB);
    const bool wide = sc->leaf_max != 0;
    std::vector<float4> geo(nb + na);
    std::vector<int> ids(nb + na);
    for (int j = 0; j < nb + na; j++) {
        const int i = j < nb ? b.idx[j] : always[j - nb];
        const rt_sphere &q = spheres[i];
        geo[j] = make_float4(q.p.x, q.p.y, q.p.z, q.rad * q.rad);     // geomfunc.h:42 product
        ids[j] = i;
    }
    const size_t nb_bytes = sizeof(float4) * nodes.size(), g_bytes = sizeof(float4) * geo.size(),
                 i_bytes = sizeof(int) * ids.size(), w_bytes = wide ? 4 * wb.words.size() : 0,
                 m_bytes = wide ? 4 * wb.maxid.size() : 0;
    const size_t w_off = (nb_bytes + g_bytes + i_bytes + 15) & ~(size_t)15;
    hipError_t e = hipMalloc(&sc->d_bvh, w_off + w_bytes + m_bytes + 16);
    char *base = (char *)sc->d_bvh;
    if (e == hipSuccess) e = hipMemcpy(base, nodes.data(), nb_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + nb_bytes, geo.data(), g_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(base + nb_bytes + g_bytes, ids.data(), i_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && wide) e = hipMemcpy(base + w_off, wb.words.data(), w_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && wide)
        e = hipMemcpy(base + w_off + w_bytes, wb.maxid.data(), m_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && wide) e = sptsched::ring_create(sc->work);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_create hierarchy upload");
    rt::smallpt::BvhView &v = sc->bvh;
    v.node = (const float4 *)base;
    v.geo = (const float4 *)(base + nb_bytes);
    v.id = (const int *)(base + nb_bytes + g_bytes);
    v.ageo = v.geo + nb;
    v.aid = v.id + nb;
    v.nalways = na;
    v.nnodes = nn;
    v.wnode = wide ? (const uint4 *)(base + w_off) : nullptr;
    v.wmax = wide ? (const uint4 *)(base + w_off + w_bytes) : nullptr;
    v.wnodes = wide ? wb.nnodes : 0;
    v.wdepth = wide ? wb.depth : 0;
    return RT_OK;
}

int check_render_args(const rt_camera *camera, float *d_colors, const uint32_t *d_seeds_in,
                      uint32_t *d_seeds_out, uint32_t *d_pixels, int w, int h, int row_begin, int row_end,
                      int first_sample, int nsamples, int mode)
{
    if (!camera || !d_colors || !d_seeds_in || !d_seeds_out || !d_pixels)
        return rtrt::fail(RT_ERR_INVALID, "spt render: null pointer");
    if (w < 1 || h < 1 || first_sample < 0 || nsamples < 0)
        return rtrt::fail(RT_ERR_INVALID, "spt render: bad sizes");
    if (row_begin < 0 || row_end > h || row_begin > row_end)
        return rtrt::fail(RT_ERR_INVALID, "spt render: bad row range");
    const int base = mode & ~(SPT_COUNT_RAYS | SPT_COST_MAX);
    if (base != SPT_PATH_TRACING && base != SPT_DIRECT_LIGHTING)
        return rtrt::fail(RT_ERR_INVALID, "spt render: bad mode");
    return RT_OK;
}

}  // namespace

extern "C" int spt_scene_create(const rt_sphere *spheres, unsigned nspheres, spt_scene **out)
{
    if (!spheres || !out || nspheres < 1 || nspheres > (1u << 24))
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_create: bad arguments");
    rtrt::DeviceState *st;
    int rc = rtrt::state(&st);
    if (rc) return rc;
    spt_scene *sc = new spt_scene();
    sc->device = st->device;
    if (st->cus > 0) sc->cus = st->cus;
    sc->n = (int)nspheres;
    sc->host.assign(spheres, spheres + nspheres);
    const char *geo_env = getenv("RT_SPT_GEO");
    sc->force_global = geo_env && !strcmp(geo_env, "global");
    const int n = sc->n;
    std::vector<float4> soa((size_t)3 * n);
    std::vector<int> lights;
    for (int i = 0; i < n; i++) {
        const rt_sphere &q = spheres[i];
        soa[i] = make_float4(q.p.x, q.p.y, q.p.z, q.rad * q.rad);
        int refl = q.refl;
        float frefl;
        memcpy(&frefl, &refl, 4);
        soa[n + i] = make_float4(q.e.x, q.e.y, q.e.z, frefl);
        soa[2 * (size_t)n + i] = make_float4(q.c.x, q.c.y, q.c.z, q.rad);
        if (!((q.e.x == 0.f) && (q.e.x == 0.f) && (q.e.z == 0.f))) lights.push_back(i);  // vec.h:44
    }
    sc->nlights = (int)lights.size();
    // render_kernel's branch order (geomfunc.h:223-281): an emitter (the
    // viszero test of vec.h:44, x tested twice) ends the path, then refl ==
    // DIFF, refl == SPEC, and EVERY other refl value takes the REFR branch
    // (:281 `else`) -- refl 2, but also 3 or -1.  Only a scene whose every
    // non-emitter is DIFF or SPEC may skip the refraction terms.
    sc->no_refr = std::all_of(spheres, spheres + nspheres, [](const rt_sphere &q) {
        const bool emitter = !((q.e.x == 0.f) && (q.e.x == 0.f) && (q.e.z == 0.f));
        return emitter || q.refl == 0 || q.refl == 1;
    });
    if (lights.empty())                    // one zero record (render_kernel loads light 0 unconditionally)
        soa.insert(soa.end(), 3, make_float4(0.f, 0.f, 0.f, 0.f));
    for (int i : lights) {                 // light records: geo, col, emi of each light, ascending
        const float4 g = soa[i], c = soa[2 * (size_t)n + i], e = soa[(size_t)n + i];
        soa.push_back(g);
        soa.push_back(c);
        soa.push_back(e);
    }
    hipError_t e = hipMalloc(&sc->d_spheres, sizeof(rt_sphere) * n);
    if (e == hipSuccess) e = hipMalloc(&sc->d_soa, sizeof(float4) * soa.size());
    if (e == hipSuccess) e = hipMemcpy(sc->d_spheres, spheres, sizeof(rt_sphere) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(sc->d_soa, soa.data(), sizeof(float4) * soa.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (sc->d_spheres) (void)hipFree(sc->d_spheres);
        if (sc->d_soa) (void)hipFree(sc->d_soa);
        delete sc;
        return rtrt::fail_hip(e, "spt_scene_create upload");
    }
    if ((rc = build_scene_bvh(sc, spheres))) {
        spt_scene_destroy(sc);
        return rc;
    }
    *out = sc;
    return RT_OK;
}

extern "C" int spt_scene_destroy(spt_scene *sc)
{
    if (!sc) return RT_OK;
    (void)hipSetDevice(sc->device);
    (void)hipDeviceSynchronize();
    if (sc->d_spheres) (void)hipFree(sc->d_spheres);
    if (sc->d_soa) (void)hipFree(sc->d_soa);
    if (sc->d_bvh) (void)hipFree(sc->d_bvh);
    sptsched::ring_release(sc->work);
    sptsched::sched_release(sc->sched);
    sptsched::sched_release(sc->sched_cnt);
    delete sc;
    return RT_OK;
}

extern "C" int spt_scene_info(const spt_scene *sc, int *out, int nout)
{
    if (!sc || !out || nout < 1) return rtrt::fail(RT_ERR_INVALID, "spt_scene_info: bad arguments");
    const spt_scene::LastLaunch &l = sc->last;
    const int v[SPT_INFO_WORDS] = {scene_geo(*sc), sc->n, sc->nlights, sc->bvh.nalways, sc->bvh.nnodes,
                                   sc->bvh.wnodes, sc->bvh.wdepth, sc->leaf_max, sc->no_refr ? 1 : 0, l.count,
                                   l.wpb, l.nblocks, l.cg, l.n1, l.n2, l.dual, l.lds};
    std::copy(v, v + std::min(nout, (int)SPT_INFO_WORDS), out);
    return RT_OK;
}

extern "C" int spt_scene_release_captures(const spt_scene *sc)
{
    if (!sc) return rtrt::fail(RT_ERR_INVALID, "spt_scene_release_captures: null scene");
    std::lock_guard<std::mutex> lk(sc->work.mu);
    sc->work.book.captured = 0;
    return RT_OK;
}

// ---- in-place update (spt_refit.h)
namespace {

// vec.h:44 viszero, x tested twice: spt_scene_create's rule for a light.
bool is_emitter(const rt_sphere &q) { return !((q.e.x == 0.f) && (q.e.x == 0.f) && (q.e.z == 0.f)); }

// The first update of a scene: staging slots, the light index array and, for
// a hierarchy scene, the topology.  The builders run once more on the scene
// as it was created (sc->host still is that scene; they are deterministic), so
// spt_scene_create keeps nothing for a scene that is never updated.
int refit_prepare(spt_scene *sc)
{
    std::unique_ptr<SceneRefit> r(new SceneRefit());
    const int n = sc->n;
    hipError_t e = hipSuccess;
    for (int k = 0; k < SceneRefit::SLOTS && e == hipSuccess; k++) {
        e = hipHostMalloc((void **)&r->h_stage[k], (sizeof(rt_sphere) + sizeof(int)) * (size_t)n, hipHostMallocDefault);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&r->done[k], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipMalloc(&r->d_lights, sizeof(int) * (size_t)n);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_update_async staging");
    r->light_cap = std::max(1, sc->nlights);
    if (sc->bvh.node) {
        std::vector<int> always;
        sptbvh::BvhBuild b;
        sptbvh::partition_and_build(sc->host.data(), n, always, b);
        sptbvh::WideBuild wb;
        if (sc->leaf_max) {
            wb.leaf_max = sc->leaf_max;
            wb.build(b);
        }
        sptrefit::Meta &m = r->meta;
        if ((int)b.nodes.size() != sc->bvh.nnodes || (int)always.size() != sc->bvh.nalways ||
            (sc->leaf_max ? wb.nnodes : 0) != sc->bvh.wnodes ||
            !sptrefit::build_meta(b, (int)always.size(), sc->leaf_max ? wb.words.data() : nullptr, wb.nnodes, m))
            return rtrt::fail(RT_ERR_INVALID, "spt_scene_update_async: the scene's topology cannot be rebuilt");
        sptregroup::build_topo(b, m, r->topo);
        std::vector<int> ints;
        ints.reserve(m.ints());
        for (const std::vector<int> *v : {&m.range, &m.pos, &m.order, &m.wslot}) ints.insert(ints.end(), v->begin(), v->end());
        const size_t planes = (6 * (size_t)m.nb + 3) & ~(size_t)3;
        e = hipMalloc(&r->d_meta, sizeof(int) * ints.size());
        if (e == hipSuccess) e = hipMalloc(&r->d_scratch, sizeof(float) * (planes + 8 * (size_t)m.nn));
        if (e == hipSuccess) e = hipMemcpy(r->d_meta, ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_update_async metadata upload");
        r->meta_bytes = sizeof(int) * ints.size() + sizeof(float) * (6 * (size_t)m.nb + 8 * (size_t)m.nn);
    }
    sc->refit = std::move(r);
    return RT_OK;
}

// The device views the refit kernels take.
sptrefit::DevRefit refit_view(const spt_scene &sc)
{
    const SceneRefit &r = *sc.refit;
    const sptrefit::Meta &m = r.meta;
    sptrefit::DevRefit v = {};
    v.spheres = sc.d_spheres;
    v.soa = sc.d_soa;
    v.n = sc.n;
    if (!sc.bvh.node) return v;
    v.nodes = const_cast<float4 *>(sc.bvh.node);
    v.geo = const_cast<float4 *>(sc.bvh.geo);
    v.ids = sc.bvh.id;
    v.wwords = (uint32_t *)const_cast<uint4 *>(sc.bvh.wnode);
    v.nn = m.nn; v.nb = m.nb; v.na = m.na; v.wn = m.wn;
    v.range = r.d_meta;
    v.pos = v.range + m.range.size();
    v.order = v.pos + m.pos.size();
    v.wslot = v.order + m.order.size();
    v.n_small = m.n_small; v.n_wave = m.n_wave; v.n_block = m.n_block;
    v.box = r.d_scratch;
    v.nbox = (float4 *)(r.d_scratch + ((6 * (size_t)m.nb + 3) & ~(size_t)3));
    return v;
}

// refit_nodes and (8-wide scenes) refit_wide behind a gather on `s`.
int launch_refit_tree(const sptrefit::DevRefit &v, hipStream_t s)
{
    const int b_small = (v.n_small + 31) / 32, b_wave = (v.n_wave + 3) / 4;
    hipLaunchKernelGGL(sptrefit::refit_nodes, dim3(b_small + b_wave + v.n_block), dim3(256), 0, s, v, b_small, b_wave);
    int rc = rtrt::check_launch("spt refit_nodes");
    if (rc == RT_OK && v.wwords) {
        hipLaunchKernelGGL(sptrefit::refit_wide, dim3((8 * v.wn + 255) / 256), dim3(256), 0, s, v);
        rc = rtrt::check_launch("spt refit_wide");
    }
    return rc;
}

// What a move needs of a scene beyond refit_prepare: the light index array on
// the device, and entry boxes that hold the whole scene.
bool move_ready(const spt_scene &sc)
{
    return sc.refit && sc.refit->lights_valid && (!sc.bvh.node || sc.refit->boxes_valid);
}

// Builds the parts of that which are missing (spt_scene_move_prepare; not on a
// capturing stream).  Allocates and waits for `s`.
int move_prepare(spt_scene *sc, hipStream_t s, const char *who)
{
    int rc;
    if (!sc->refit && (rc = refit_prepare(sc))) return rc;
    SceneRefit &r = *sc->refit;
    if (!r.lights_valid) {
        // e is the host's alone to edit: sc->host names the emitters whatever moved
        std::vector<int> lights;
        for (int i = 0; i < sc->n; i++)
            if (is_emitter(sc->host[i])) lights.push_back(i);
        hipError_t e = hipSuccess;
        if (!lights.empty())
            e = hipMemcpyAsync(r.d_lights, lights.data(), sizeof(int) * lights.size(), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);    // (`lights` is pageable and ends with this scope)
        if (e != hipSuccess) return rtrt::fail_hip(e, who);
        r.lights_valid = true;
    }
    if (sc->bvh.node && !r.boxes_valid) {
        // the whole scene's entry boxes (and geo) from the AoS array, as a regroup's refit takes them
        const sptrefit::DevRefit v = refit_view(*sc);
        hipLaunchKernelGGL(sptrefit::refit_gather, dim3((v.nb + v.na + 255) / 256), dim3(256), 0, s, v, 0, 0, 0, sc->n,
                           (const int *)nullptr, 0, 0);
        rc = rtrt::check_launch("spt refit_gather");
        if (rc == RT_OK) rc = launch_refit_tree(v, s);
        if (rc != RT_OK) return rc;
        r.boxes_valid = true;
    }
    return RT_OK;
}

}  // namespace

extern "C" int spt_scene_update_async(spt_scene *sc, const rt_sphere *spheres, unsigned first, unsigned count,
                                      void *stream)
{
    if (!sc || !spheres) return rtrt::fail(RT_ERR_INVALID, "spt_scene_update_async: null pointer");
    if (first > (unsigned)sc->n || count > (unsigned)sc->n - first)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_update_async: range out of bounds");
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(s, &cap);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_update_async stream");
    if (cap != hipStreamCaptureStatusNone)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_update_async: the stream is capturing");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_update_async: the scene's device is not the current one");
    if (count == 0) return RT_OK;
    int rc;
    if (!sc->refit && (rc = refit_prepare(sc))) return rc;
    SceneRefit &r = *sc->refit;
    const int n = sc->n;

    // The light list and no_refr of the edited scene, by spt_scene_create's
    // rules -- the list only if the range held or holds an emitter.
    bool lights_touched = false;
    for (unsigned i = 0; i < count; i++)
        lights_touched = lights_touched || is_emitter(sc->host[first + i]) || is_emitter(spheres[i]);
    const int slot = r.next;
    if (r.used[slot] && (e = hipEventSynchronize(r.done[slot])) != hipSuccess)   // (the update two calls back: long done)
        return rtrt::fail_hip(e, "spt_scene_update_async staging wait");
    rt_sphere *h_sp = (rt_sphere *)r.h_stage[slot];
    int *h_lights = (int *)(r.h_stage[slot] + sizeof(rt_sphere) * (size_t)n);
    std::copy(spheres, spheres + count, h_sp);
    std::copy(spheres, spheres + count, sc->host.begin() + first);
    int nl = sc->nlights;
    if (lights_touched) {
        nl = 0;
        for (int i = 0; i < n; i++)
            if (is_emitter(sc->host[i])) h_lights[nl++] = i;
    }
    sc->no_refr = std::all_of(sc->host.begin(), sc->host.end(), [](const rt_sphere &q) {
        return is_emitter(q) || q.refl == 0 || q.refl == 1;
    });
    if (nl > r.light_cap) {
        // More lights than d_soa has records for: a larger array.  The one
        // path that synchronises (launches on other streams may still read
        // the old array, and hipFree waits for them).
        const int cap2 = std::max(nl, 2 * r.light_cap);
        float4 *soa2 = nullptr;
        e = hipMalloc(&soa2, sizeof(float4) * (3 * (size_t)n + 3 * (size_t)cap2));
        if (e == hipSuccess) e = hipMemcpyAsync(soa2, sc->d_soa, sizeof(float4) * 3 * (size_t)n, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e == hipSuccess) e = hipFree(sc->d_soa);
        if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_update_async light records");
        sc->d_soa = soa2;
        r.light_cap = cap2;
        r.reallocs++;
    }
    sc->nlights = nl;

    e = hipMemcpyAsync(sc->d_spheres + first, h_sp, sizeof(rt_sphere) * (size_t)count, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && lights_touched && nl)
        e = hipMemcpyAsync(r.d_lights, h_lights, sizeof(int) * (size_t)nl, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_update_async copy");
    if (lights_touched) r.lights_valid = true;           // (no light left: nothing reads the array)
    const sptrefit::DevRefit v = refit_view(*sc);
    const bool tree = v.nodes != nullptr;
    const int nrec = lights_touched ? std::max(1, nl) : 0;
    // entry boxes: the whole scene at the first refit, the changed range after it
    const int efirst = r.boxes_valid ? (int)first : 0, ecount = r.boxes_valid ? (int)count : n;
    const int lanes = std::max({(int)count, tree ? v.nb + v.na : 0, nrec});
    hipLaunchKernelGGL(sptrefit::refit_gather, dim3((lanes + 255) / 256), dim3(256), 0, s, v, (int)first, (int)count,
                       efirst, ecount, r.d_lights, nl, nrec);
    rc = rtrt::check_launch("spt refit_gather");
    if (rc == RT_OK && tree) {
        rc = launch_refit_tree(v, s);
        if (rc == RT_OK) {
            r.boxes_valid = true;
            r.refits++;
        }
    }
    e = hipEventRecord(r.done[slot], s);
    if (rc == RT_OK && e != hipSuccess) rc = rtrt::fail_hip(e, "spt_scene_update_async record");
    r.used[slot] = true;
    r.next = (slot + 1) % SceneRefit::SLOTS;
    if (rc == RT_OK) {
        r.updates++;
        if (lights_touched) r.light_rebuilds++;
    }
    return rc;
}

extern "C" int spt_scene_update_info(const spt_scene *sc, uint64_t *out, int nout)
{
    if (!sc || !out || nout < 1) return rtrt::fail(RT_ERR_INVALID, "spt_scene_update_info: bad arguments");
    const SceneRefit *r = sc->refit.get();
    const uint64_t v[SPT_UPDATE_INFO_WORDS] = {r ? r->updates : 0, r ? r->refits : 0, r ? r->light_rebuilds : 0,
                                               r ? r->reallocs : 0, r ? r->meta_bytes : 0};
    std::copy(v, v + std::min(nout, (int)SPT_UPDATE_INFO_WORDS), out);
    return RT_OK;
}

// ---- geometry from device memory (spt_move.h)
extern "C" int spt_scene_move_prepare(spt_scene *sc, void *stream)
{
    if (!sc) return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_prepare: null scene");
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(s, &cap);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_move_prepare stream");
    if (cap != hipStreamCaptureStatusNone)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_prepare: the stream is capturing");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_prepare: the scene's device is not the current one");
    return move_prepare(sc, s, "spt_scene_move_prepare light indices");
}

extern "C" int spt_scene_move_async(spt_scene *sc, const float *d_geom, unsigned first, unsigned count, void *stream)
{
    if (!sc || !d_geom) return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_async: null pointer");
    if ((uintptr_t)d_geom & 15) return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_async: d_geom is not 16-byte aligned");
    if (first > (unsigned)sc->n || count > (unsigned)sc->n - first)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_async: range out of bounds");
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(s, &cap);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_move_async stream");
    const bool capturing = cap != hipStreamCaptureStatusNone;
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_async: the scene's device is not the current one");
    if (capturing && !move_ready(*sc))
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_async: capture needs spt_scene_move_prepare first");
    if (count == 0) return RT_OK;
    int rc;
    if (!move_ready(*sc) && (rc = move_prepare(sc, s, "spt_scene_move_async light indices"))) return rc;
    SceneRefit &r = *sc->refit;
    // Everything below is by value and fixed while the light list stays: a
    // capture records exactly these launches.
    const sptrefit::DevRefit v = refit_view(*sc);
    const bool tree = v.nodes != nullptr;
    const int lanes = std::max({(int)count, tree ? v.nb + v.na : 0, sc->nlights});
    hipLaunchKernelGGL(sptrefit::move_gather, dim3((lanes + 255) / 256), dim3(256), 0, s, v, (const float4 *)d_geom,
                       (int)first, (int)count, r.d_lights, sc->nlights);
    rc = rtrt::check_launch("spt move_gather");
    if (rc == RT_OK && tree) {
        rc = launch_refit_tree(v, s);
        if (rc == RT_OK) r.move_refits++;
    }
    if (rc == RT_OK) {
        r.moves++;
        if (capturing) r.moves_captured++;
    }
    return rc;
}

extern "C" int spt_scene_move_info(const spt_scene *sc, uint64_t *out, int nout)
{
    if (!sc || !out || nout < 1) return rtrt::fail(RT_ERR_INVALID, "spt_scene_move_info: bad arguments");
    const SceneRefit *r = sc->refit.get();
    const uint64_t v[SPT_MOVE_INFO_WORDS] = {r ? r->moves : 0, r ? r->moves_captured : 0, r ? r->move_refits : 0};
    std::copy(v, v + std::min(nout, (int)SPT_MOVE_INFO_WORDS), out);
    return RT_OK;
}

extern "C" int spt_scene_read_spheres(const spt_scene *sc, rt_sphere *out, unsigned cap)
{
    if (!sc || !out) return rtrt::fail(RT_ERR_INVALID, "spt_scene_read_spheres: null pointer");
    if (cap < (unsigned)sc->n) return rtrt::fail(RT_ERR_INVALID, "spt_scene_read_spheres: buffer too small");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_read_spheres: the scene's device is not the current one");
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, sc->d_spheres, sizeof(rt_sphere) * (size_t)sc->n, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_read_spheres");
    return RT_OK;
}

// ---- regroup (spt_regroup.h)
namespace {

// The first regroup of a scene: the launch plan, Topo's and the plan's ints on
// the device, the sort's scratch.  RT_SPT_REGROUP_LDS=<entries>: the largest
// subtree the LDS tier takes (A/B; 0: no LDS tier, every tree level sorted by
// passes of its own; at most SUB_MAX).
int regroup_prepare(spt_scene *sc)
{
    SceneRefit &r = *sc->refit;
    std::unique_ptr<SceneRegroup> g(new SceneRegroup());
    const char *le = getenv("RT_SPT_REGROUP_LDS");
    const int sub_max = le ? std::min(std::max(atoi(le), 0), sptregroup::SUB_MAX) : sptregroup::SUB_DEFAULT;
    sptregroup::build_plan(r.meta, r.topo, sub_max, g->plan);
    std::vector<int> ints;
    for (const std::vector<int> *v : {&r.topo.left, &r.topo.right, &r.topo.axis, &r.topo.wpos, &g->plan.sub, &g->plan.desc})
        ints.insert(ints.end(), v->begin(), v->end());
    hipError_t e = hipMalloc(&g->d_ints, sizeof(int) * ints.size());
    if (e == hipSuccess) e = hipMalloc(&g->d_scratch, 2 * sizeof(uint32_t) * (size_t)r.meta.nb);
    if (e == hipSuccess) e = hipMemcpy(g->d_ints, ints.data(), sizeof(int) * ints.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_regroup_async metadata upload");
    g->bytes = sizeof(int) * ints.size() + 2 * sizeof(uint32_t) * (size_t)r.meta.nb;
    r.regroup = std::move(g);
    return RT_OK;
}

}  // namespace

extern "C" int spt_scene_regroup_async(spt_scene *sc, void *stream)
{
    if (!sc) return rtrt::fail(RT_ERR_INVALID, "spt_scene_regroup_async: null scene");
    hipStream_t s = (hipStream_t)stream;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(s, &cap);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_regroup_async stream");
    if (cap != hipStreamCaptureStatusNone)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_regroup_async: the stream is capturing");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_regroup_async: the scene's device is not the current one");
    if (!sc->bvh.node) return RT_OK;
    int rc;
    if (!sc->refit && (rc = refit_prepare(sc))) return rc;
    SceneRefit &r = *sc->refit;
    if (!r.regroup && (rc = regroup_prepare(sc))) return rc;
    SceneRegroup &g = *r.regroup;
    const sptregroup::Plan &p = g.plan;
    const sptrefit::DevRefit v = refit_view(*sc);
    const size_t nn = (size_t)v.nn;
    sptregroup::DevRegroup d = {};
    d.spheres = sc->d_spheres;
    d.ids = const_cast<int *>(sc->bvh.id);
    d.maxid = (uint32_t *)const_cast<uint4 *>(sc->bvh.wmax);
    d.nb = v.nb;
    d.range = v.range; d.order = v.order;
    d.left = g.d_ints; d.right = d.left + nn; d.axis = d.right + nn; d.wpos = d.axis + nn;
    d.n_small = v.n_small; d.n_wave = v.n_wave; d.n_block = v.n_block;
    d.keys = g.d_scratch;
    d.tmp = (int *)(g.d_scratch + v.nb);
    const int2 *sub = (const int2 *)(d.wpos + nn), *desc = sub + p.sub.size() / 2;
    // the levels above the LDS tier, top-down: keys, ranks, copy back
    rc = RT_OK;
    for (size_t l = 0; l < p.lev_count.size() && rc == RT_OK; l++) {
        const dim3 grid(p.lev_count[l]), block(sptregroup::CHUNK);
        hipLaunchKernelGGL(sptregroup::regroup_keys, grid, block, 0, s, d, desc + p.lev_first[l]);
        hipLaunchKernelGGL(sptregroup::regroup_rank, grid, block, 0, s, d, desc + p.lev_first[l]);
        hipLaunchKernelGGL(sptregroup::regroup_copy, grid, block, 0, s, d, desc + p.lev_first[l]);
        rc = rtrt::check_launch("spt regroup level");
    }
    if (rc == RT_OK && !p.sub.empty()) {
        hipLaunchKernelGGL(sptregroup::regroup_subtree, dim3(p.sub.size() / 2), dim3(256), 0, s, d, sub);
        rc = rtrt::check_launch("spt regroup_subtree");
    }
    // ids is final: the whole scene's geo and entry boxes, the refit, the highest-index table
    if (rc == RT_OK) {
        hipLaunchKernelGGL(sptrefit::refit_gather, dim3((v.nb + v.na + 255) / 256), dim3(256), 0, s, v, 0, 0, 0, sc->n,
                           (const int *)nullptr, 0, 0);
        rc = rtrt::check_launch("spt refit_gather");
    }
    if (rc == RT_OK) {
        const int b_small = (v.n_small + 31) / 32, b_wave = (v.n_wave + 3) / 4;
        hipLaunchKernelGGL(sptrefit::refit_nodes, dim3(b_small + b_wave + v.n_block), dim3(256), 0, s, v, b_small, b_wave);
        rc = rtrt::check_launch("spt refit_nodes");
        if (rc == RT_OK && v.wwords) {
            hipLaunchKernelGGL(sptrefit::refit_wide, dim3((8 * v.wn + 255) / 256), dim3(256), 0, s, v);
            hipLaunchKernelGGL(sptregroup::regroup_maxid, dim3(b_small + b_wave + v.n_block), dim3(256), 0, s, d, b_small,
                               b_wave);
            rc = rtrt::check_launch("spt regroup_maxid");
        }
    }
    if (rc == RT_OK) {
        r.boxes_valid = true;
        g.regroups++;
    }
    return rc;
}

extern "C" int spt_scene_regroup_info(const spt_scene *sc, uint64_t *out, int nout)
{
    if (!sc || !out || nout < 1) return rtrt::fail(RT_ERR_INVALID, "spt_scene_regroup_info: bad arguments");
    const SceneRegroup *g = sc->refit ? sc->refit->regroup.get() : nullptr;
    const uint64_t v[SPT_REGROUP_INFO_WORDS] = {g ? g->regroups : 0, g ? (uint64_t)g->plan.levels : 0,
                                                g ? (uint64_t)g->plan.lev_count.size() : 0, g ? g->bytes : 0};
    std::copy(v, v + std::min(nout, (int)SPT_REGROUP_INFO_WORDS), out);
    return RT_OK;
}

extern "C" int spt_scene_read_hierarchy(const spt_scene *sc, void *out, size_t cap, size_t sizes[5])
{
    if (!sc || !sizes) return rtrt::fail(RT_ERR_INVALID, "spt_scene_read_hierarchy: null pointer");
    const rt::smallpt::BvhView &v = sc->bvh;
    for (int k = 0; k < 5; k++) sizes[k] = 0;
    if (!v.node) return RT_OK;
    const char *src[5] = {(const char *)v.node, (const char *)v.geo, (const char *)v.id, (const char *)v.wnode,
                          (const char *)v.wmax};
    sizes[0] = (size_t)(src[1] - src[0]);
    sizes[1] = (size_t)(src[2] - src[1]);
    sizes[2] = sizes[1] / 4;                                  // an int per float4 entry
    sizes[3] = sizeof(uint32_t) * sptbvh::WIDE_WORDS * (size_t)v.wnodes;
    sizes[4] = v.wnode ? sizeof(uint32_t) * sptbvh::WIDE * (size_t)v.wnodes : 0;
    if (!out) return RT_OK;
    if (cap < sizes[0] + sizes[1] + sizes[2] + sizes[3] + sizes[4])
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_read_hierarchy: buffer too small");
    hipError_t e = hipDeviceSynchronize();
    char *dst = (char *)out;
    for (int k = 0; k < 5 && e == hipSuccess; k++) {
        if (sizes[k]) e = hipMemcpy(dst, src[k], sizes[k], hipMemcpyDeviceToHost);
        dst += sizes[k];
    }
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_read_hierarchy");
    return RT_OK;
}

// ---- ray queries (spt_query.h)
namespace {
using QueryKernel = decltype(&rt::smallpt::query_kernel<0, 0>);

template <int GEO>
QueryKernel pick_query(int kind)
{
    if (kind == SPT_QUERY_ANY) return rt::smallpt::query_kernel<GEO, SPT_QUERY_ANY>;
    if (kind == SPT_QUERY_OCCLUDER) return rt::smallpt::query_kernel<GEO, SPT_QUERY_OCCLUDER>;
    return rt::smallpt::query_kernel<GEO, SPT_QUERY_NEAREST>;
}
}  // namespace

extern "C" int spt_scene_query_async(const spt_scene *sc, const float *d_rays, const float *d_tmax, size_t nrays,
                                     int kind, float *d_t, int *d_id, void *stream)
{
    static_assert(rt::smallpt::Q_NEAREST == SPT_QUERY_NEAREST && rt::smallpt::Q_ANY == SPT_QUERY_ANY &&
                  rt::smallpt::Q_OCCLUDER == SPT_QUERY_OCCLUDER, "rt_hip.h's query kinds");
    if (!sc || !d_rays) return rtrt::fail(RT_ERR_INVALID, "spt_scene_query_async: null scene or rays");
    if (kind != SPT_QUERY_NEAREST && kind != SPT_QUERY_ANY && kind != SPT_QUERY_OCCLUDER)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_query_async: unknown kind");
    if (!d_t && !d_id) return rtrt::fail(RT_ERR_INVALID, "spt_scene_query_async: no output");
    if (kind != SPT_QUERY_NEAREST && (!d_tmax || !d_id))
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_query_async: an occlusion query needs d_tmax and d_id");
    if (nrays > (size_t)INT32_MAX) return rtrt::fail(RT_ERR_INVALID, "spt_scene_query_async: too many rays");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_query_async: the scene's device is not the current one");
    if (nrays == 0) return RT_OK;
    // The family rendering picks (scene_geo); the LDS family always fits here
    // (the geo records alone: a third of the scene copy it was admitted by).
    const int geo = scene_geo(*sc);
    const bool counted = kind == SPT_QUERY_OCCLUDER;
    const SceneSizes sizes{sc->n, sc->nlights, sc->bvh.wnodes, sc->bvh.wdepth};
    const size_t lds = query_lds_bytes(geo, sizes, counted);
    const int wpb = query_wpb(geo);
    // Persistent blocks: one per CU for the 8-wide family (its LDS copy of the
    // tree), else up to QUERY_BLOCKS_PER_CU; fewer for a small batch.
    // RT_SPT_QUERY_BLOCKS=<n> caps the grid (tests: several rounds per block).
    constexpr int QUERY_BLOCKS_PER_CU = 8;
    const long long nchunks = ((long long)nrays + 63) / 64;
    long long nblocks = std::min<long long>((nchunks + wpb - 1) / wpb,
                                            (long long)sc->cus * (geo == GEO_WIDE ? 1 : QUERY_BLOCKS_PER_CU));
    if (const char *cap = getenv("RT_SPT_QUERY_BLOCKS")) nblocks = std::min<long long>(nblocks, std::max(atoi(cap), 1));
    // wide_walk: no early return (stop 0), the leaf batch threshold rendering uses
    const int opts = sptpolicy::pack_split(0, false, 0, 255, sptpolicy::SptTune().batch, 0);
    const rt::smallpt::QueryArgs a{d_rays, d_tmax, kind == SPT_QUERY_NEAREST ? d_t : nullptr, d_id, (int)nrays, sc->n,
                                   sc->d_soa, opts};
    const QueryKernel kern = geo == GEO_WIDE  ? pick_query<GEO_WIDE>(kind)
                             : geo == GEO_BVH ? pick_query<GEO_BVH>(kind)
                             : geo == GEO_LDS ? pick_query<GEO_LDS>(kind)
                                              : pick_query<GEO_GLOBAL>(kind);
    hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(64 * wpb), lds, (hipStream_t)stream, a, sc->bvh);
    return rtrt::check_launch("spt query_kernel");
}

// ---- radiance queries (spt_radiance.h)
namespace {
using RadianceKernel = decltype(&rt::smallpt::radiance_kernel<0, false>);

template <int GEO>
RadianceKernel pick_radiance(bool dl)
{
    return dl ? rt::smallpt::radiance_kernel<GEO, true> : rt::smallpt::radiance_kernel<GEO, false>;
}
}  // namespace

extern "C" int spt_scene_radiance_async(const spt_scene *sc, const float *d_rays, size_t nrays,
                                        const uint32_t *d_seeds_in, uint32_t *d_seeds_out, float *d_radiance,
                                        int first_sample, int nsamples, int mode, void *stream)
{
    if (!sc || !d_rays || !d_seeds_in || !d_seeds_out || !d_radiance)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_radiance_async: null scene, rays, seeds or radiance");
    if (nsamples < 0 || first_sample < 0)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_radiance_async: negative nsamples or first_sample");
    if (mode != SPT_PATH_TRACING && mode != SPT_DIRECT_LIGHTING)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_radiance_async: unknown mode (no flags are taken)");
    if (nrays > (size_t)INT32_MAX) return rtrt::fail(RT_ERR_INVALID, "spt_scene_radiance_async: too many rays");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_radiance_async: the scene's device is not the current one");
    if (nrays == 0) return RT_OK;
    // The family rendering picks (scene_geo); an LDS-family scene whose copy
    // would not fit a block reads the same records from global memory (with
    // MAX_LDS_BYTES below a CU's LDS every admitted copy fits today).
    const SceneSizes sizes{sc->n, sc->nlights, sc->bvh.wnodes, sc->bvh.wdepth};
    int geo = scene_geo(*sc);
    if (geo == GEO_LDS && radiance_lds_bytes(geo, sizes) > (size_t)CU_LDS_BYTES) geo = GEO_GLOBAL;
    const size_t lds = radiance_lds_bytes(geo, sizes);
    const int wpb = query_wpb(geo);
    // query_kernel's grid: persistent blocks, one per CU for the 8-wide
    // family, else up to RADIANCE_BLOCKS_PER_CU; RT_SPT_QUERY_BLOCKS caps it.
    constexpr int RADIANCE_BLOCKS_PER_CU = 8;
    const long long nchunks = ((long long)nrays + 63) / 64;
    long long nblocks = std::min<long long>((nchunks + wpb - 1) / wpb,
                                            (long long)sc->cus * (geo == GEO_WIDE ? 1 : RADIANCE_BLOCKS_PER_CU));
    if (const char *cap = getenv("RT_SPT_QUERY_BLOCKS")) nblocks = std::min<long long>(nblocks, std::max(atoi(cap), 1));
    const int opts = sptpolicy::pack_split(0, false, 0, 255, sptpolicy::SptTune().batch, 0);
    const rt::smallpt::RadianceArgs a{d_rays, d_seeds_in, d_seeds_out, d_radiance, (int)nrays, first_sample, nsamples,
                                      sc->n, sc->nlights, sc->d_soa, opts};
    const bool dl = mode == SPT_DIRECT_LIGHTING;
    const RadianceKernel kern = geo == GEO_WIDE  ? pick_radiance<GEO_WIDE>(dl)
                                : geo == GEO_BVH ? pick_radiance<GEO_BVH>(dl)
                                : geo == GEO_LDS ? pick_radiance<GEO_LDS>(dl)
                                                 : pick_radiance<GEO_GLOBAL>(dl);
    hipLaunchKernelGGL(kern, dim3((unsigned)nblocks), dim3(64 * wpb), lds, (hipStream_t)stream, a, sc->bvh);
    return rtrt::check_launch("spt radiance_kernel");
}

// ---- pixel lists (spt_pixels.h)
namespace {
template <bool STATS>
using PixelsKernel = decltype(&rt::smallpt::pixels_kernel<0, false, STATS>);

template <int GEO, bool STATS>
PixelsKernel<STATS> pick_pixels(bool dl)
{
    return dl ? rt::smallpt::pixels_kernel<GEO, true, STATS> : rt::smallpt::pixels_kernel<GEO, false, STATS>;
}

template <bool STATS>
PixelsKernel<STATS> pick_pixels(int geo, bool dl)
{
    return geo == GEO_WIDE  ? pick_pixels<GEO_WIDE, STATS>(dl)
           : geo == GEO_BVH ? pick_pixels<GEO_BVH, STATS>(dl)
           : geo == GEO_LDS ? pick_pixels<GEO_LDS, STATS>(dl)
                            : pick_pixels<GEO_GLOBAL, STATS>(dl);
}

// Both pixel-list entry points: `who` names the caller in the messages;
// stats: the second-moment plane d_m2 is kept (the STATS kernels).
int render_pixels(const char *who, const spt_scene *sc, const rt_camera *camera, float *d_colors,
                  const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels, int w, int h,
                  const int32_t *d_list, const int32_t *d_take, size_t nlist, int nsamples, int32_t *d_done,
                  int first_sample, int mode, bool stats, float *d_m2, void *stream)
{
    const auto bad = [who](const char *what) { return rtrt::fail(RT_ERR_INVALID, (std::string(who) + ": " + what).c_str()); };
    if (!sc || !camera || !d_colors || !d_seeds_in || !d_seeds_out || !d_pixels || !d_list)
        return bad("null scene, camera, colours, seeds, pixels or list");
    if (stats && !d_m2) return bad("null d_m2");
    if (w < 1 || h < 1 || (long long)w * h > (long long)INT32_MAX) return bad("bad frame size");
    if (nsamples < 0 || first_sample < 0) return bad("negative nsamples or first_sample");
    if (d_take && nsamples > 0) return bad("nsamples must be 0 beside d_take");
    if (d_done && first_sample > 0) return bad("first_sample must be 0 beside d_done");
    if (mode != SPT_PATH_TRACING && mode != SPT_DIRECT_LIGHTING) return bad("unknown mode (no flags are taken)");
    if (nlist > (size_t)INT32_MAX) return bad("list too long");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device) return bad("the scene's device is not the current one");
    if (nlist == 0) return RT_OK;
    // spt_scene_radiance_async's family, LDS bytes and grid: persistent
    // blocks over the list's chunks; RT_SPT_QUERY_BLOCKS caps the grid.
    const SceneSizes sizes{sc->n, sc->nlights, sc->bvh.wnodes, sc->bvh.wdepth};
    int geo = scene_geo(*sc);
    if (geo == GEO_LDS && radiance_lds_bytes(geo, sizes) > (size_t)CU_LDS_BYTES) geo = GEO_GLOBAL;
    const size_t lds = radiance_lds_bytes(geo, sizes);
    const int wpb = query_wpb(geo);
    constexpr int PIXELS_BLOCKS_PER_CU = 8;
    const long long nchunks = ((long long)nlist + 63) / 64;
    long long nblocks = std::min<long long>((nchunks + wpb - 1) / wpb,
                                            (long long)sc->cus * (geo == GEO_WIDE ? 1 : PIXELS_BLOCKS_PER_CU));
    if (const char *cap = getenv("RT_SPT_QUERY_BLOCKS")) nblocks = std::min<long long>(nblocks, std::max(atoi(cap), 1));
    // RT_SPT_PIXELS_REFILL=0 (read at the call; tools/pixel_list_time.py): lanes
    // claim only when their whole wave is out of samples.  Same results.
    const char *rf = getenv("RT_SPT_PIXELS_REFILL");
    const int refill = !(rf && !strcmp(rf, "0"));
    const int opts = sptpolicy::pack_split(0, false, 0, 255, sptpolicy::SptTune().batch, 0);
    const rt::smallpt::PixelsArgs a{*camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, d_list, d_take,
                                    (int)nlist, nsamples, d_done, first_sample, sc->n, sc->nlights, sc->d_soa, opts,
                                    refill};
    const bool dl = mode == SPT_DIRECT_LIGHTING;
    if (stats) {
        const rt::smallpt::PixelsStatsArgs as{a, d_m2};
        hipLaunchKernelGGL(pick_pixels<true>(geo, dl), dim3((unsigned)nblocks), dim3(64 * wpb), lds, (hipStream_t)stream,
                           as, sc->bvh);
    } else {
        hipLaunchKernelGGL(pick_pixels<false>(geo, dl), dim3((unsigned)nblocks), dim3(64 * wpb), lds, (hipStream_t)stream,
                           a, sc->bvh);
    }
    return rtrt::check_launch(stats ? "spt pixels_kernel (stats)" : "spt pixels_kernel");
}
}  // namespace

extern "C" int spt_scene_render_pixels_async(const spt_scene *sc, const rt_camera *camera, float *d_colors,
                                             const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels,
                                             int w, int h, const int32_t *d_list, const int32_t *d_take, size_t nlist,
                                             int nsamples, int32_t *d_done, int first_sample, int mode, void *stream)
{
    return render_pixels("spt_scene_render_pixels_async", sc, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h,
                         d_list, d_take, nlist, nsamples, d_done, first_sample, mode, false, nullptr, stream);
}

extern "C" int spt_scene_render_pixels_stats_async(const spt_scene *sc, const rt_camera *camera, float *d_colors,
                                                   const uint32_t *d_seeds_in, uint32_t *d_seeds_out,
                                                   uint32_t *d_pixels, float *d_m2, int w, int h,
                                                   const int32_t *d_list, const int32_t *d_take, size_t nlist,
                                                   int nsamples, int32_t *d_done, int first_sample, int mode,
                                                   void *stream)
{
    return render_pixels("spt_scene_render_pixels_stats_async", sc, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels,
                         w, h, d_list, d_take, nlist, nsamples, d_done, first_sample, mode, true, d_m2, stream);
}

// ---- the sample plan (spt_plan.h)
extern "C" size_t spt_frame_plan_scratch_bytes(int w, int h)
{
    if (w < 1 || h < 1 || (long long)w * h > (long long)INT32_MAX) return 0;
    return rt::smallpt::plan_scratch_bytes(rt::smallpt::plan_tiles(w, h));
}

extern "C" int spt_frame_plan_async(const float *d_colors, const float *d_m2, const int32_t *d_done, int w, int h,
                                    const spt_plan_params *params, int32_t *d_list, int32_t *d_take, size_t cap,
                                    float *d_error, uint64_t *d_totals, void *d_scratch, void *stream)
{
    const auto bad = [](const char *what) { return rtrt::fail(RT_ERR_INVALID, what); };
    if (!d_colors || !d_m2 || !d_done || !params || !d_scratch)
        return bad("spt_frame_plan_async: null colours, second moments, counts, params or scratch");
    if (cap > 0 && (!d_list || !d_take)) return bad("spt_frame_plan_async: null d_list or d_take");
    if (w < 1 || h < 1 || (long long)w * h > (long long)INT32_MAX) return bad("spt_frame_plan_async: bad frame size");
    if (params->min_samples < 1 || params->max_samples < params->min_samples || params->step < 1)
        return bad("spt_frame_plan_async: min_samples < 1, max_samples < min_samples or step < 1");
    if (!(params->tol >= 0.f) || !(params->floor >= 0.f))
        return bad("spt_frame_plan_async: tol or floor negative or not a number");
    if (cap > (size_t)INT32_MAX) return bad("spt_frame_plan_async: cap too large");
    namespace sp = rt::smallpt;
    const int ntiles = sp::plan_tiles(w, h);
    const sp::PlanArgs a{d_colors, d_m2, d_done, w, h, ntiles, *params, d_list, d_take, (int)cap, d_error, d_totals,
                         sp::plan_scratch_head(d_scratch), sp::plan_scratch_sums(d_scratch),
                         sp::plan_scratch_counts(d_scratch, ntiles)};
    const hipStream_t s = (hipStream_t)stream;
    const dim3 tiles((unsigned)((ntiles + sp::PLAN_WPB - 1) / sp::PLAN_WPB)), waves(64 * sp::PLAN_WPB);
    hipLaunchKernelGGL(sp::plan_count_kernel<sp::PLAN_WPB>, tiles, waves, 0, s, a);
    hipLaunchKernelGGL(sp::plan_scan_kernel<sp::PLAN_SCAN_ITEMS>, dim3(1), dim3(sp::PLAN_SCAN_THREADS), 0, s, a);
    if (cap > 0) hipLaunchKernelGGL(sp::plan_scatter_kernel<sp::PLAN_WPB>, tiles, waves, 0, s, a);
    return rtrt::check_launch("spt plan kernels");
}

namespace {
// One launch of rows [r0, r1) (every gstride-th 8-row group), or (c.list)
// of the caller's nlist tile groups over the whole frame.
int scene_render(const spt_scene *sc, const RenderCall &c)
{
    if (c.r0 >= c.r1 || (c.list && c.nlist < 1)) return RT_OK;
    Shape grid = sptpolicy::launch_shape(sc->cus, sc->bvh.wnode != nullptr, c.w, c.r0, c.r1, c.gstride,
                                         c.list ? c.nlist : 0, sptpolicy::spt_tune());
    // Full-counter launches learn and use an order of their own: their
    // shadow walks seek the highest-index occluder (twice the uncounted
    // walk's work, unevenly over the tiles), so their tile costs would order
    // the uncounted launches wrongly (configs[4]: 28.0 ms with such an order,
    // 25.4 ms with the uncounted kernel's own) -- and the uncounted order is
    // not theirs either (counted 44.7 ms with it, 52.9 ms with none).
    sptsched::SptSched &sched = counter_mode(c) == CNT_FULL ? sc->sched_cnt : sc->sched;
    bool record = false;
    if (c.list) {
        // The caller's order, heaviest first: its first groups get the
        // heavy-tile treatment (cooperative or routed tiles)
        // as with a learnt order -- unless the launch records costs
        // (c.cost): the list is then taken as unordered and every tile runs
        // a lane per pixel, so the recorded costs compare like with like.
        grid.order = c.list;
        grid.cost = sc->bvh.node ? c.cost : nullptr;
        grid.cost_max = (c.mode & SPT_COST_MAX) != 0;
        grid.tiers = c.cost == nullptr;
    } else if (sc->bvh.node) {                          // (the full-scan kernels have no order/cost code)
        record = sptsched::sched_before(sched, grid, c.stream,
                                        {c.w, c.h, c.r0, c.r1, c.gstride, c.nsamples,
                                         c.mode & ~(SPT_COUNT_RAYS | SPT_COST_MAX), grid.nslots, *c.cam});
    }
    int rc = launch(*sc, c, grid);
    if (!c.list && sc->bvh.node) sptsched::sched_used(sched, c.stream);
    if (rc == RT_OK) rc = rtrt::check_launch("spt render_kernel");
    if (rc == RT_OK && record) sptsched::sched_after(sched, c.stream);
    return rc;
}
}  // namespace

extern "C" int spt_scene_render_async(const spt_scene *sc, const rt_camera *camera, float *d_colors,
                                      const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels,
                                      int w, int h, int row_begin, int row_end, int first_sample,
                                      int nsamples, int mode, uint64_t *d_counters, void *stream)
{
    if (!sc) return rtrt::fail(RT_ERR_INVALID, "spt_scene_render_async: null scene");
    int rc = check_render_args(camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, row_begin,
                               row_end, first_sample, nsamples, mode);
    if (rc) return rc;
    return scene_render(sc, {camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, row_begin, row_end, 1,
                             first_sample, nsamples, mode, (unsigned long long *)d_counters, (hipStream_t)stream});
}

extern "C" int spt_scene_render_groups_async(const spt_scene *sc, const rt_camera *camera, float *d_colors,
                                             const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels,
                                             int w, int h, int group, int ngroups, int first_sample, int nsamples,
                                             int mode, uint64_t *d_counters, void *stream)
{
    if (!sc) return rtrt::fail(RT_ERR_INVALID, "spt_scene_render_groups_async: null scene");
    if (ngroups < 1 || group < 0 || group >= ngroups)
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_render_groups_async: need 0 <= group < ngroups");
    int rc = check_render_args(camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, 0, h, first_sample,
                               nsamples, mode);
    if (rc) return rc;
    return scene_render(sc, {camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, 8 * group, h, ngroups,
                             first_sample, nsamples, mode, (unsigned long long *)d_counters, (hipStream_t)stream});
}

extern "C" int spt_group_count(int w, int h)
{
    if (w < 1 || h < 1) return rtrt::fail(RT_ERR_INVALID, "spt_group_count: bad size");
    const long long n = ((long long)((w + 7) / 8) * ((h + 7) / 8) + 3) / 4;
    if (n > (1LL << 28)) return rtrt::fail(RT_ERR_INVALID, "spt_group_count: frame too large");
    return (int)n;
}

extern "C" int spt_scene_render_list_async(const spt_scene *sc, const rt_camera *camera, float *d_colors,
                                           const uint32_t *d_seeds_in, uint32_t *d_seeds_out, uint32_t *d_pixels,
                                           int w, int h, const int *d_groups, int ngroups, int first_sample,
                                           int nsamples, int mode, uint64_t *d_counters, unsigned *d_group_cost,
                                           void *stream)
{
    if (!sc) return rtrt::fail(RT_ERR_INVALID, "spt_scene_render_list_async: null scene");
    const int total = spt_group_count(w, h);
    if (total < 0) return total;
    if (ngroups < 0 || ngroups > total || (ngroups > 0 && !d_groups))
        return rtrt::fail(RT_ERR_INVALID, "spt_scene_render_list_async: need 0 <= ngroups <= spt_group_count(w, h)");
    const bool is_set = (mode & SPT_LIST_SET) != 0;
    mode &= ~SPT_LIST_SET;
    int rc = check_render_args(camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, 0, h, first_sample,
                               nsamples, mode);
    if (rc || ngroups == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    RenderCall call = {camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, 0, h, 1, first_sample, nsamples,
                       mode, (unsigned long long *)d_counters, s, d_groups, ngroups, d_group_cost};
    if (is_set) return scene_render(sc, call);          // (the caller's promise: no dedup pass)
    // The list as a set (list_dedup_kernel): repeated entries render once.
    // Stream-ordered scratch (graph-capturable): ngroups entries + the claim bits.
    const size_t bits = sizeof(unsigned) * (size_t)((total + 31) / 32);
    char *scratch = nullptr;
    hipError_t e = hipMallocAsync((void **)&scratch, sizeof(int) * (size_t)ngroups + bits, s);
    if (e == hipSuccess) e = hipMemsetAsync(scratch + sizeof(int) * (size_t)ngroups, 0, bits, s);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_scene_render_list_async scratch");
    int *d_set = (int *)scratch;
    const unsigned blocks = (unsigned)std::min((ngroups + 255) / 256, 1024);
    hipLaunchKernelGGL(rt::smallpt::list_dedup_kernel, dim3(blocks), dim3(256), 0, s, d_groups, ngroups, total,
                       (unsigned *)(scratch + sizeof(int) * (size_t)ngroups), d_set);
    rc = rtrt::check_launch("spt list_dedup_kernel");
    call.list = d_set;
    if (rc == RT_OK) rc = scene_render(sc, call);
    e = hipFreeAsync(scratch, s);
    if (rc == RT_OK && e != hipSuccess) rc = rtrt::fail_hip(e, "spt_scene_render_list_async scratch free");
    return rc;
}

namespace {
int groups_copy(bool pack, float *d_colors, int w, int h, const int *d_groups, int n, float *d_buf, void *stream)
{
    const int total = spt_group_count(w, h);
    if (total < 0) return total;
    if (!d_colors || !d_buf || n < 0 || n > total || (n > 0 && !d_groups))
        return rtrt::fail(RT_ERR_INVALID, "spt_groups_pack/unpack: bad arguments");
    if (n == 0) return RT_OK;
    const size_t ne = (size_t)n * rt::smallpt::GROUP_FLOATS;
    const unsigned blocks = (unsigned)std::min<size_t>((ne + 255) / 256, 8192);
    if (pack)
        hipLaunchKernelGGL(rt::smallpt::groups_copy_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                           d_colors, w, h, d_groups, n, d_buf);
    else
        hipLaunchKernelGGL(rt::smallpt::groups_copy_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                           d_colors, w, h, d_groups, n, d_buf);
    return rtrt::check_launch("spt groups_copy_kernel");
}
}  // namespace

extern "C" int spt_groups_pack_async(const float *d_colors, int w, int h, const int *d_groups, int ngroups,
                                     float *d_out, void *stream)
{
    return groups_copy(true, (float *)d_colors, w, h, d_groups, ngroups, d_out, stream);
}

extern "C" int spt_groups_unpack_async(float *d_colors, int w, int h, const int *d_groups, int ngroups,
                                       const float *d_in, void *stream)
{
    return groups_copy(false, d_colors, w, h, d_groups, ngroups, (float *)d_in, stream);
}

namespace {
// One prepared scene per device for the entry points that take a bare sphere
// array (spt_render, spt_render_async), reused while the array is unchanged
// (compared byte for byte): a progressive loop calling them once per pass no
// longer re-uploads the scene, rebuilds its hierarchy (>= 256 spheres) and
// synchronises the device to free it on every call.
struct SceneCache {
    std::vector<rt_sphere> host;
    std::string hooks;                // the preparation's test hooks (RT_SPT_NO_BVH, RT_SPT_GEO, RT_SPT_WIDE[_LEAF])
    spt_scene *sc = nullptr;
};
SceneCache g_scene_cache[64];

}  // namespace

namespace rtrt {
std::string scene_prep_hooks()
{
    std::string h;
    for (const char *k : {"RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_WIDE"}) {
        const char *v = getenv(k);
        h += v ? v : "-";
        h += "|";
    }
    return h;
}
}  // namespace rtrt

namespace {
// Caller holds the device state's lock.
int cached_scene(const rtrt::DeviceState &st, const rt_sphere *spheres, unsigned n, spt_scene **out)
{
    SceneCache &c = g_scene_cache[st.device];
    const std::string hooks = rtrt::scene_prep_hooks();
    if (c.sc && c.host.size() == n && c.hooks == hooks &&
        memcmp(c.host.data(), spheres, sizeof(rt_sphere) * n) == 0) {
        *out = c.sc;
        return RT_OK;
    }
    if (c.sc) {
        spt_scene_destroy(c.sc);          // waits for the frames that use it
        c.sc = nullptr;
        c.host.clear();
    }
    int rc = spt_scene_create(spheres, n, &c.sc);
    if (rc) {
        c.sc = nullptr;
        return rc;
    }
    c.host.assign(spheres, spheres + n);
    c.hooks = hooks;
    *out = c.sc;
    return RT_OK;
}
}  // namespace

namespace rtrt {
// Under each device state's lock, the one cached_scene's callers hold: a
// render on another thread never sees a destroyed cached scene.
void release_cached_scenes()
{
    for (int d = 0; d < 64; d++) {
        SceneCache &c = g_scene_cache[d];
        DeviceState *st = nullptr;
        if (c.sc) {
            DeviceScope scope;
            if (scope.select(d) == RT_OK && state(&st) == RT_OK) {
                std::lock_guard<std::recursive_mutex> lk(st->mu);
                if (c.sc) spt_scene_destroy(c.sc);
                c.sc = nullptr;
                c.host.clear();
                continue;
            }
        }
        if (c.sc) spt_scene_destroy(c.sc);
        c.sc = nullptr;
        c.host.clear();
    }
}
}  // namespace rtrt

// Device-pointer-only entry: reads the sphere array back (one sync of
// `stream`) to find or prepare the cached scene, then renders asynchronously.
extern "C" int spt_render_async(const rt_sphere *d_spheres, unsigned nspheres, const rt_camera *camera,
                                float *d_colors, const uint32_t *d_seeds_in, uint32_t *d_seeds_out,
                                uint32_t *d_pixels, int w, int h, int row_begin, int row_end,
                                int first_sample, int nsamples, int mode, uint64_t *d_counters,
                                void *stream)
{
    if (!d_spheres || nspheres < 1 || nspheres > (1u << 24))
        return rtrt::fail(RT_ERR_INVALID, "spt_render_async: bad scene");
    int rc = check_render_args(camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, row_begin,
                               row_end, first_sample, nsamples, mode);
    if (rc) return rc;
    rtrt::DeviceState *st;
    if ((rc = rtrt::state(&st))) return rc;
    std::lock_guard<std::recursive_mutex> lk(st->mu);
    std::vector<rt_sphere> host(nspheres);
    hipError_t e = hipMemcpyAsync(host.data(), d_spheres, sizeof(rt_sphere) * nspheres, hipMemcpyDeviceToHost,
                                  (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_render_async scene read");
    spt_scene *sc;
    if ((rc = cached_scene(*st, host.data(), nspheres, &sc))) return rc;
    return spt_scene_render_async(sc, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, row_begin,
                                  row_end, first_sample, nsamples, mode, d_counters, stream);
}

extern "C" int spt_pack_pixels_async(const float *d_colors, uint32_t *d_pixels, int w, int h, int row_begin,
                                     int row_end, void *stream)
{
    if (!d_colors || !d_pixels || w < 1 || h < 1 || row_begin < 0 || row_end > h || row_begin > row_end)
        return rtrt::fail(RT_ERR_INVALID, "spt_pack_pixels_async: bad arguments");
    const size_t n = (size_t)(row_end - row_begin) * w;
    if (n == 0) return RT_OK;
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(rt::smallpt::pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, d_colors, d_pixels,
                       w, h, row_begin, row_end);
    return rtrt::check_launch("spt pack_kernel");
}

#ifdef RT_SPT_PROF
// Tools-only: reads and clears the block profile (2 * PB_N counters).
extern "C" int spt_prof_read(unsigned long long *out)
{
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(rt::smallpt::g_spt_prof), sizeof(rt::smallpt::g_spt_prof));
    static const unsigned long long zero[2 * rt::smallpt::PB_N] = {};
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(rt::smallpt::g_spt_prof), zero, sizeof(zero));
    return e == hipSuccess ? RT_OK : rtrt::fail_hip(e, "spt_prof_read");
}
#endif

#ifdef RT_SPT_TRACE
// Tools-only: sets the wave-timeline buffer (uint4 per wave of the grid; null: off).
extern "C" int spt_trace_set(void *buf)
{
    uint4 *p = (uint4 *)buf;
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(rt::smallpt::g_spt_trace), &p, sizeof(p));
    return e == hipSuccess ? RT_OK : rtrt::fail_hip(e, "spt_trace_set");
}

// Tools-only: renders only tile group g (-1: all) in later launches.
extern "C" int spt_trace_only_group(int g)
{
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(rt::smallpt::g_spt_only_group), &g, sizeof(g));
    return e == hipSuccess ? RT_OK : rtrt::fail_hip(e, "spt_trace_only_group");
}
#endif

extern "C" int spt_render(const rt_sphere *spheres, unsigned nspheres, const rt_camera *camera,
                          float *colors, uint32_t *seeds, uint32_t *pixels, int w, int h,
                          int first_sample, int nsamples, int mode, uint64_t *counters)
{
    if (!spheres || !camera || !colors || !seeds || !pixels || w < 1 || h < 1 || nspheres < 1)
        return rtrt::fail(RT_ERR_INVALID, "spt_render: bad arguments");
    rtrt::DeviceState *st;
    int rc = rtrt::state(&st);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(st->mu);
    const size_t npx = (size_t)w * h;
    void *d_col, *d_seed, *d_px, *d_cnt;
    if ((rc = rtrt::scratch(*st, 1, 3 * sizeof(float) * npx, &d_col))) return rc;
    if ((rc = rtrt::scratch(*st, 2, 2 * sizeof(uint32_t) * npx, &d_seed))) return rc;
    if ((rc = rtrt::scratch(*st, 3, sizeof(uint32_t) * npx, &d_px))) return rc;
    if ((rc = rtrt::scratch(*st, 4, 4 * sizeof(uint64_t), &d_cnt))) return rc;
    spt_scene *sc;
    if ((rc = cached_scene(*st, spheres, nspheres, &sc))) return rc;
    hipStream_t s = st->stream;
    hipError_t e = hipMemcpyAsync(d_seed, seeds, 2 * sizeof(uint32_t) * npx, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && first_sample > 0)
        e = hipMemcpyAsync(d_col, colors, 3 * sizeof(float) * npx, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && counters) e = hipMemsetAsync(d_cnt, 0, 4 * sizeof(uint64_t), s);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_render H2D");
    rc = spt_scene_render_async(sc, camera, (float *)d_col, (uint32_t *)d_seed, (uint32_t *)d_seed,
                                (uint32_t *)d_px, w, h, 0, h, first_sample, nsamples, mode,
                                counters ? (uint64_t *)d_cnt : nullptr, s);
    if (rc) return rc;
    e = hipMemcpyAsync(seeds, d_seed, 2 * sizeof(uint32_t) * npx, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && nsamples > 0) {
        e = hipMemcpyAsync(colors, d_col, 3 * sizeof(float) * npx, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipMemcpyAsync(pixels, d_px, sizeof(uint32_t) * npx, hipMemcpyDeviceToHost, s);
    }
    if (e == hipSuccess && counters)
        e = hipMemcpyAsync(counters, d_cnt, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return rtrt::fail_hip(e, "spt_render D2H");
    return RT_OK;
}
