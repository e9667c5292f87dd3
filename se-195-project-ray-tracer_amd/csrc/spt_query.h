// spt_query.h -- caller-supplied ray queries on a prepared smallpt scene
// (spt_scene_query_async): nearest hit, occluded-or-not and the highest-index
// occluder, one ray per lane.  Not a stand-alone header: smallpt.hip includes
// it inside namespace rt::smallpt, after spt_walk.h -- the sphere loops
// (query_bf, shadow_bf) and the walks (bvh_walk, wide_walk) are render_kernel's
// own, driven here by rays that come from memory instead of from a path.
#ifndef SPT_QUERY_H
#define SPT_QUERY_H

// ---------------------------------------------------------------------------
// Mapping.  64 consecutive rays are a chunk, one per lane; wave v of block b
// takes chunks b * W + v, + G * W, ... (W waves per block, G blocks): a static
// grid-stride loop, no atomics and no work ring.  Blocks are persistent, so
// the LDS copy a family needs -- the geo records (GEO_LDS), the 8-wide nodes
// and, for the highest-occluder kind, their highest-index table (GEO_WIDE) --
// is staged once per block (spt_layout.h query_lds_bytes).
//
// Why the results are the full scan's.  The two scan families run the loops
// render_kernel runs over every sphere.  The walks test a subset with the same
// float formula and skip a sphere only when its distance provably cannot be
// taken (spt_walk.h's margin argument, which holds per ray and nowhere assumes
// where the ray came from; a direction far from unit length gets alpha = 1e30,
// no culling); nearest hit and highest occluder are order-independent choices.
// Two things the path tracer never asks are settled before a loop or walk:
//   * A ray with a non-finite component hits nothing under SphereIntersect
//     (every det is NaN, or a root is +-inf or NaN: tests/test_ray_query.py
//     checks it on the restatement), and a bound that is <= EPS or NaN accepts
//     nothing.  Such a lane is classified up front and returns the miss: no
//     NaN reaches a walk's slab tests, and a scan runs the lane on a stand-in
//     ray whose result is dropped.
//   * Nearest hit with a caller's bound B takes d < B, strictly.  The walks
//     take a distance equal to their running t when its index is higher than
//     the one they hold (the tie rule), and they start holding -1: started at
//     t = B they would take d == B.  They start at the float below B instead:
//     d < B is then "d below that float, or tied with it", ties to the highest
//     index as ever, and B = +inf (below it: FLT_MAX) needs no case of its own.
//     The scan loops compare keys strictly (spt_accept.h) and take B as it is.
// ---------------------------------------------------------------------------
constexpr int Q_NEAREST = 0, Q_ANY = 1, Q_OCCLUDER = 2;      // rt_hip.h's SPT_QUERY_*

struct QueryArgs {
    const float *rays;        // 6 floats per ray: o.xyz, d.xyz
    const float *tmax;        // one per ray (nearest hit: nullable, 1e20f)
    float *t;                 // nearest hit only, nullable
    int *id;                  // nullable for the nearest hit
    int nrays;
    int n;                    // spheres
    const float4 *geo;        // the scene's SoA geo records (scan families)
    int opts;                 // wide_walk's options (spt_policy.h's split word)
};

template <int GEO, int KIND>
__global__ void __launch_bounds__(64 * query_wpb(GEO)) query_kernel(QueryArgs a, BvhView bvh)
{
    constexpr bool SHADOW = KIND != Q_NEAREST, COUNT = KIND == Q_OCCLUDER;
    extern __shared__ __attribute__((aligned(16))) char qmem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    DynGeo geo{a.geo, a.n};
    const uint4 *wL = (const uint4 *)qmem;
    unsigned *wstk = nullptr;
    if constexpr (GEO == GEO_LDS) {
        float4 *s = (float4 *)qmem;
        for (int i = threadIdx.x; i < a.n; i += blockDim.x) s[i] = a.geo[i];
        __syncthreads();
        geo.g = s;
    }
    if constexpr (GEO == GEO_WIDE) {
        uint4 *d = (uint4 *)qmem;
        for (int i = threadIdx.x; i < 7 * bvh.wnodes; i += blockDim.x) d[i] = bvh.wnode[i];
        if (COUNT)
            for (int i = threadIdx.x; i < 2 * bvh.wnodes; i += blockDim.x) d[7 * bvh.wnodes + i] = bvh.wmax[i];
        wstk = (unsigned *)(qmem + wide_stack_offset(bvh.wnodes, COUNT)) +
               (size_t)wave * WIDE_LEVEL_DW * (bvh.wdepth > 1 ? bvh.wdepth - 1 : 1);
        __syncthreads();
    }
    const int nchunks = (int)(((unsigned)a.nrays + 63u) >> 6);
    for (int c = (int)blockIdx.x * wpb + wave; c < nchunks; c += (int)gridDim.x * wpb) {
        const size_t r = (size_t)c * 64 + lane;
        const bool valid = r < (size_t)a.nrays;
        ray3 ray;
        ray.o = mk(0.f, 0.f, 0.f);
        ray.d = mk(0.f, 0.f, 1.f);
        float bound = 1e20f;
        if (valid) {
            const float *p = a.rays + 6 * r;
            ray.o = mk(p[0], p[1], p[2]);
            ray.d = mk(p[3], p[4], p[5]);
            if (SHADOW || a.tmax) bound = a.tmax[r];
        }
        const bool finite = fabsf(ray.o.x) < MISS && fabsf(ray.o.y) < MISS && fabsf(ray.o.z) < MISS &&
                            fabsf(ray.d.x) < MISS && fabsf(ray.d.y) < MISS && fabsf(ray.d.z) < MISS;
        const bool live = valid && finite && bound > EPS;
        float t = bound;
        int id = -1;               // nearest hit: its index; highest occluder: that
        bool occ = false;          // occluded or not
        if constexpr (GEO == GEO_LDS || GEO == GEO_GLOBAL) {
            // every lane runs the wave-uniform loop; a lane without a query
            // runs it on a stand-in whose result is dropped
            ray3 q = ray;
            if (!live) {
                q.o = mk(0.f, 0.f, 0.f);
                q.d = mk(0.f, 0.f, 1.f);
                t = 1e20f;
            }
            int first = -1;
            if constexpr (KIND == Q_ANY) {
                occ = shadow_bf(geo, q, t, live);
            } else {
                id = query_bf<COUNT, true>(geo, q, t, first);
                if (COUNT) id = first;
            }
        } else if constexpr (GEO == GEO_BVH) {
            BvhWalk W = {};
            bool walking = live;
            if (live) bvh_begin<COUNT>(bvh, ray, SHADOW, SHADOW ? bound : __uint_as_float(__float_as_uint(bound) - 1u), W);
            while (wave_any(walking)) {
                if (walking) walking = !bvh_walk<COUNT>(bvh, ray, SHADOW, W);
            }
            if (live) {
                t = W.t;
                id = W.id;
                occ = W.id >= 0;
            }
        } else {
            BvhWalk W = {};
            bool walking = live;
            if (live) wide_begin<COUNT>(bvh, ray, SHADOW, SHADOW ? bound : __uint_as_float(__float_as_uint(bound) - 1u), W);
            while (wave_any(walking)) {
                if (walking) walking = !wide_walk<COUNT>(bvh, wL, wstk, ray, SHADOW, W, a.opts);
            }
            if (live) {
                t = W.t;
                id = W.id;
                occ = W.id >= 0;
            }
        }
        if (valid) {
            if constexpr (KIND == Q_NEAREST) {
                const bool hit = live && id >= 0;
                if (a.id) a.id[r] = hit ? id : -1;
                // (a miss: the bound's own bits, whatever they are)
                if (a.t) ((unsigned *)a.t)[r] = hit ? __float_as_uint(t) : __float_as_uint(bound);
            } else if constexpr (KIND == Q_ANY) {
                a.id[r] = (live && occ) ? 1 : 0;
            } else {
                a.id[r] = (live && id >= 0) ? id : -1;
            }
        }
    }
}

#endif  // SPT_QUERY_H
