// prims_query.hip -- caller-supplied ray queries on the level-pass tracers'
// scenes (rt_hip.h "level-pass tracers, ray queries": rtw_prims_create,
// rtq_prims_create, rtw_prims_set_async, rtq_prims_set_async, rtp_query_async):
// what does this ray hit, is this point shadowed, and by which primitive --
// with the loops the Whitted tracer (whitted.hip) and the queue tracer
// (queue.hip) render with: rt_prims.h's nearest_n and first_occluder over the
// lists fill_lists builds.  Nothing here is on the tracers' frame path.
//
// Mapping.  A prepared scene is one device image (Image: the PrimLists, a
// table from occluder position to primitive index, the tracer's tag), built by
// one wave, a lane per primitive, from the reference's 96-byte primitive array
// -- at create from a staged copy of the host array, at set_async straight
// from the caller's device array on the caller's stream, so queries enqueued
// after it on that stream see the new primitives.  Query blocks are
// persistent: each stages the ~5.4 KB image into LDS once (load_scene) and its
// waves then walk chunks of 64 x R consecutive rays in a static grid-stride
// loop -- wave v of block b takes chunks b * W + v, + G * W, ... -- with no
// atomics, as spt_query.h does.  A lane past nrays runs an all-NaN ray (every
// sphere's det is NaN, so it neither asks for the wave's exact-sqrt redo nor
// takes anything; every plane candidate is +inf) and stores nothing; in the
// occluded-or-not kind it starts as "occluded" so that it never holds back
// the wave-level exit.
//
// Why a bound is a filter (NEAREST with d_tmax).  A primitive's candidate
// distance does not depend on the distance to beat (scene.cpp:125-190,
// raytracer_non_OpenCL.c:95-160 compare it with *a_Dist only after computing
// it), so the reference's loop started at B <= far returns the unbounded
// nearest hit when that is < B and nothing otherwise: nearest_n keeps its
// compile-time far, and the bound is one comparison on its answer
// (tests/test_prims_query_ref.py checks the claim on the oracle's own loop).
//
// Each tracer's classification of a primitive (sphere / plane / light /
// occluder and the two geometry float4s) is restated here from its
// build_scene (whitted.hip, queue.hip) instead of shared with it: the tracers'
// code -- and with it every row of their resource usage -- stays what it was.
// The frame tests pin the tracers' statement to the oracle, and
// tests/test_gpu_prims_query.py pins this one to the same oracle.
#include <algorithm>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "rt_common.h"
#include "rt_prims.h"
#include "rt_runtime.h"

namespace rt {
namespace pquery {

using prims::MAXP;
using prims::PrimLists;

constexpr int NONE = 0x7fffffff;           // first_occluder's "nothing occludes"

struct Image : PrimLists {
    int occ_id[MAXP];   // occluder position (first_occluder's result) -> primitive index
    int tracer;         // Whitted::tag or Queue::tag
    int pad2_[3];       // sizeof % 16 == 0 (load_scene)
};

// raytracer3.0.06: Engine_Raytrace's nearest hit (raytracer.cpp:39-49) and
// shadow loop (:76-110); whitted.hip's NearestTraits and build_scene.
struct Whitted {
    using prim_t = rt_primitive;
    static constexpr int tag = 0;
    static constexpr float far = 1000000.0f;
    static constexpr int result0 = 0, miss = 0x7fffffff;
    static __device__ bool sphere(const prim_t &q) { return q.type == 1; }
    static __device__ bool plane(const prim_t &q) { return q.type == 2; }
    static __device__ bool light(const prim_t &q) { return q.m_Light > 0; }
    static __device__ bool occluder(const prim_t &q) { return q.m_Light == 0; }     // raytracer.cpp:100
    static __device__ float4 sphere_geo(const prim_t &q)
    {
        return make_float4(q.m_Centre.x, q.m_Centre.y, q.m_Centre.z, q.m_SqRadius);
    }
    static __device__ float4 plane_geo(const prim_t &q)
    {
        return make_float4(q.plane_N.x, q.plane_N.y, q.plane_N.z, q.plane_D);
    }
};

// Raytracer3.2.03: raytrace's nearest hit (raytracer_non_OpenCL.c:181-193) and
// shadow loop (:224-241); queue.hip's NearestTraits and build_scene.
struct Queue {
    using prim_t = rtq_primitive;
    static constexpr int tag = 1;
    static constexpr float far = 10000000.0f;
    static constexpr int result0 = 1, miss = -1;
    static __device__ bool sphere(const prim_t &q) { return q.type == 1; }
    static __device__ bool plane(const prim_t &q) { return q.type == 0; }
    static __device__ bool light(const prim_t &q) { return q.is_light != 0; }
    static __device__ bool occluder(const prim_t &q) { return q.is_light == 0; }    // :232
    static __device__ float4 sphere_geo(const prim_t &q)
    {
        return make_float4(q.center.x, q.center.y, q.center.z, q.sq_radius);
    }
    static __device__ float4 plane_geo(const prim_t &q)
    {
        return make_float4(q.normal.x, q.normal.y, q.normal.z, q.depth);
    }
};

// The image from the primitive array: one wave, a lane per primitive.  Every
// count is rewritten, so a set may change nprims; list entries past the new
// counts are stale and never read.
template <class T>
__global__ void __launch_bounds__(64) build_kernel(Image *__restrict__ S, const typename T::prim_t *__restrict__ src,
                                                   int nprims)
{
    const int p = threadIdx.x;
    const bool v = p < nprims;
    typename T::prim_t q{};
    if (v) q = src[p];
    const bool occ = v && T::occluder(q);
    prims::fill_lists(*S, v, T::sphere(q), T::plane(q), T::light(q), T::occluder(q), T::sphere_geo(q),
                      T::plane_geo(q));
    // fill_lists' osph_pos / opln_pos are ranks among the occluders: the same rank, per primitive
    const int pos = __popcll(__builtin_amdgcn_ballot_w64(occ) & ((1ull << p) - 1ull));
    if (occ) S->occ_id[pos] = p;
    if (p == 0) S->tracer = T::tag;
}

struct Args {
    const float *rays;      // 6 floats per ray: o.xyz, d.xyz
    const float *tmax;      // one per ray (NEAREST: nullable)
    float *t;               // NEAREST only, nullable
    int *id;                // nullable for NEAREST
    int *result;            // NEAREST only, nullable
    int nrays;
};

constexpr int WPB = 4;      // waves per block

// Ray i as given, or the all-NaN stand-in of a lane without one.
__device__ __forceinline__ ray3 ray_or_nan(const float *__restrict__ rays, size_t i, bool valid)
{
    const float nan = __builtin_nanf("");
    ray3 r;
    r.o = mk(nan, nan, nan);
    r.d = mk(nan, nan, nan);
    if (valid) {
        const float *p = rays + 6 * i;
        r.o = mk(p[0], p[1], p[2]);
        r.d = mk(p[3], p[4], p[5]);
    }
    return r;
}

// NEAREST, R rays per lane per iteration: chunk c is rays [c * 64 R, (c + 1) * 64 R),
// slot s of a lane the ray c * 64 R + 64 s + lane (coalesced per slot).
template <class T, int R>
__global__ void __launch_bounds__(64 * WPB) nearest_kernel(const Image *__restrict__ g, Args a)
{
    __shared__ Image S;
    prims::load_scene(S, g);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr unsigned PER = 64u * R;
    const int nchunks = (int)(((unsigned)a.nrays + PER - 1u) / PER);
    for (int c = (int)blockIdx.x * WPB + wave; c < nchunks; c += (int)gridDim.x * WPB) {
        ray3 ray[R];
        size_t idx[R];
        bool valid[R];
        float bound[R];
#pragma unroll
        for (int s = 0; s < R; s++) {
            idx[s] = (size_t)c * PER + 64u * s + lane;
            valid[s] = idx[s] < (size_t)a.nrays;
            ray[s] = ray_or_nan(a.rays, idx[s], valid[s]);
            bound[s] = (valid[s] && a.tmax) ? a.tmax[idx[s]] : __builtin_inff();
        }
        float dist[R];
        int prim[R], result[R];
        prims::nearest_n<R, T>(S, ray, dist, prim, result);
#pragma unroll
        for (int s = 0; s < R; s++) {
            if (!valid[s]) continue;
            // (a miss is T::miss: 0x7fffffff or -1; a NaN bound accepts nothing)
            const bool hit = (unsigned)prim[s] < (unsigned)MAXP && dist[s] < bound[s];
            if (a.t) a.t[idx[s]] = hit ? dist[s] : T::far;
            if (a.id) a.id[idx[s]] = hit ? prim[s] : -1;
            if (a.result) a.result[idx[s]] = hit ? result[s] : 0;
        }
    }
}

// SHADOW (COUNT = false: occluded or not, with first_occluder's wave-level
// exit) and OCCLUDER (COUNT = true: the primitive the reference's loop breaks
// at).  Which primitives occlude is in the image, so the tracers share these.
template <bool COUNT>
__global__ void __launch_bounds__(64 * WPB) shadow_kernel(const Image *__restrict__ g, Args a)
{
    __shared__ Image S;
    prims::load_scene(S, g);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nchunks = (int)(((unsigned)a.nrays + 63u) >> 6);
    for (int c = (int)blockIdx.x * WPB + wave; c < nchunks; c += (int)gridDim.x * WPB) {
        const size_t i = (size_t)c * 64 + lane;
        const bool valid = i < (size_t)a.nrays;
        const ray3 ray = ray_or_nan(a.rays, i, valid);
        const float len = valid ? a.tmax[i] : 0.f;
        int first = (COUNT || valid) ? NONE : 0;
        prims::first_occluder<COUNT>(S, ray, len, first);
        if (valid) {
            if (COUNT) a.id[i] = first == NONE ? -1 : S.occ_id[first == NONE ? 0 : first];
            else a.id[i] = first != NONE ? 1 : 0;
        }
    }
}

}  // namespace pquery
}  // namespace rt

namespace pq = rt::pquery;

struct rtp_scene {
    int device = -1;
    int cus = 256;
    int tracer = -1;
    int nprims = 0;                 // of the last create / set (host bookkeeping)
    pq::Image *d_image = nullptr;
    void *d_stage = nullptr;        // create's device copy of the host array
};

namespace {

template <class T>
int prims_create(const char *who, const typename T::prim_t *prims, int nprims, rtp_scene **out)
{
    static_assert(sizeof(typename T::prim_t) == 96, "the references' 96-byte primitives");
    static_assert(sizeof(pq::Image) % 16 == 0, "load_scene copies 16-B words");
    char msg[128];
    if (!prims || !out || nprims < 1 || nprims > pq::MAXP) {
        snprintf(msg, sizeof(msg), "%s: null pointer, or nprims outside 1..%d", who, pq::MAXP);
        return rtrt::fail(RT_ERR_INVALID, msg);
    }
    *out = nullptr;
    rtrt::DeviceState *st;
    int rc = rtrt::state(&st);
    if (rc) return rc;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    hipError_t e = hipStreamIsCapturing(st->stream, &cap);
    if (e != hipSuccess) return rtrt::fail_hip(e, who);
    if (cap != hipStreamCaptureStatusNone) {
        snprintf(msg, sizeof(msg), "%s: the stream is capturing", who);
        return rtrt::fail(RT_ERR_INVALID, msg);
    }
    rtp_scene *sc = new rtp_scene();
    sc->device = st->device;
    if (st->cus > 0) sc->cus = st->cus;
    sc->tracer = T::tag;
    sc->nprims = nprims;
    const size_t bytes = sizeof(typename T::prim_t) * (size_t)nprims;
    e = hipMalloc((void **)&sc->d_image, sizeof(pq::Image));
    if (e == hipSuccess) e = hipMalloc(&sc->d_stage, sizeof(typename T::prim_t) * pq::MAXP);
    if (e == hipSuccess) e = hipMemsetAsync(sc->d_image, 0, sizeof(pq::Image), st->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sc->d_stage, prims, bytes, hipMemcpyHostToDevice, st->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(pq::build_kernel<T>, dim3(1), dim3(64), 0, st->stream, sc->d_image,
                           (const typename T::prim_t *)sc->d_stage, nprims);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st->stream);     // (the host array is free again; any stream may query)
    if (e != hipSuccess) {
        if (sc->d_image) (void)hipFree(sc->d_image);
        if (sc->d_stage) (void)hipFree(sc->d_stage);
        delete sc;
        return rtrt::fail_hip(e, who);
    }
    *out = sc;
    return RT_OK;
}

template <class T>
int prims_set(const char *who, rtp_scene *sc, const typename T::prim_t *d_prims, int nprims, void *stream)
{
    char msg[128];
    if (!sc || !d_prims || nprims < 1 || nprims > pq::MAXP) {
        snprintf(msg, sizeof(msg), "%s: null pointer, or nprims outside 1..%d", who, pq::MAXP);
        return rtrt::fail(RT_ERR_INVALID, msg);
    }
    if (sc->tracer != T::tag) {
        snprintf(msg, sizeof(msg), "%s: the scene was created for the other tracer", who);
        return rtrt::fail(RT_ERR_INVALID, msg);
    }
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device) {
        snprintf(msg, sizeof(msg), "%s: the scene's device is not the current one", who);
        return rtrt::fail(RT_ERR_INVALID, msg);
    }
    hipLaunchKernelGGL(pq::build_kernel<T>, dim3(1), dim3(64), 0, (hipStream_t)stream, sc->d_image, d_prims, nprims);
    const int rc = rtrt::check_launch(who);
    if (rc == RT_OK) sc->nprims = nprims;
    return rc;
}

// NEAREST's rays per lane: 1, or 2 as the tracers' latency-bound root kernels
// run nearest_n.  RT_PRIMS_QUERY_RAYS=1|2 (read at the call) overrides the
// default, for tests and tools/prims_query_time.py.
constexpr int NEAREST_RAYS = 1;

using QueryKernel = void (*)(const pq::Image *, pq::Args);

QueryKernel pick_kernel(int tracer, int kind, int rays)
{
    if (kind == RTP_QUERY_SHADOW) return pq::shadow_kernel<false>;
    if (kind == RTP_QUERY_OCCLUDER) return pq::shadow_kernel<true>;
    if (tracer == pq::Whitted::tag)
        return rays == 2 ? pq::nearest_kernel<pq::Whitted, 2> : pq::nearest_kernel<pq::Whitted, 1>;
    return rays == 2 ? pq::nearest_kernel<pq::Queue, 2> : pq::nearest_kernel<pq::Queue, 1>;
}

}  // namespace

extern "C" int rtw_prims_create(const rt_primitive *prims, int nprims, rtp_scene **out)
{
    return prims_create<pq::Whitted>("rtw_prims_create", prims, nprims, out);
}

extern "C" int rtq_prims_create(const rtq_primitive *prims, int nprims, rtp_scene **out)
{
    return prims_create<pq::Queue>("rtq_prims_create", prims, nprims, out);
}

extern "C" int rtp_scene_destroy(rtp_scene *sc)
{
    if (!sc) return RT_OK;
    hipError_t e = hipFree(sc->d_image);        // (waits for the device's work, queries included)
    const hipError_t e2 = hipFree(sc->d_stage);
    if (e == hipSuccess) e = e2;
    delete sc;
    return e == hipSuccess ? RT_OK : rtrt::fail_hip(e, "rtp_scene_destroy");
}

extern "C" int rtw_prims_set_async(rtp_scene *sc, const rt_primitive *d_prims, int nprims, void *stream)
{
    return prims_set<pq::Whitted>("rtw_prims_set_async", sc, d_prims, nprims, stream);
}

extern "C" int rtq_prims_set_async(rtp_scene *sc, const rtq_primitive *d_prims, int nprims, void *stream)
{
    return prims_set<pq::Queue>("rtq_prims_set_async", sc, d_prims, nprims, stream);
}

extern "C" int rtp_query_async(const rtp_scene *sc, const float *d_rays, const float *d_tmax, size_t nrays, int kind,
                               float *d_t, int *d_id, int *d_result, void *stream)
{
    // Everything that needs no device first, the scene last among it.
    if (kind != RTP_QUERY_NEAREST && kind != RTP_QUERY_SHADOW && kind != RTP_QUERY_OCCLUDER)
        return rtrt::fail(RT_ERR_INVALID, "rtp_query_async: unknown kind");
    if (kind == RTP_QUERY_NEAREST && !d_t && !d_id && !d_result)
        return rtrt::fail(RT_ERR_INVALID, "rtp_query_async: no output");
    if (kind != RTP_QUERY_NEAREST && (!d_tmax || !d_id))
        return rtrt::fail(RT_ERR_INVALID, "rtp_query_async: a shadow query needs d_tmax and d_id");
    if (nrays > (size_t)INT32_MAX) return rtrt::fail(RT_ERR_INVALID, "rtp_query_async: too many rays");
    if (!sc || !d_rays) return rtrt::fail(RT_ERR_INVALID, "rtp_query_async: null scene or rays");
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != sc->device)
        return rtrt::fail(RT_ERR_INVALID, "rtp_query_async: the scene's device is not the current one");
    if (nrays == 0) return RT_OK;
    int rays = NEAREST_RAYS;
    if (const char *r = getenv("RT_PRIMS_QUERY_RAYS")) rays = atoi(r) == 2 ? 2 : atoi(r) == 1 ? 1 : rays;
    if (kind != RTP_QUERY_NEAREST) rays = 1;
    // Persistent blocks: up to QUERY_BLOCKS_PER_CU per compute unit, fewer
    // for a small batch.  RT_PRIMS_QUERY_BLOCKS=<n> caps the grid (tests:
    // several chunks per wave).
    constexpr int QUERY_BLOCKS_PER_CU = 8;
    const long long per = 64LL * rays * pq::WPB;
    long long nblocks = std::min<long long>(((long long)nrays + per - 1) / per, (long long)sc->cus * QUERY_BLOCKS_PER_CU);
    if (const char *cap = getenv("RT_PRIMS_QUERY_BLOCKS")) nblocks = std::min<long long>(nblocks, std::max(atoi(cap), 1));
    const bool nearest = kind == RTP_QUERY_NEAREST;
    const pq::Args a{d_rays, d_tmax, nearest ? d_t : nullptr, d_id, nearest ? d_result : nullptr, (int)nrays};
    hipLaunchKernelGGL(pick_kernel(sc->tracer, kind, rays), dim3((unsigned)nblocks), dim3(64 * pq::WPB), 0,
                       (hipStream_t)stream, (const pq::Image *)sc->d_image, a);
    return rtrt::check_launch("rtp query kernel");
}
