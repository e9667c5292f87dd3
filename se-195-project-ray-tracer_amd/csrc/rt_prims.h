// rt_prims.h -- the primitive code the two level-pass tracers share
// (whitted.hip: raytracer3.0.06's Engine_Raytrace; queue.hip: Raytracer3.2.03's
// raytrace): the dense per-type primitive lists of a <= 64-primitive scene,
// the nearest-hit and first-occluder loops over them, the ballot-rank fill
// that builds them, and the scene image's copy into LDS.  Both references
// intersect spheres and planes with the same float operations; what differs
// per tracer (the far distance, the initial result, the no-hit primitive) is
// a traits struct, and everything about materials stays in the tracers.
// Besides the tracers' frame tests, nearest_n, first_occluder, light_len_inv
// and fill_lists are run on their own (tests/native/gpu_prims_check.hip) and
// compared bit for bit with the references' loops at the edges where they
// branch: tests/test_gpu_prims.py.
#ifndef RT_PRIMS_H
#define RT_PRIMS_H

#include "rt_common.h"

namespace rt {
namespace prims {

constexpr int MAXP = 64;        // the references allocate 50 (scene.cpp:225, raytracer.c:720)

// Geometry in dense per-type arrays (no index indirection in the hot loops):
// the nearest-hit and occlusion results are independent of the visiting order
// once distance ties go to the lowest primitive index (the references' strict
// '<' over ascending s), and the scene's counts.  Each tracer's Scene starts
// with it.  The counts sit together, in this order, on purpose: the kernels
// read them with wide LDS loads, and with n and nlights apart from the rest
// (in the tracer's Scene) queue.hip's counted root kernel spills 8 B/lane more.
struct PrimLists {
    float4 sph[MAXP];   // sphere centre.xyz, squared radius
    float4 pln[MAXP];   // plane normal.xyz, D
    int sph_id[MAXP], pln_id[MAXP];        // original primitive index
    float4 osph[MAXP];  // non-light spheres (the shadow loop's occluders)
    float4 opln[MAXP];  // non-light planes
    int osph_pos[MAXP], opln_pos[MAXP];    // position in the non-light order (test counts)
    int n, ns, np, nos, nop, nlights, nnonlight;   // primitives, per list, lights, non-lights
    int pad_;                                      // sizeof % 16 == 0
};

// Sphere half of the references' intersect (scene.cpp:130-169,
// raytracer_non_OpenCL.c:111-148): the candidate distance (INPRIM: i2, HIT:
// i1) or +inf with res = 0.
__device__ __forceinline__ float sphere_cand(float4 g, const ray3 &r, int &res)
{
    const float vx = r.o.x - g.x, vy = r.o.y - g.y, vz = r.o.z - g.z;
    float b = vx * r.d.x + vy * r.d.y + vz * r.d.z;
    b = -b;
    float det = (b * b) - (vx * vx + vy * vy + vz * vz) + g.w;
    res = 0;
    float cand = __builtin_inff();
    if (det > 0) {
        det = sqrt_exact(det);
        const float i1 = b - det, i2 = b + det;
        if (i2 > 0) {
            cand = i1 < 0 ? i2 : i1;
            res = i1 < 0 ? -1 : 1;
        }
    }
    return cand;
}

// Plane half (scene.cpp:171-185, raytracer_non_OpenCL.c:95-109), without
// branches: the division for every lane, its result kept only where the
// reference divides (d != 0) and t > 0.  (The per-lane-branch forms of this
// and of the sphere loops cost more exec-mask instructions than VALU, and an
// all-occluded exit per occluder sphere or per plane did not pay:
// profiles/r04.)
__device__ __forceinline__ float plane_cand_lean(float4 g, const ray3 &r)
{
    const float d = g.x * r.d.x + g.y * r.d.y + g.z * r.d.z;
    const float t = -((g.x * r.o.x + g.y * r.o.y + g.z * r.o.z) + g.w) / d;
    return (d != 0 && t > 0) ? t : __builtin_inff();
}

// The nearest hit (raytracer.cpp:39-49, raytracer_non_OpenCL.c:181-193: min
// distance below T::far, lowest index on ties) for R rays per lane in
// lock-step: each sphere and plane record is read once for all of them and
// their dependency chains interleave (R = 2 in the latency-bound root
// kernels).  Branch-lean: a sphere is one wave-uniform branch (skipped when
// no lane's det is positive) around a straight-line body -- sqrt_nr for every
// lane, its range checked once per loop, a lane outside it redoing its ray
// with the exact per-sphere test -- and a plane test is straight-line (the
// division for every lane, kept where the reference divides).  det <= 0 or
// NaN needs no test of its own: sqrt_nr returns NaN there (v_rsq of a
// negative, 0 x inf at zero), so i2 > 0 fails.  (The per-lane-branch forms
// cost more exec-mask instructions than VALU:
// profiles/r04/whitted_lean_loops_ab.log.)
// T: static constexpr float far (the distance a hit must beat), int result0
// (result without a hit), int miss (prim without a hit: 0x7fffffff or a
// negative value).  Inside, "no hit yet" is always a negative prim (`none`),
// which `id < prim[r]` never replaces on a tie: a first candidate exactly at
// T::far is refused, as by the references' strict '<' (with prim at
// 0x7fffffff it was taken); a non-negative T::miss is put in at the end.
// (For a negative T::miss the prim[r] >= 0 test says nothing more than
// id < prim[r] does; it stays because queue.hip's kernels compile to other
// code without it.)  Checked alone, at these edges, against the references'
// loops by tests/test_gpu_prims.py.
template <int R, class T>
__device__ __forceinline__ void nearest_n(const PrimLists &S, const ray3 (&ray)[R], float (&dist)[R], int (&prim)[R],
                                          int (&result)[R])
{
    constexpr int none = T::miss < 0 ? T::miss : -1;
    bool bad[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        dist[r] = T::far;
        prim[r] = none;
        result[r] = T::result0;
        bad[r] = false;
    }
    for (int k = 0; k < S.ns; k++) {
        const float4 g = S.sph[k];
        float b[R], det[R];
        bool anyp = false;
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float vx = ray[r].o.x - g.x, vy = ray[r].o.y - g.y, vz = ray[r].o.z - g.z;
            b[r] = vx * ray[r].d.x + vy * ray[r].d.y + vz * ray[r].d.z;
            b[r] = -b[r];
            det[r] = (b[r] * b[r]) - (vx * vx + vy * vy + vz * vz) + g.w;
            anyp = anyp || det[r] > 0;
        }
        if (wave_any(anyp)) {
            const int id = S.sph_id[k];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float sd = sqrt_nr(det[r]);
                bad[r] = bad[r] || (det[r] > 0 && !sqrt_nr_ok(det[r]));
                const float i1 = b[r] - sd, i2 = b[r] + sd;
                const float c = i1 < 0 ? i2 : i1;
                const bool take = i2 > 0 && (c < dist[r] || (c == dist[r] && (T::miss >= 0 || prim[r] >= 0) && id < prim[r]));
                dist[r] = take ? c : dist[r];
                prim[r] = take ? id : prim[r];
                result[r] = take ? (i1 < 0 ? -1 : 1) : result[r];
            }
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++) {
        if (wave_any(bad[r])) {                         // (rare: det outside sqrt_nr's range)
            dist[r] = T::far;
            prim[r] = none;
            result[r] = T::result0;
            for (int k = 0; k < S.ns; k++) {
                int res;
                const float c = sphere_cand(S.sph[k], ray[r], res);
                const int id = S.sph_id[k];
                if (res && (c < dist[r] || (c == dist[r] && (T::miss >= 0 || prim[r] >= 0) && id < prim[r]))) {
                    dist[r] = c; prim[r] = id; result[r] = res;
                }
            }
        }
    }
#pragma unroll 4
    for (int k = 0; k < S.np; k++) {
        const float4 g = S.pln[k];
        const int id = S.pln_id[k];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const float c = plane_cand_lean(g, ray[r]);
            const bool take = c < dist[r] || (c == dist[r] && (T::miss >= 0 || prim[r] >= 0) && id < prim[r]);
            dist[r] = take ? c : dist[r];
            prim[r] = take ? id : prim[r];
            result[r] = take ? 1 : result[r];
        }
    }
    if (T::miss >= 0) {
#pragma unroll
        for (int r = 0; r < R; r++) prim[r] = prim[r] < 0 ? T::miss : prim[r];
    }
}

// The shadow test of a sphere light `len` away along r (raytracer.cpp:76-110,
// raytracer_non_OpenCL.c:224-241): any non-light primitive nearer than the
// light centre shades the point.  The reference breaks at the first one;
// which one does not matter, only the count of tests, recovered from its
// position in the non-light order: `first` (0x7fffffff on entry) becomes that
// position and stays 0x7fffffff when nothing occludes.  (The caller's
// variable, not a return value: returned, whitted.hip's uncounted kernels
// spill 8 B/lane more.)  The loops are nearest_n's lean forms.  (An
// all-occluded exit after each sphere measured slower; the planes take one
// all-occluded check before their loop.)  COUNT = false: only "occluded or
// not" is used, so the test stops as soon as every lane of the wave has
// found an occluder (the reference's own early exit, at wave granularity).
template <bool COUNT>
__device__ __forceinline__ void first_occluder(const PrimLists &S, const ray3 &r, float len, int &first)
{
    bool sbad = false;
    for (int k = 0; k < S.nos; k++) {
        const float4 g = S.osph[k];
        const float vx = r.o.x - g.x, vy = r.o.y - g.y, vz = r.o.z - g.z;
        float b = vx * r.d.x + vy * r.d.y + vz * r.d.z;
        b = -b;
        const float det = (b * b) - (vx * vx + vy * vy + vz * vz) + g.w;
        if (wave_any(det > 0)) {
            const float sd = sqrt_nr(det);
            sbad = sbad || (det > 0 && !sqrt_nr_ok(det));
            const float i1 = b - sd, i2 = b + sd;
            const float c = i1 < 0 ? i2 : i1;
            const bool occ = i2 > 0 && c < len;
            first = occ ? min(first, S.osph_pos[k]) : first;
        }
    }
    if (wave_any(sbad)) {
        first = 0x7fffffff;
        for (int k = 0; k < S.nos; k++) {
            int res;
            const float c = sphere_cand(S.osph[k], r, res);
            if (res && c < len) first = min(first, S.osph_pos[k]);
            if (!COUNT && !wave_any(first == 0x7fffffff)) break;
        }
    }
    const bool pl_any = COUNT || wave_any(first == 0x7fffffff);   // (all occluded by a sphere: no plane test)
#pragma unroll 4
    for (int k = 0; pl_any && k < S.nop; k++) {
        const float c = plane_cand_lean(S.opln[k], r);
        first = c < len ? min(first, S.opln_pos[k]) : first;
    }
}

// len = sqrtf(d2) and inv = 1.0f / len (the shaded point to a light centre),
// bit-exact: the short forms unless a lane of the wave is outside their range.
__device__ __forceinline__ void light_len_inv(float d2, float &len, float &inv)
{
    if (!wave_any(!sqrt_nr_ok(d2))) {
        len = sqrt_nr(d2);
        inv = rcp_nr(len);
    } else {
        len = sqrt_rn(d2);
        inv = 1.0f / len;
    }
}

// The lists and counts from one wave, a lane per primitive (MAXP = 64): each
// list position is the count of the earlier primitives of its kind (ballot
// prefix), so the lists keep the reference's order.  The lane's primitive
// (if `valid`) is a sphere, a plane or neither, and a light, an occluder or
// neither.  Returns the lane's rank among the lights, for the tracer's own
// lights[].
__device__ __forceinline__ int fill_lists(PrimLists &S, bool valid, bool is_sphere, bool is_plane, bool is_light,
                                          bool is_occluder, float4 sphere_geo, float4 plane_geo)
{
    static_assert(MAXP <= 64, "one lane per primitive");
    const int p = __lane_id();
    const bool light = valid && is_light, occluder = valid && is_occluder;
    const bool sph = valid && is_sphere, pln = valid && is_plane;
    const unsigned long long below = (1ull << p) - 1ull;       // lanes before this one
    const auto rank = [&](bool b) { return __popcll(__builtin_amdgcn_ballot_w64(b) & below); };
    const auto total = [](bool b) { return __popcll(__builtin_amdgcn_ballot_w64(b)); };
    const int il = rank(light), in = rank(occluder), is = rank(sph), ip = rank(pln);
    const int ios = rank(sph && occluder), iop = rank(pln && occluder);
    if (sph) {
        S.sph[is] = sphere_geo;
        S.sph_id[is] = p;
        if (occluder) { S.osph[ios] = sphere_geo; S.osph_pos[ios] = in; }
    } else if (pln) {
        S.pln[ip] = plane_geo;
        S.pln_id[ip] = p;
        if (occluder) { S.opln[iop] = plane_geo; S.opln_pos[iop] = in; }
    }
    const int n = total(valid), nl = total(light), nn = total(occluder), ns = total(sph), np = total(pln);
    const int nos = total(sph && occluder), nop = total(pln && occluder);
    if (p == 0) {
        S.n = n; S.nlights = nl; S.nnonlight = nn;
        S.ns = ns; S.np = np; S.nos = nos; S.nop = nop;
    }
    return il;
}

// Block-cooperative copy of the scene image into LDS (coalesced 16-B loads).
template <class SceneT>
__device__ __forceinline__ void load_scene(SceneT &S, const SceneT *__restrict__ g)
{
    static_assert(sizeof(SceneT) % 16 == 0, "Scene image is copied in 16-B words");
    const uint4 *src = (const uint4 *)g;
    uint4 *dst = (uint4 *)&S;
    for (int i = threadIdx.x; i < (int)(sizeof(SceneT) / 16); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// Grid-stride zero fill (16-B stores) of up to three regions of n0, n1, n2
// words: a slab's counters and flag words in one launch (prep_kernel).
__device__ __forceinline__ void zero_fill(uint4 *__restrict__ z0, int n0, uint4 *__restrict__ z1, int n1,
                                          uint4 *__restrict__ z2 = nullptr, int n2 = 0)
{
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n0 + n1 + n2; i += gridDim.x * blockDim.x) {
        if (i < n0) z0[i] = zero;
        else if (i < n0 + n1) z1[i - n0] = zero;
        else z2[i - n0 - n1] = zero;
    }
}

}  // namespace prims
}  // namespace rt

#endif
