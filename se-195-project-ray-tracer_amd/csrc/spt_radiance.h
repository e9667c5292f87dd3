// spt_radiance.h -- radiance queries on a prepared smallpt scene
// (spt_scene_radiance_async): the reference's estimator, RadiancePathTracing
// (geomfunc.h:167-338) or RadianceDirectLighting (:340-483), along rays the
// caller supplies, folded into the caller's running average as
// smallptCPU.cpp:110-118 folds a pixel's samples.  Not a stand-alone header:
// smallpt.hip includes it inside namespace rt::smallpt, after spt_query.h --
// the sphere loop (query_bf) and the walks (bvh_walk, wide_walk) are
// render_kernel's own; the shading below is a restatement of geomfunc.h in the
// reference's order, one small function per step, with render_kernel's exact
// primitives (get_random, sqrt_exact, rcp_nr, rtm::sincos_2pi_draw, vnorm).
#ifndef SPT_RADIANCE_H
#define SPT_RADIANCE_H

// ---------------------------------------------------------------------------
// Mapping: query_kernel's.  64 consecutive rays are a chunk, one per lane;
// wave v of block b takes chunks b * W + v, + G * W, ...; blocks are
// persistent and stage their family's LDS copy once (spt_layout.h
// radiance_lds_bytes): the four record arrays (GEO_LDS) or the 8-wide nodes
// (GEO_WIDE, materials from global memory).
//
// Per lane a path state machine, render_kernel's one-query form: every
// iteration of the wave's loop issues exactly one query per live lane -- the
// path ray's nearest hit (Intersect) or, while a DIFF vertex samples its
// lights, the shadow ray of the light it is at (IntersectP: the same query
// with the bound len - EPS, "some sphere was taken") -- so the scan families'
// wave-uniform sphere loop runs with every lane, and the resumable walks are
// called until no lane of the wave is left walking.  Between two queries a
// lane runs the reference's code for what the query answered, draws included,
// up to the next ray it needs; a lane that ends sample j starts sample j + 1
// at once, and lanes wait for each other only at the end of a chunk.
//
// Why it is exact: per lane the float operations and the draws are the
// reference's, in its order (the statements below are geomfunc.h's, line by
// line); a query returns what the full scan returns (spt_query.h); and no
// state is shared between lanes.  A ray with a non-finite component hits
// nothing under SphereIntersect (spt_query.h): its samples are the miss's
// zeros and it never reaches a walk.
// ---------------------------------------------------------------------------
struct RadianceArgs {
    const float *rays;            // 6 floats per ray: o.xyz, d.xyz
    const uint32_t *seeds_in;     // 2 words per ray (may alias seeds_out)
    uint32_t *seeds_out;
    float *radiance;              // 3 floats per ray, the running average
    int nrays, first_sample, nsamples;
    int n, nlights;               // spheres, lights
    const float4 *soa;            // the scene's records: geo | emi | col (n each) | lrec (3 per light)
    int opts;                     // wide_walk's options (spt_policy.h's split word)
};

// A path between two queries.
struct RadPath {
    ray3 ray;                     // the ray queried next (after a hit: from the hit point)
    v3 rad, thr;                  // rad, throughput
    v3 nl;                        // the DIFF vertex's oriented normal (SampleLights, the bounce)
    v3 lsum;                      // SampleLights' *result so far
    float lmax, lw;               // the pending shadow ray's maxt = len - EPSILON and its light's weight s (:159)
    int depth, li;                // li: the light (in the scene's light list) SampleLights is at
    bool specular, shadow;        // specularBounce; `ray` is light li's shadow ray
};
enum { RAD_RAY, RAD_LIGHTS, RAD_DONE };     // what a step leaves: a path ray to query, lights to sample, the sample's end

__device__ __forceinline__ void rad_begin(RadPath &P, const ray3 &start)        // :176-181
{
    P.ray = start;
    P.rad = mk(0.f, 0.f, 0.f);
    P.thr = mk(1.f, 1.f, 1.f);
    P.depth = 0;
    P.specular = true;
    P.shadow = false;
}

// sqrt(d2) and 1.f / that (:145-146), bit-exact: the short forms unless a
// lane of the wave is outside their range.
__device__ __forceinline__ void rad_len_inv(float d2, float &len, float &inv)
{
    if (!wave_any(!sqrt_nr_ok(d2))) {
        len = sqrt_nr(d2);
        inv = rcp_nr(len);
    } else {
        len = sqrt_rn(d2);
        inv = 1.f / len;
    }
}

// The REFR branch (:281-336, :426-481) at hit point `hit` of sphere colour c.
__device__ __forceinline__ void rad_refract(RadPath &P, const v3 hit, const v3 normal, const v3 nl, const v3 c,
                                            uint32_t &s0, uint32_t &s1)
{
    v3 newDir = vsmul(2.f * vdot(normal, P.ray.d), normal);
    newDir = vsub(P.ray.d, newDir);                             // reflRay: (hit, newDir)
    const bool into = vdot(normal, nl) > 0;
    const float nc = 1.f, nt = 1.5f;
    const float nnt = into ? nc / nt : nt / nc;
    const float ddn = vdot(P.ray.d, nl);
    const float cos2t = 1.f - nnt * nnt * (1.f - ddn * ddn);
    if (cos2t < 0.f) {                                          // total internal reflection
        P.thr = vmul(P.thr, c);
        P.ray.o = hit;
        P.ray.d = newDir;
        return;
    }
    const float kk = (into ? 1.f : -1.f) * (ddn * nnt + sqrt_exact(cos2t));
    const v3 nkk = vsmul(kk, normal);
    v3 transDir = vsmul(nnt, P.ray.d);
    transDir = vsub(transDir, nkk);
    transDir = vnorm(transDir);
    const float a = nt - nc, b = nt + nc;
    const float R0 = a * a / (b * b);
    const float cc = 1 - (into ? -ddn : vdot(transDir, normal));
    const float Re = R0 + (1 - R0) * cc * cc * cc * cc * cc;
    const float Tr = 1.f - Re;
    const float Pr = .25f + .5f * Re;
    const float RP = Re / Pr;
    const float TP = Tr / (1.f - Pr);
    if (get_random(s0, s1) < Pr) {                              // R.R.
        P.thr = vsmul(RP, P.thr);
        P.thr = vmul(P.thr, c);
        P.ray.d = newDir;
    } else {
        P.thr = vsmul(TP, P.thr);
        P.thr = vmul(P.thr, c);
        P.ray.d = transDir;
    }
    P.ray.o = hit;
}

// One loop body of :182-337 / :355-482 after Intersect found sphere id at t:
// up to the `continue` of a SPEC or REFR hit, or to SampleLights' call.
__device__ __forceinline__ int rad_hit(const Scene &S, RadPath &P, float t, int id, uint32_t &s0, uint32_t &s1)
{
    const float4 og = S.geo[id], oe = S.emi[id], oc = S.col[id];
    v3 hit = vsmul(t, P.ray.d);
    hit = vadd(P.ray.o, hit);
    v3 normal = vsub(hit, mk(og.x, og.y, og.z));
    normal = vnorm(normal);
    const float dp = vdot(normal, P.ray.d);
    const float invSignDP = -1.f * (dp > 0 ? 1.f : -1.f);
    const v3 nl = vsmul(invSignDP, normal);
    if (!((oe.x == 0.f) && (oe.x == 0.f) && (oe.z == 0.f))) {  // viszero (vec.h: x twice, as written there)
        if (P.specular) {
            v3 e = vsmul(fabsf(dp), mk(oe.x, oe.y, oe.z));
            e = vmul(P.thr, e);
            P.rad = vadd(P.rad, e);
        }
        return RAD_DONE;
    }
    const v3 c = mk(oc.x, oc.y, oc.z);
    const int refl = __float_as_int(oe.w);
    P.depth++;                                                  // (the for's ++depth, taken at its `continue`)
    if (refl == DIFF) {
        P.specular = false;
        P.thr = vmul(P.thr, c);
        P.ray.o = hit;
        P.nl = nl;
        P.lsum = mk(0.f, 0.f, 0.f);                             // :122
        P.li = 0;
        return RAD_LIGHTS;
    }
    P.specular = true;
    if (refl == SPEC) {
        v3 newDir = vsmul(2.f * vdot(normal, P.ray.d), normal);
        newDir = vsub(P.ray.d, newDir);
        P.thr = vmul(P.thr, c);
        P.ray.o = hit;
        P.ray.d = newDir;
    } else {
        rad_refract(P, hit, normal, nl, c, s0, s1);
    }
    return P.depth > 6 ? RAD_DONE : RAD_RAY;                    // :184 at the next bounce
}

// SampleLights (:112-165) from light P.li on, up to the next light that needs
// its shadow test: true with P.ray that shadow ray, false when the lights are
// through.  UniformSampleSphere's two arguments are drawn second-first, as
// the g++-built oracle evaluates them (:138).
__device__ __forceinline__ bool rad_sample_lights(const Scene &S, RadPath &P, uint32_t &s0, uint32_t &s1)
{
    while (P.li < S.nlights) {
        const float4 lg = S.lrec[3 * P.li], lc = S.lrec[3 * P.li + 1];      // centre; colour.xyz, rad
        const float u2 = get_random(s0, s1);
        const float u1 = get_random(s0, s1);
        const float zz = 1.f - 2.f * u1;                        // :61-69
        const float q = 1.f - zz * zz;
        const float r = sqrt_exact((0.f > q) ? 0.f : q);
        float sn, cs;                                           // of phi = 2 PI u2
        rtm::sincos_2pi_draw(u2, sn, cs);
        const v3 unit = mk(r * cs, r * sn, zz);
        v3 sp = vsmul(lc.w, unit);
        sp = vadd(sp, mk(lg.x, lg.y, lg.z));
        v3 sd = vsub(sp, P.ray.o);                              // shadowRay.d
        float len, ilen;
        rad_len_inv(vdot(sd, sd), len, ilen);
        sd = vsmul(ilen, sd);
        float wo = vdot(sd, unit);
        if (!(wo > 0.f)) {                                      // (else: the other half of the sphere)
            wo = -wo;
            const float wi = vdot(sd, P.nl);
            if (wi > 0.f) {
                P.ray.d = sd;
                P.lmax = len - EPS;
                P.lw = (4.f * PI_F * lc.w * lc.w) * wi * wo / (len * len);
                P.shadow = true;
                return true;
            }
        }
        P.li++;
    }
    return false;
}

// The DIFF branch behind SampleLights (:237-269, :410-414): true when the
// sample ends here, else P.ray is the bounce.
template <bool DL>
__device__ __forceinline__ bool rad_diffuse(RadPath &P, uint32_t &s0, uint32_t &s1)
{
    P.rad = vadd(P.rad, vmul(P.thr, P.lsum));
    if (DL) return true;
    const float u1 = get_random(s0, s1);                        // r1 = 2 PI u1
    const float r2 = get_random(s0, s1);
    if (P.depth > 6) return true;                               // :184 (the draws are taken before it)
    const float r2s = sqrt_exact(r2);
    const v3 w = P.nl;
    const v3 a = (fabsf(w.x) > .1f) ? mk(0.f, 1.f, 0.f) : mk(1.f, 0.f, 0.f);
    v3 u = vxcross(a, w);
    u = vnorm(u);
    v3 v = vxcross(w, u);
    float sn, cs;
    rtm::sincos_2pi_draw(u1, sn, cs);
    u = vsmul(cs * r2s, u);
    v = vsmul(sn * r2s, v);
    v3 newDir = vadd(u, v);
    newDir = vadd(newDir, vsmul(sqrt_nr(1 - r2), w));          // 1 - r2 in [2^-23, 1]: sqrt_nr's range
    P.ray.d = newDir;                                           // origin: the hit point
    return false;
}

// smallptCPU.cpp:110-118 for sample number `current`, per component
// (render_kernel's form: 1.f / (k1 + 1.f) through rcp_nr, exact on its range).
__device__ __forceinline__ void rad_fold(v3 &col, const v3 r, int current)
{
    if (current == 0) {
        col = r;
    } else {
        const float k1 = (float)current;
        const float k2 = rcp_nr(k1 + 1.f);
        col.x = (col.x * k1 + r.x) * k2;
        col.y = (col.y * k1 + r.y) * k2;
        col.z = (col.z * k1 + r.z) * k2;
    }
}

// The same fold for one scalar with rad_fold's own k1, k2: the running mean of
// a per-sample quantity kept beside the colour (spt_pixels.h's second moment).
__device__ __forceinline__ void rad_fold1(float &m, const float q, int current)
{
    if (current == 0) {
        m = q;
    } else {
        const float k1 = (float)current;
        const float k2 = rcp_nr(k1 + 1.f);
        m = (m * k1 + q) * k2;
    }
}

// One query for every lane with `want` set: the nearest hit below t, or
// (shadow) any hit below t; returns the sphere (negative: none) and the
// distance in t.  Scan families: the loop runs with every lane (a lane
// without a query holds a stand-in ray; its result is dropped).  Hierarchy
// families: the uncounted resumable walks, to the end; the nearest hit starts
// at the float below t, so that it takes d < t strictly (spt_query.h).
template <int GEO>
__device__ __forceinline__ int rad_query(const DynGeo &geo, const BvhView &bvh, const uint4 *wL, unsigned *wstk,
                                         int opts, const ray3 &ray, bool shadow, float &t, bool want)
{
    if constexpr (GEO == GEO_LDS || GEO == GEO_GLOBAL) {
        int first = -1;
        return query_bf<false, true>(geo, ray, t, first);
    } else {
        BvhWalk W = {};
        bool walking = want;
        const float start = shadow ? t : __uint_as_float(__float_as_uint(t) - 1u);
        if constexpr (GEO == GEO_BVH) {
            if (want) bvh_begin<false>(bvh, ray, shadow, start, W);
            while (wave_any(walking)) {
                if (walking) walking = !bvh_walk<false>(bvh, ray, shadow, W);
            }
        } else {
            if (want) wide_begin<false>(bvh, ray, shadow, start, W);
            while (wave_any(walking)) {
                if (walking) walking = !wide_walk<false>(bvh, wL, wstk, ray, shadow, W, opts);
            }
        }
        if (!want) return -1;
        t = W.t;
        return W.id;
    }
}

template <int GEO, bool DL>
__global__ void __launch_bounds__(64 * query_wpb(GEO)) radiance_kernel(RadianceArgs a, BvhView bvh)
{
    extern __shared__ __attribute__((aligned(16))) char rmem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wpb = blockDim.x >> 6;
    Scene S;
    S.geo = a.soa; S.emi = a.soa + a.n; S.col = a.soa + 2 * a.n; S.lrec = a.soa + 3 * a.n;
    S.n = a.n;
    S.nlights = a.nlights;
    const uint4 *wL = (const uint4 *)rmem;
    unsigned *wstk = nullptr;
    if constexpr (GEO == GEO_LDS) {                             // the four record arrays, as render_kernel stages them
        float4 *s = (float4 *)rmem;
        const int nrec = scene_records(a.n, a.nlights);
        for (int i = threadIdx.x; i < nrec; i += blockDim.x) s[i] = a.soa[i];
        __syncthreads();
        S.geo = s; S.emi = s + a.n; S.col = s + 2 * a.n; S.lrec = s + 3 * a.n;
    }
    if constexpr (GEO == GEO_WIDE) {
        uint4 *d = (uint4 *)rmem;
        for (int i = threadIdx.x; i < 7 * bvh.wnodes; i += blockDim.x) d[i] = bvh.wnode[i];
        wstk = (unsigned *)(rmem + wide_stack_offset(bvh.wnodes, false)) +
               (size_t)wave * WIDE_LEVEL_DW * (bvh.wdepth > 1 ? bvh.wdepth - 1 : 1);
        __syncthreads();
    }
    const DynGeo geo{S.geo, S.n};
    ray3 idle;                                                  // what a lane without a query holds
    idle.o = mk(0.f, 0.f, 0.f);
    idle.d = mk(0.f, 0.f, 1.f);
    const int nchunks = (int)(((unsigned)a.nrays + 63u) >> 6);
    for (int c = (int)blockIdx.x * wpb + wave; c < nchunks; c += (int)gridDim.x * wpb) {
        const size_t r = (size_t)c * 64 + lane;
        const bool valid = r < (size_t)a.nrays;
        ray3 start = idle;
        uint32_t s0 = 0, s1 = 0;
        v3 col = mk(0.f, 0.f, 0.f);
        if (valid) {
            const float *p = a.rays + 6 * r;
            start.o = mk(p[0], p[1], p[2]);
            start.d = mk(p[3], p[4], p[5]);
            s0 = a.seeds_in[2 * r];
            s1 = a.seeds_in[2 * r + 1];
            if (a.first_sample > 0) col = mk(a.radiance[3 * r], a.radiance[3 * r + 1], a.radiance[3 * r + 2]);
        }
        const bool finite = fabsf(start.o.x) < MISS && fabsf(start.o.y) < MISS && fabsf(start.o.z) < MISS &&
                            fabsf(start.d.x) < MISS && fabsf(start.d.y) < MISS && fabsf(start.d.z) < MISS;
        const int ns = valid ? a.nsamples : 0;
        int k = 0;
        if (!finite) {                                          // every sample is the miss: zeros, no draw
            for (; k < ns; k++) rad_fold(col, mk(0.f, 0.f, 0.f), a.first_sample + k);
        }
        RadPath P;
        P.nl = P.lsum = mk(0.f, 0.f, 0.f);
        P.lmax = P.lw = 0.f;
        P.li = 0;
        rad_begin(P, k < ns ? start : idle);
        while (wave_any(k < ns)) {
            const bool live = k < ns;
            float t = P.shadow ? P.lmax : 1e20f;
            const int id = rad_query<GEO>(geo, bvh, wL, wstk, a.opts, P.ray, P.shadow, t, live);
            if (live) {
                int next;
                if (P.shadow) {                                 // :157-162: the light is visible
                    if (id < 0) {
                        const float4 le = S.lrec[3 * P.li + 2];
                        P.lsum = vadd(P.lsum, vsmul(P.lw, mk(le.x, le.y, le.z)));
                    }
                    P.li++;
                    P.shadow = false;
                    next = RAD_LIGHTS;
                } else if (id < 0) {                            // :191-194
                    next = RAD_DONE;
                } else {
                    next = rad_hit(S, P, t, id, s0, s1);
                }
                if (next == RAD_LIGHTS && !rad_sample_lights(S, P, s0, s1))
                    next = rad_diffuse<DL>(P, s0, s1) ? RAD_DONE : RAD_RAY;
                if (next == RAD_DONE) {
                    rad_fold(col, P.rad, a.first_sample + k);
                    k++;
                    // the next sample's path from the caller's ray again (re-read: six registers
                    // less across the loop); a lane out of samples idles
                    if (k < ns) {
                        const float *p = a.rays + 6 * r;
                        start.o = mk(p[0], p[1], p[2]);
                        start.d = mk(p[3], p[4], p[5]);
                    }
                    rad_begin(P, k < ns ? start : idle);
                }
            }
        }
        if (valid) {
            if (a.nsamples > 0) {
                a.radiance[3 * r] = col.x;
                a.radiance[3 * r + 1] = col.y;
                a.radiance[3 * r + 2] = col.z;
            }
            a.seeds_out[2 * r] = s0;
            a.seeds_out[2 * r + 1] = s1;
        }
    }
}

#endif  // SPT_RADIANCE_H
