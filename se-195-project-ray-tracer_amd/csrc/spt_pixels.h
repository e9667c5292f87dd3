// spt_pixels.h -- a list of pixels, each with its own sample count
// (spt_scene_render_pixels_async): the camera statement of UpdateRenderingCPU
// (smallptCPU.cpp:84-105), spt_radiance.h's estimator and the fold of
// smallptCPU.cpp:110-118 for the pixels the caller lists, `take` samples each.
// Two parts.  The claim arithmetic below is plain integer code (SPT_HD, no HIP
// types): tests/native/pixel_claim_check.cpp includes this header under g++
// and sweeps it.  The kernel (under __HIPCC__) is not stand-alone: smallpt.hip
// includes this header inside namespace rt::smallpt, after spt_radiance.h --
// the queries and the shading are that header's functions as they are.
#ifndef SPT_PIXELS_H
#define SPT_PIXELS_H

#include "spt_policy.h"     // SPT_HD (smallpt.hip has it in already)

// ---------------------------------------------------------------------------
// The wave's sequence and the claim step.  64 consecutive list entries are a
// chunk; wave v of block b (W waves a block, G blocks) owns chunks b * W + v,
// + G * W, ...: a static sequence, so a launch keeps no state outside its
// registers.  The wave holds a cursor (chunk, pos), the same in every lane:
// positions [pos, 64) of `chunk` and everything in the chunks behind it are
// unclaimed.  In a claim step the lanes that want an entry are ranked (ballot,
// mbcnt); rank r takes position pos + r, a position >= 64 lying in the wave's
// next chunk -- at most one advance a step, since pos <= 64 and r <= 63.  An
// entry at or past nlist is "exhausted", and so is every later one: the
// entries a wave is handed grow strictly.
// ---------------------------------------------------------------------------
struct PixCursor {
    int chunk, pos;             // pos in [0, 64]
};

SPT_HD constexpr PixCursor pix_cursor(int first_chunk) { return PixCursor{first_chunk, 0}; }

// The entry the lane of rank `rank` takes, or -1: exhausted.  (64-bit: a
// chunk past the list's end times 64 may not fit an int.)
SPT_HD constexpr int pix_claim_entry(PixCursor c, int rank, int stride, int nlist)
{
    const int p = c.pos + rank;
    const long long e = p < 64 ? (long long)c.chunk * 64 + p : ((long long)c.chunk + stride) * 64 + (p - 64);
    return e < (long long)nlist ? (int)e : -1;
}

// The cursor after `count` lanes have claimed.  A wave that is exhausted
// claims no more, so chunk stays within one stride of the list's end.
SPT_HD constexpr PixCursor pix_claim_advance(PixCursor c, int count, int stride)
{
    return c.pos + count > 64 ? PixCursor{c.chunk + stride, c.pos + count - 64} : PixCursor{c.chunk, c.pos + count};
}

// One claim step for a whole wave, as the kernel's lanes take it together:
// entry[l] for every lane l of `need` (other lanes: untouched), the cursor
// advanced; returns whether a lane was told "exhausted".  (The host's form of
// the step: the kernel calls the two functions above with the hardware's
// rank and count.)
inline bool pix_claim_step(PixCursor &c, unsigned long long need, int stride, int nlist, int entry[64])
{
    int rank = 0;
    bool out = false;
    for (int l = 0; l < 64; l++) {
        if (!((need >> l) & 1)) continue;
        entry[l] = pix_claim_entry(c, rank++, stride, nlist);
        out |= entry[l] < 0;
    }
    c = pix_claim_advance(c, rank, stride);
    return out;
}

#ifdef __HIPCC__
// ---------------------------------------------------------------------------
// The kernel: radiance_kernel's blocks, LDS staging and one-query-per-
// iteration path state machine (spt_radiance.h), with two changes.
//
// A lane's ray is the camera's: at the start of every sample it draws the two
// jitter values and builds the ray -- render_kernel's pass B restated,
// operation for operation (x + fma(f, .5, -1.5) is x + (GetRandom() - .5f),
// exact; invW = 1.f / w) -- so a pixel's draws and float operations are the
// ones every other window runs for it.
//
// Takes differ per lane (0 next to 64; one lane at 40 among lanes at 1), so
// lanes do not wait for each other at the end of a chunk: a lane whose pixel
// is complete stores it (colour, seeds, sample count; d_pixels follows in the
// pack pass at the kernel's end) and claims the next unclaimed entry of its
// wave's sequence (above).  The claim step repeats before the next query
// until no lane wants an entry or the wave is exhausted -- a run of zero-take
// or out-of-range entries costs no query iteration -- and the wave ends when
// it is exhausted and no lane is live.  refill == 0 (a measuring hook): lanes
// claim only once no lane of the wave is live, the chunk-synchronous form.
//
// Per lane on top of the path: x, y, the sample number k and its end.  An
// idle lane has k == kend == 0; a lane whose pixel waits to be stored has
// k == kend > 0 (a listed pixel with a take of 0 is finished inside the claim
// step and never held).  The slot, the pixel index and the entry's take are
// recomputed or were folded into (k, kend); the camera comes from the kernel
// arguments (SGPRs).
//
// Why it is exact: a pixel owns its RNG words and its accumulator, the list
// is a set, and nothing else is shared; per pixel the statements are
// UpdateRenderingCPU's in its order.
// ---------------------------------------------------------------------------
struct PixelsArgs {
    rt_camera cam;
    float *colors;                // 3 floats per slot (h - y - 1) * w + x
    const uint32_t *seeds_in;     // 2 words per slot (may alias seeds_out)
    uint32_t *seeds_out;
    uint32_t *pixels;             // at y * w + x
    int w, h;
    const int32_t *list;          // nlist pixel indices y * w + x; outside [0, w * h): skipped
    const int32_t *take;          // null: every entry takes nsamples
    int nlist, nsamples;
    int32_t *done;                // null, or the pixel's currentSample per slot
    int first_sample;             // (done == null) the first sample's number
    int n, nlights;               // spheres, lights
    const float4 *soa;            // the scene's records (RadianceArgs)
    int opts;                     // wide_walk's options
    int refill;                   // 0: the chunk-synchronous form
};

// spt_scene_render_pixels_stats_async's arguments: the same, and the plane of
// second moments.  A type of its own, so that the plain kernels' argument
// block -- and with it their code -- stays what it was.
struct PixelsStatsArgs : PixelsArgs {
    float *m2;                    // 1 float per slot: the running mean of |R|^2
};
template <bool STATS> struct PixelsArgsOf { using type = PixelsArgs; };
template <> struct PixelsArgsOf<true> { using type = PixelsStatsArgs; };

// STATS: beside the colour the lane keeps m2, the running mean of the samples'
// |R|^2 folded with rad_fold's own factors (rad_fold1) -- read where the
// colour is read, stored where it is stored.  One more live float and one
// more pointer; every other statement is the plain kernel's, so colours,
// seeds, pixels and counts are its bits.
template <int GEO, bool DL, bool STATS>
__global__ void __launch_bounds__(64 * query_wpb(GEO))
pixels_kernel(typename PixelsArgsOf<STATS>::type a, BvhView bvh)
{
    extern __shared__ __attribute__((aligned(16))) char rmem[];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), wpb = (int)(blockDim.x >> 6);
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
    const float invW = 1.f / a.w, invH = 1.f / a.h;             // smallptCPU.cpp:80-81
    const unsigned npix = (unsigned)a.w * (unsigned)a.h;
    const int stride = (int)gridDim.x * wpb;
    PixCursor cur = pix_cursor((int)blockIdx.x * wpb + wave);
    bool exhausted = false;                                     // (the same in every lane, as cur is)
    int x = 0, y = 0, k = 0, kend = 0;
    bool need_cam = false;                                      // the lane's next sample has no ray yet
    uint32_t s0 = 0, s1 = 0;
    v3 col = mk(0.f, 0.f, 0.f);
    float m2 = 0.f;                                             // (STATS)
    RadPath P;
    P.nl = P.lsum = mk(0.f, 0.f, 0.f);
    P.lmax = P.lw = 0.f;
    P.li = 0;
    rad_begin(P, idle);
    while (true) {
        // ---- claim steps: lanes out of samples store their pixel and take
        // the next entries of the wave's sequence
        while (true) {
            const bool want = k >= kend;
            if (want && kend > 0) {                             // a complete pixel: smallptCPU.cpp:119-122
                const size_t i = (size_t)(a.h - y - 1) * a.w + x;
                a.colors[3 * i] = col.x;
                a.colors[3 * i + 1] = col.y;
                a.colors[3 * i + 2] = col.z;
                a.seeds_out[2 * i] = s0;
                a.seeds_out[2 * i + 1] = s1;
                if (a.done) a.done[i] = kend;
                if constexpr (STATS) a.m2[i] = m2;
                k = kend = 0;
            }
            if (exhausted) break;
            if (!a.refill && wave_any(!want)) break;
            const unsigned long long need = __builtin_amdgcn_ballot_w64(want);
            if (!need) break;
            const int count = __builtin_popcountll(need);
            const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(need >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)need, 0u));
            bool out = false;
            if (want) {
                const int e = pix_claim_entry(cur, rank, stride, a.nlist);
                out = e < 0;
                if (!out) {
                    const int p = a.list[e];
                    int t = a.nsamples;
                    if (a.take) t = a.take[e] > 0 ? a.take[e] : 0;
                    if ((unsigned)p < npix) {
                        const int py = p / a.w, px = p - py * a.w;
                        const size_t i = (size_t)(a.h - py - 1) * a.w + px;
                        const uint32_t r0 = a.seeds_in[2 * i], r1 = a.seeds_in[2 * i + 1];
                        if (t == 0) {                           // the seeds are copied, nothing else is written
                            a.seeds_out[2 * i] = r0;
                            a.seeds_out[2 * i + 1] = r1;
                        } else {
                            const int base = a.done ? a.done[i] : a.first_sample;
                            x = px;
                            y = py;
                            s0 = r0;
                            s1 = r1;
                            col = mk(0.f, 0.f, 0.f);
                            if (base > 0) col = mk(a.colors[3 * i], a.colors[3 * i + 1], a.colors[3 * i + 2]);
                            if constexpr (STATS) m2 = base > 0 ? a.m2[i] : 0.f;
                            k = base;
                            kend = base + t;
                            need_cam = true;
                        }
                    }
                }
            }
            cur = pix_claim_advance(cur, count, stride);
            exhausted = wave_any(out);
        }
        // ---- the sample's camera ray (smallptCPU.cpp:89-105; render_kernel's
        // pass B).  A ray with a non-finite component hits nothing
        // (spt_radiance.h): its sample is the miss's zeros, and the lane
        // draws for its next one.
        while (need_cam) {
            const float f1 = get_random_f(s0, s1), f2 = get_random_f(s0, s1);
            const float kcx = (x + __builtin_fmaf(f1, .5f, -1.5f)) * invW - .5f;    // r1 = GetRandom() - .5f
            const float kcy = (y + __builtin_fmaf(f2, .5f, -1.5f)) * invH - .5f;
            const v3 rdir = mk(a.cam.x.x * kcx + a.cam.y.x * kcy + a.cam.dir.x,
                               a.cam.x.y * kcx + a.cam.y.y * kcy + a.cam.dir.y,
                               a.cam.x.z * kcx + a.cam.y.z * kcy + a.cam.dir.z);
            const v3 vn = vnorm(rdir);
            v3 rorig = vsmul(0.1f, rdir);
            rorig = vadd(rorig, mk(a.cam.orig.x, a.cam.orig.y, a.cam.orig.z));
            const bool finite = fabsf(rorig.x) < MISS && fabsf(rorig.y) < MISS && fabsf(rorig.z) < MISS &&
                                fabsf(vn.x) < MISS && fabsf(vn.y) < MISS && fabsf(vn.z) < MISS;
            if (finite) {
                P.ray.o = rorig;
                P.ray.d = vn;
                need_cam = false;
            } else {
                rad_fold(col, mk(0.f, 0.f, 0.f), k);
                if constexpr (STATS) rad_fold1(m2, 0.f, k);
                k++;
                need_cam = k < kend;
            }
        }
        const bool live = k < kend;
        if (!wave_any(live)) {
            if (exhausted && !wave_any(kend > 0)) break;
            continue;                                           // (pixels to store, or entries left to claim)
        }
        // ---- one query per live lane and the reference's code for its answer: radiance_kernel's body
        float t = P.shadow ? P.lmax : 1e20f;
        const int id = rad_query<GEO>(geo, bvh, wL, wstk, a.opts, P.ray, P.shadow, t, live);
        if (live) {
            int next;
            if (P.shadow) {                                     // :157-162: the light is visible
                if (id < 0) {
                    const float4 le = S.lrec[3 * P.li + 2];
                    P.lsum = vadd(P.lsum, vsmul(P.lw, mk(le.x, le.y, le.z)));
                }
                P.li++;
                P.shadow = false;
                next = RAD_LIGHTS;
            } else if (id < 0) {                                // :191-194
                next = RAD_DONE;
            } else {
                next = rad_hit(S, P, t, id, s0, s1);
            }
            if (next == RAD_LIGHTS && !rad_sample_lights(S, P, s0, s1))
                next = rad_diffuse<DL>(P, s0, s1) ? RAD_DONE : RAD_RAY;
            if (next == RAD_DONE) {
                rad_fold(col, P.rad, k);
                if constexpr (STATS) rad_fold1(m2, (P.rad.x * P.rad.x + P.rad.y * P.rad.y) + P.rad.z * P.rad.z, k);
                k++;
                need_cam = k < kend;                            // the next sample's ray: drawn above; else the lane idles
                rad_begin(P, idle);
            }
        }
    }
    // ---- the pack pass (smallptCPU.cpp:119-122): d_pixels of every pixel the
    // wave stored, from the colour it stored, over the wave's chunks again.
    // Kept out of the loop above: toInt's powf holds ten registers of
    // constants that would otherwise live across every query.  The colours
    // were written by lanes of this wave (release / acquire at workgroup scope
    // orders them before the loads below); a pixel's pack is a function of its
    // final colour alone.
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const int nchunks = (int)(((unsigned)a.nlist + 63u) >> 6);
    for (int c = (int)blockIdx.x * wpb + wave; c < nchunks; c += stride) {
        const int e = c * 64 + (int)(threadIdx.x & 63);
        if (e >= a.nlist) break;
        const int p = a.list[e];
        const int t = a.take ? a.take[e] : a.nsamples;
        if ((unsigned)p < npix && t > 0) {
            const int py = p / a.w, px = p - py * a.w;
            const float *c3 = a.colors + 3 * ((size_t)(a.h - py - 1) * a.w + px);
            a.pixels[p] = pack_rgb(c3[0], c3[1], c3[2]);
        }
    }
}
#endif  // __HIPCC__

#endif  // SPT_PIXELS_H
