// spt_refit_check.cpp -- test-only CPU checks of the hierarchy refit
// (csrc/spt_refit.h): the sections spt_scene_create uploads are assembled here
// as build_scene_bvh assembles them, refitted on the host with refit_host, and
// checked: containment of every box in long double, and scalar restatements
// of the device walks (spt_walk.h's 8-wide and binary walks, minus the wave
// scheduling) over the refitted sections against the reference's full scan
// (geomfunc.h:71-110) ray by ray.  tests/test_refit.py builds this file into a
// shared library with g++ -O2 -std=c++17 -ffp-contract=off -pthread; with
// -DSPT_REFIT_MAIN it is a stand-alone program (its own scenes and edits) for
// a run under -fsanitize=address,undefined,float-cast-overflow
// (tests/test_degenerate.py).
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>
#include "spt_bvh.h"
#include "spt_policy.h"
#include "spt_refit.h"

namespace {

constexpr float EPS = 0.01f;     // geom.h:29
constexpr float MISS = INFINITY;

float sphere_hit(const rt_sphere &s, const float *o, const float *d)
{
    // SphereIntersect, geomfunc.h:32-59 (a miss as +inf)
    const float opx = s.p.x - o[0], opy = s.p.y - o[1], opz = s.p.z - o[2];
    const float b = opx * d[0] + opy * d[1] + opz * d[2];
    float det = b * b - (opx * opx + opy * opy + opz * opz) + s.rad * s.rad;
    if (det < 0.f) return MISS;
    det = sqrtf(det);
    float t = b - det;
    if (t > EPS) return t;
    t = b + det;
    return t > EPS ? t : MISS;
}

float f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

struct State {
    int n = 0, nn = 0, nb = 0, na = 0, wn = 0, wdepth = 0, leaf_max = 0;
    std::vector<rt_sphere> sp;
    // the five sections: node records (8 floats each, eight layouts), geo (4
    // floats per entry, tree entries then always entries), ids, wide words, maxid
    std::vector<float> nodes, geo;
    std::vector<int> ids;
    std::vector<uint32_t> words, maxid;
    sptrefit::Meta meta;
    std::vector<float> nbox;     // 8 floats per binary node: lo | margin, hi | 0
};

// As build_scene_bvh (csrc/smallpt.hip) assembles what it uploads.
State *create(const rt_sphere *sp, int n, int wide)
{
    State *S = new State();
    S->n = n;
    S->sp.assign(sp, sp + n);
    std::vector<int> always;
    sptbvh::BvhBuild b;
    sptbvh::partition_and_build(S->sp.data(), n, always, b);
    S->nn = (int)b.nodes.size();
    S->nb = (int)b.idx.size();
    S->na = (int)always.size();
    for (int oct = 0; oct < 8; oct++) {
        std::vector<sptbvh::f4> lay;
        if (S->nn) b.emit(0, oct, lay);
        for (const sptbvh::f4 &v : lay) { S->nodes.push_back(v.x); S->nodes.push_back(v.y); S->nodes.push_back(v.z); S->nodes.push_back(v.w); }
    }
    sptbvh::WideBuild wb;
    if (wide) S->leaf_max = sptbvh::choose_wide(b, wb, sptpolicy::WIDE_WPB);
    if (S->leaf_max) {
        S->words = wb.words;
        S->maxid = wb.maxid;
        S->wn = wb.nnodes;
        S->wdepth = wb.depth;
    }
    for (int j = 0; j < S->nb + S->na; j++) {
        const int i = j < S->nb ? b.idx[j] : always[j - S->nb];
        const rt_sphere &q = S->sp[i];
        S->geo.push_back(q.p.x); S->geo.push_back(q.p.y); S->geo.push_back(q.p.z);
        S->geo.push_back(q.rad * q.rad);
        S->ids.push_back(i);
    }
    if (!sptrefit::build_meta(b, S->na, S->wn ? S->words.data() : nullptr, S->wn, S->meta)) {
        delete S;
        return nullptr;
    }
    S->nbox.assign(8 * (size_t)S->nn, 0.f);
    for (int i = 0; i < S->nn; i++) {
        const sptbvh::HostNode &h = b.nodes[i];
        float *o = &S->nbox[8 * (size_t)i];
        for (int k = 0; k < 3; k++) { o[k] = h.lo[k]; o[4 + k] = h.hi[k]; }
        o[3] = h.margin;
    }
    return S;
}

void refit(State *S, const rt_sphere *sp)
{
    S->sp.assign(sp, sp + S->n);
    sptrefit::refit_host(S->meta, S->sp.data(), S->nodes.data(), S->geo.data(), S->ids.data(),
                         S->wn ? S->words.data() : nullptr, S->nbox);
}

// Containment of the current sections around the current spheres, in long
// double.  Returns the number of violations; msg receives the first.
long long check(const State *S, char *msg, int cap)
{
    long long bad = 0;
    auto fail = [&](const char *what, int a, int b) {
        if (!bad && msg && cap > 0) snprintf(msg, cap, "%s (node %d, item %d)", what, a, b);
        bad++;
    };
    const sptrefit::Meta &m = S->meta;
    for (int i = 0; i < S->nn; i++) {
        const float *o = &S->nbox[8 * (size_t)i];
        for (int j = m.range[2 * i]; j < m.range[2 * i + 1]; j++) {
            const rt_sphere &q = S->sp[S->ids[j]];
            const float c[3] = {q.p.x, q.p.y, q.p.z};
            // The float box c -+ |rad| (the reference uses rad only as rad *
            // rad).  Exempt only where a component of that box is not finite:
            // such a sphere is never hit (rad * rad or |p - o|^2 is inf or NaN).
            const float r = fabsf(q.rad);
            bool finite = true;
            for (int k = 0; k < 3; k++) finite = finite && std::isfinite(c[k] - r) && std::isfinite(c[k] + r);
            if (!finite) continue;
            for (int k = 0; k < 3; k++) {
                if (!((long double)o[k] <= (long double)(c[k] - r) && (long double)o[4 + k] >= (long double)(c[k] + r)))
                    fail("a binary node's box does not contain a sphere of its range", i, j);
            }
        }
        // spt_bvh.h's margin formula on this box.  The builder's own margin is
        // that value rounded to the nearest float, so "at least the formula"
        // holds to within that one rounding: the next float up must reach it.
        long double d2 = 0, mag = 0;
        for (int k = 0; k < 3; k++) {
            const long double e = (long double)(float)(o[4 + k] - o[k]);     // the float extent of spt_bvh.h:90
            d2 += e * e;
            mag = std::max(mag, (long double)std::max(fabsf(o[k]), fabsf(o[4 + k])));
        }
        const long double want = (long double)sptbvh::ALPHA_R * 0.5L * sqrtl(d2) + 1e-3L + 1e-5L * mag;
        if (!((long double)nextafterf(o[3], INFINITY) >= want)) fail("margin below the builder's formula", i, 0);
        // the records hold this box and margin in all eight layouts
        float c[3], h[3];
        sptrefit::node_record(o, o + 4, c, h);
        for (int oct = 0; oct < 8; oct++) {
            const float *r = &S->nodes[8 * (size_t)m.pos[8 * (size_t)i + oct]];
            if (memcmp(r, c, 12) || memcmp(r + 4, h, 12) || memcmp(r + 7, o + 3, 4)) fail("a layout's record differs", i, oct);
        }
    }
    for (int w = 0; w < S->wn; w++) {
        const uint32_t *ww = &S->words[(size_t)w * sptbvh::WIDE_WORDS];
        const int *slot = &m.wslot[8 * (size_t)w];
        // (the float constants: a node whose children are all empty holds them exactly)
        const long double elo = sptbvh::BOX_EMPTY_LO, ehi = sptbvh::BOX_EMPTY_HI;
        long double lo[3] = {elo, elo, elo}, hi[3] = {ehi, ehi, ehi};
        for (int s = 0; s < 8; s++) {
            if (slot[s] < 0) continue;
            const float *o = &S->nbox[8 * (size_t)slot[s]];
            for (int k = 0; k < 3; k++) {
                lo[k] = std::min(lo[k], (long double)o[k]);
                hi[k] = std::max(hi[k], (long double)o[4 + k]);
                const long double sc = ldexpl(1.0L, (int)((ww[3] >> (8 * k)) & 255u) - 127);
                const long double p = (long double)f32(ww[k]);
                const uint32_t ql = (ww[16 + 6 * (s >> 2) + k] >> (8 * (s & 3))) & 255u;
                const uint32_t qh = (ww[16 + 6 * (s >> 2) + 3 + k] >> (8 * (s & 3))) & 255u;
                if (!(p + ql * sc <= (long double)o[k] && p + qh * sc >= (long double)o[4 + k]))
                    fail("a quantised child box does not contain its binary node's box", w, s);
            }
            if (!(f32(ww[5]) >= o[3])) fail("K below a child's margin", w, s);
            if (!((ww[3] >> (24 + s)) & 1u)) fail("a filled slot is not valid", w, s);
        }
        long double d2 = 0;
        for (int k = 0; k < 3; k++) d2 += (hi[k] - lo[k]) * (hi[k] - lo[k]);
        if (!((long double)f32(ww[4]) >= sqrtl(d2))) fail("D0 below the node diagonal", w, 0);
        for (int k = 0; k < 3; k++)
            if (!((long double)f32(ww[k]) <= lo[k])) fail("the frame origin is above a child's low corner", w, k);
    }
    return bad;
}

struct Ray {
    float inv[3], alpha;
    int oct;
};

Ray walk_ray(const float *d)
{
    Ray r;
    float dv[3];
    for (int k = 0; k < 3; k++) dv[k] = fabsf(d[k]) < 1e-30f ? copysignf(1e-30f, d[k]) : d[k];
    for (int k = 0; k < 3; k++) r.inv[k] = 1.f / dv[k];
    const float e = fabsf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2] - 1.f);
    r.alpha = e < 0x1p-16f ? 2.f * (1.04e-3f + sqrtf(e + 0x1p-22f)) : 1e30f;
    r.oct = (dv[0] < 0.f ? 1 : 0) | (dv[1] < 0.f ? 2 : 0) | (dv[2] < 0.f ? 4 : 0);
    return r;
}

void take(const State *S, int j, const float *o, const float *d, bool shadow, float maxt, float &t, int &id)
{
    const int i = S->ids[j];
    const float dd = sphere_hit(S->sp[i], o, d);
    if (shadow) {
        if (dd < maxt && i > id) id = i;
    } else if (dd < t || (dd == t && i > id)) {
        t = dd;
        id = i;
    }
}

// Visit-order hit mask of wide node nd (wide_visit): bit p = the child in slot p ^ oct.
unsigned visit(const State *S, int nd, const float *o, const Ray &r, float lim, int idmin)
{
    const uint32_t *w = &S->words[(size_t)nd * sptbvh::WIDE_WORDS];
    const uint32_t *hid = &S->maxid[(size_t)nd * sptbvh::WIDE];
    const float c[3] = {f32(w[0]) - o[0], f32(w[1]) - o[1], f32(w[2]) - o[2]};
    const float dist = sqrtf(fmaf(c[0], c[0], fmaf(c[1], c[1], c[2] * c[2])));
    const float m = fmaf(r.alpha, dist + f32(w[4]), f32(w[5]));
    float a[3], bn[3], bf[3];
    for (int k = 0; k < 3; k++) {
        const float sc = f32(((w[3] >> (8 * k)) & 255u) << 23);
        a[k] = sc * r.inv[k];
        const float b = c[k] * r.inv[k], mk = m * fabsf(r.inv[k]);
        bn[k] = b - mk;
        bf[k] = b + mk;
    }
    unsigned hm = 0;
    for (int s = 0; s < 8; s++) {
        if (!((w[3] >> (24 + s)) & 1u)) continue;
        if (idmin >= 0 && (int)hid[s] <= idmin) continue;
        float tn = 0.f, tf = lim;
        for (int k = 0; k < 3; k++) {
            const bool neg = (r.oct >> k) & 1;
            const uint32_t lo = (w[16 + 6 * (s >> 2) + k] >> (8 * (s & 3))) & 255u;
            const uint32_t hi = (w[16 + 6 * (s >> 2) + 3 + k] >> (8 * (s & 3))) & 255u;
            tn = std::max(tn, fmaf((float)(neg ? hi : lo), a[k], bn[k]));
            tf = std::min(tf, fmaf((float)(neg ? lo : hi), a[k], bf[k]));
        }
        if (tn <= tf) hm |= 1u << (s ^ r.oct);
    }
    return hm;
}

// The 8-wide walk (counted form: a shadow query returns the highest occluder).
bool walk_wide(const State *S, const float *o, const float *d, bool shadow, float maxt, float &t_out, int &id_out)
{
    float t = shadow ? maxt : 1e20f;
    int id = -1;
    for (int j = S->nb; j < S->nb + S->na; j++) take(S, j, o, d, shadow, maxt, t, id);
    const Ray r = walk_ray(d);
    std::vector<uint32_t> stack;
    int cur = 0;
    unsigned m = visit(S, 0, o, r, shadow ? maxt : t, shadow ? id : -1);
    while (true) {
        while (m == 0 && !stack.empty()) {
            cur = (int)(stack.back() >> 8);
            m = stack.back() & 255u;
            stack.pop_back();
        }
        if (m == 0) break;
        const int pbit = __builtin_ctz(m);
        m &= ~(1u << pbit);
        const int32_t cw = (int32_t)S->words[(size_t)cur * sptbvh::WIDE_WORDS + 8 + (pbit ^ r.oct)];
        if (cw < 0) {
            const int f = (~cw) & 0xffffff, c = (~cw) >> 24;
            for (int q = 0; q < c; q++) take(S, f + q, o, d, shadow, maxt, t, id);
        } else {
            const unsigned hm = visit(S, cw, o, r, shadow ? maxt : t, shadow ? id : -1);
            if (hm) {
                if (m) stack.push_back(((uint32_t)cur << 8) | m);
                if ((int)stack.size() > S->wdepth - 1) return false;     // stack bound violated
                cur = cw;
                m = hm;
            }
        }
    }
    t_out = t;
    id_out = id;
    return true;
}

// The binary walk over the ray's octant layout (bvh_walk: near child first, escape links).
bool walk_binary(const State *S, const float *o, const float *d, bool shadow, float maxt, float &t_out, int &id_out)
{
    float t = shadow ? maxt : 1e20f;
    int id = -1;
    for (int j = S->nb; j < S->nb + S->na; j++) take(S, j, o, d, shadow, maxt, t, id);
    const Ray r = walk_ray(d);
    const float *lay = &S->nodes[8 * (size_t)S->nn * r.oct];
    int node = 0, steps = 0;
    while (node < S->nn) {
        if (node < 0 || ++steps > 2 * S->nn) return false;               // a broken link
        const float *a = lay + 8 * (size_t)node, *b = a + 4;
        int link;
        memcpy(&link, &a[3], 4);
        const float lim = shadow ? maxt : t;
        const float c[3] = {a[0] - o[0], a[1] - o[1], a[2] - o[2]};
        const float dist = sqrtf(fmaf(c[0], c[0], fmaf(c[1], c[1], c[2] * c[2])));
        const float m = fmaf(r.alpha, dist, b[3]);
        float lo3[3], hi3[3];
        for (int k = 0; k < 3; k++) {
            const float tc = c[k] * r.inv[k], h = (b[k] + m) * fabsf(r.inv[k]);
            lo3[k] = tc - h;
            hi3[k] = tc + h;
        }
        // folded as the device folds them (three NaN slabs give a NaN, which fails the test below)
        const float tn = fmaxf(fmaxf(lo3[0], lo3[1]), lo3[2]), tf = fminf(fminf(hi3[0], hi3[1]), hi3[2]);
        const bool cross = tn <= tf && tf >= 0.f && tn <= lim;
        if (link < 0) {
            if (cross) {
                const int f = (~link) & 0xffffff, cnt = (~link) >> 24;
                for (int q = 0; q < cnt; q++) take(S, f + q, o, d, shadow, maxt, t, id);
            }
            node++;
        } else {
            node = cross ? node + 1 : link;
        }
    }
    t_out = t;
    id_out = id;
    return true;
}

// Mismatches of the walks (the 8-wide one where the scene has a wide tree, and
// the binary one) against the full scan over nrays rays (o.xyz, d.xyz); maxt:
// shadow queries (null: nearest hit).  t_scan / id_scan (optional) receive the
// full scan's results.  Rays are independent: up to eight threads share them.
long long walk_check(const State *S, const float *rays, const float *maxt, long long nrays, float *t_scan,
                     int *id_scan)
{
    if (S->nn == 0) return -1;
    const int nt = (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<long long> bad(nt, 0);
    auto part = [&](int th) {
        for (long long k = th; k < nrays; k += nt) {
            const float *o = rays + 6 * k, *d = o + 3;
            const bool shadow = maxt != nullptr;
            // Intersect (nearest, ties to the highest index) or IntersectP (the
            // highest index below maxt, as counted)
            float t = shadow ? maxt[k] : 1e20f;
            int id = -1;
            for (int i = S->n - 1; i >= 0; i--) {
                const float dd = sphere_hit(S->sp[i], o, d);
                if (shadow) {
                    if (dd < maxt[k] && id < 0) id = i;
                } else if (dd < t) {
                    t = dd;
                    id = i;
                }
            }
            if (t_scan) t_scan[k] = t;
            if (id_scan) id_scan[k] = id;
            for (int which = S->wn ? 0 : 1; which < 2; which++) {
                float tw = 0.f;
                int iw = -2;
                const bool ok = which == 0 ? walk_wide(S, o, d, shadow, shadow ? maxt[k] : 0.f, tw, iw)
                                           : walk_binary(S, o, d, shadow, shadow ? maxt[k] : 0.f, tw, iw);
                if (!ok || iw != id || (!shadow && memcmp(&tw, &t, 4))) bad[th]++;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int th = 1; th < nt; th++) pool.emplace_back(part, th);
    part(0);
    for (std::thread &th : pool) th.join();
    long long total = 0;
    for (long long v : bad) total += v;
    return total;
}

}  // namespace

extern "C" {

void *rfc_create(const rt_sphere *sp, int n, int wide) { return create(sp, n, wide); }
void rfc_destroy(void *s) { delete (State *)s; }

// out[0..4]: bytes of the five sections; then binary nodes, tree entries,
// always entries, wide nodes, wide depth, leaf size, bytes of refit metadata
// (the topology's ints, the entry boxes and the canonical boxes).
void rfc_sizes(const void *s, long long *out)
{
    const State *S = (const State *)s;
    out[0] = 4 * (long long)S->nodes.size();
    out[1] = 4 * (long long)S->geo.size();
    out[2] = 4 * (long long)S->ids.size();
    out[3] = 4 * (long long)S->words.size();
    out[4] = 4 * (long long)S->maxid.size();
    out[5] = S->nn; out[6] = S->nb; out[7] = S->na; out[8] = S->wn; out[9] = S->wdepth; out[10] = S->leaf_max;
    out[11] = 4 * (long long)S->meta.ints() + 4 * 6 * (long long)S->nb + 4 * 8 * (long long)S->nn;
}

void rfc_sections(const void *s, void *out)
{
    const State *S = (const State *)s;
    char *p = (char *)out;
    memcpy(p, S->nodes.data(), 4 * S->nodes.size()); p += 4 * S->nodes.size();
    memcpy(p, S->geo.data(), 4 * S->geo.size()); p += 4 * S->geo.size();
    memcpy(p, S->ids.data(), 4 * S->ids.size()); p += 4 * S->ids.size();
    memcpy(p, S->words.data(), 4 * S->words.size()); p += 4 * S->words.size();
    memcpy(p, S->maxid.data(), 4 * S->maxid.size());
}

void rfc_refit(void *s, const rt_sphere *sp) { refit((State *)s, sp); }
long long rfc_check(const void *s, char *msg, int cap) { return check((const State *)s, msg, cap); }
long long rfc_walk(const void *s, const float *rays, const float *maxt, long long nrays, float *t_scan, int *id_scan)
{
    return walk_check((const State *)s, rays, maxt, nrays, t_scan, id_scan);
}

}  // extern "C"

#ifdef SPT_REFIT_MAIN
// Stand-alone run: two scenes of its own (a small and a larger cloud over a
// ground sphere), the five kinds of edit of tests/test_refit.py, each followed
// by the containment check and both walks; then the degenerate kinds of
// tests/scenes_layouts.py (negative, zero and non-finite radii and centres):
// a tree built from each, a tree refitted to each and back, both walks.
namespace {
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double uni()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}
std::vector<rt_sphere> scene(int n, float half)
{
    std::vector<rt_sphere> v(n);
    for (int i = 0; i < n; i++) {
        rt_sphere &q = v[i];
        memset(&q, 0, sizeof(q));
        q.rad = (float)pow(10.0, -2.5 + 2.0 * uni());
        q.p.x = (float)((2 * uni() - 1) * half);
        q.p.y = (float)((2 * uni() - 1) * half);
        q.p.z = (float)((2 * uni() - 1) * half);
        q.c.x = q.c.y = q.c.z = 0.5f;
        q.refl = i % 3;
    }
    v[0].rad = 1e4f; v[0].p.x = 0.f; v[0].p.y = -1e4f - half - 2.f; v[0].p.z = 0.f;
    v[1].rad = 3.f; v[1].e.x = v[1].e.y = v[1].e.z = 20.f;
    return v;
}
int run(int n, float half)
{
    const std::vector<rt_sphere> base = scene(n, half);
    int rc = 0;
    for (int edit = 0; edit <= 5; edit++) {
        State *S = create(base.data(), n, 1);
        if (!S) return 1;
        std::vector<rt_sphere> v = base;
        if (edit == 1)
            for (int i = 0; i < n; i += 10) {
                v[i].p.x += (float)((2 * uni() - 1) * half);
                v[i].p.z += (float)((2 * uni() - 1) * half);
                v[i].rad *= (float)pow(2.0, 2 * uni() - 1);
            }
        if (edit == 2) v[n / 2].p.x += 2e3f * half;
        if (edit == 3) for (rt_sphere &q : v) q.rad *= 0x1p-6f;
        if (edit == 4) { v[n / 3].rad = 200.f; v[0].rad = 0.05f; }
        if (edit == 5)
            for (int j = 0; j < S->nb; j++) { rt_sphere &q = v[S->ids[j]]; q.p.x = 1.f; q.p.y = 2.f; q.p.z = 3.f; q.rad = 0.25f; }
        refit(S, v.data());
        char msg[256] = "";
        const long long bad = check(S, msg, sizeof(msg));
        std::vector<float> rays, maxt;
        for (int k = 0; k < 400; k++) {
            float d[3] = {(float)(2 * uni() - 1), (float)(2 * uni() - 1), (float)(2 * uni() - 1)};
            const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-9f;
            for (int a = 0; a < 3; a++) rays.push_back((float)((2 * uni() - 1) * half));
            for (int a = 0; a < 3; a++) rays.push_back(d[a] / l);
            maxt.push_back((float)(uni() * 2 * half));
        }
        const long long wrong = walk_check(S, rays.data(), nullptr, 400, nullptr, nullptr) +
                                walk_check(S, rays.data(), maxt.data(), 400, nullptr, nullptr);
        printf("n %d edit %d: nodes %d wide %d violations %lld %s walk mismatches %lld\n", n, edit, S->nn, S->wn, bad,
               msg, wrong);
        if (bad || wrong) rc = 1;
        delete S;
    }
    return rc;
}

// Kind k on every seventh sphere from 20 on (k == 10: every sphere from 4 on
// with a negated radius; 11: with a NaN centre; 12: kinds 0..9 in turn).
void degenerate(std::vector<rt_sphere> &v, int kind)
{
    const int n = (int)v.size();
    auto one = [&](rt_sphere &q, int k, int j) {
        float *c = j % 3 == 0 ? &q.p.x : (j % 3 == 1 ? &q.p.y : &q.p.z);
        switch (k) {
        case 0: q.rad *= -4.f; break;
        case 1: q.rad = 0.f; break;
        case 2: q.rad = 1e-40f; break;
        case 3: q.rad = INFINITY; break;
        case 4: q.rad = -INFINITY; break;
        case 5: q.rad = NAN; break;
        case 6: *c = NAN; break;
        case 7: *c = j % 2 ? -INFINITY : INFINITY; break;
        case 8: *c = j % 4 < 2 ? 3.4e38f : -3.4e38f; break;
        case 9: *c = 3.4e38f; q.rad = 1e36f; break;
        }
    };
    if (kind == 10) { for (int i = 4; i < n; i++) v[i].rad = -v[i].rad; return; }
    if (kind == 11) { for (int i = 4; i < n; i++) v[i].p.x = v[i].p.y = v[i].p.z = NAN; return; }
    int j = 0;
    for (int i = 20; i < n; i += 7, j++) one(v[i], kind == 12 ? j % 10 : kind, j);
}

bool same_sections(const State *A, const State *B)
{
    auto eq = [](const auto &a, const auto &b) { return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * sizeof(a[0])); };
    return eq(A->nodes, B->nodes) && eq(A->geo, B->geo) && eq(A->ids, B->ids) && eq(A->words, B->words) && eq(A->maxid, B->maxid);
}

int run_degenerate(int n, float half, int nrays)
{
    const std::vector<rt_sphere> base = scene(n, half);
    State *fresh = create(base.data(), n, 1);
    if (!fresh) return 1;
    std::vector<float> rays, maxt;
    for (int k = 0; k < nrays; k++) {
        float d[3] = {(float)(2 * uni() - 1), (float)(2 * uni() - 1), (float)(2 * uni() - 1)};
        const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-9f;
        for (int a = 0; a < 3; a++) rays.push_back((float)((2 * uni() - 1) * half));
        for (int a = 0; a < 3; a++) rays.push_back(d[a] / l);
        maxt.push_back((float)(uni() * 2 * half));
    }
    int rc = 0;
    for (int kind = 0; kind <= 12; kind++) {
        std::vector<rt_sphere> v = base;
        degenerate(v, kind);
        State *built = create(v.data(), n, 1), *S = create(base.data(), n, 1);
        if (!built || !S) return 1;
        char msg[256] = "";
        long long bad = check(built, msg, sizeof(msg));
        long long wrong = walk_check(built, rays.data(), nullptr, nrays, nullptr, nullptr) +
                          walk_check(built, rays.data(), maxt.data(), nrays, nullptr, nullptr);
        refit(S, v.data());
        bad += check(S, msg, sizeof(msg));
        wrong += walk_check(S, rays.data(), nullptr, nrays, nullptr, nullptr) +
                 walk_check(S, rays.data(), maxt.data(), nrays, nullptr, nullptr);
        refit(S, base.data());
        const bool back = same_sections(S, fresh);
        printf("n %d degenerate kind %d: violations %lld %s walk mismatches %lld refit back %s\n", n, kind, bad, msg, wrong,
               back ? "equal" : "DIFFERS");
        if (bad || wrong || !back) rc = 1;
        delete built;
        delete S;
    }
    delete fresh;
    return rc;
}
}  // namespace

int main()
{
    const int a = run(300, 5.f), b = run(3000, 30.f);
    const int c = run_degenerate(300, 5.f, 2000), d = run_degenerate(3000, 30.f, 500);
    return a | b | c | d;
}
#endif
