// spt_refit.h -- refit of a prepared smallpt scene's hierarchy after its
// spheres changed (spt_scene_update_async): the tree keeps its topology and
// every box, margin and quantised child box is recomputed from the new
// spheres, with the expressions of the builders in spt_bvh.h.
//
// Why a refit cannot change a pixel: culling is exact (spt_walk.h, "Skipping
// rule"), so any tree whose boxes contain their spheres and whose margins are
// those of spt_bvh.h renders the full scan's bits.  A stale order or a stale
// always / tree partition costs speed only.
//
// Three parts:
//   1. the arithmetic, `__host__ __device__` inline (plain inline under g++,
//      no HIP header needed): the device kernels and the CPU check
//      (tests/native/spt_refit_check.cpp) run the same expressions, none of
//      which the compiler may fuse (every product feeds a store, a compare or
//      a conversion, and everything here builds with -ffp-contract=off);
//   2. Meta, the frozen topology (host, built once from a BvhBuild and the
//      wide words), and refit_host, the refit over host copies of the
//      sections -- the statement the device is compared against byte for byte;
//   3. the three kernels (hipcc only).  Order comes from kernel boundaries
//      alone: no launch reads what another workgroup of the same launch wrote.
#ifndef SPT_REFIT_H
#define SPT_REFIT_H

#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "spt_bvh.h"

#if defined(__HIPCC__)
#define SPT_RF_HD __host__ __device__ inline
#else
#define SPT_RF_HD inline
#endif

namespace sptrefit {

// ---------------------------------------------------------------- arithmetic
SPT_RF_HD uint32_t rf_bits(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
#endif
}
SPT_RF_HD float rf_float(uint32_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    memcpy(&f, &u, 4);
    return f;
#endif
}
SPT_RF_HD double rf_double(uint64_t u)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double((long long)u);
#else
    double d;
    memcpy(&d, &u, 8);
    return d;
#endif
}
SPT_RF_HD uint64_t rf_dbits(double d)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint64_t)__double_as_longlong(d);
#else
    uint64_t u;
    memcpy(&u, &d, 8);
    return u;
#endif
}

// std::min / std::max of the builders, made independent of the order of a
// reduction: of two equal values (+0 and -0, the only equal pair with
// different bits) min takes -0 and max +0, whichever comes first.
SPT_RF_HD float rf_min(float a, float b)
{
    if (a == b) return rf_float(rf_bits(a) | rf_bits(b));
    return b < a ? b : a;
}
SPT_RF_HD float rf_max(float a, float b)
{
    if (a == b) return rf_float(rf_bits(a) & rf_bits(b));
    return a < b ? b : a;
}

constexpr float BOX_EMPTY_LO = sptbvh::BOX_EMPTY_LO, BOX_EMPTY_HI = sptbvh::BOX_EMPTY_HI;   // the builders' empty box

// BvhBuild::box: the float box c -+ |rad| of a sphere, or the empty box where
// a component of it is not finite (such a sphere is never hit).  No entry box
// holds an inf or a NaN, so the reductions below see ordered values alone and
// give the same bits in any order.
SPT_RF_HD void sphere_box(float rad, float px, float py, float pz, float *lo, float *hi)
{
    const float r = fabsf(rad);
    lo[0] = px - r; lo[1] = py - r; lo[2] = pz - r;
    hi[0] = px + r; hi[1] = py + r; hi[2] = pz + r;
    bool finite = true;
    for (int k = 0; k < 3; k++) finite = finite && fabsf(lo[k]) <= 3.402823466e+38f && fabsf(hi[k]) <= 3.402823466e+38f;
    if (!finite)
        for (int k = 0; k < 3; k++) { lo[k] = BOX_EMPTY_LO; hi[k] = BOX_EMPTY_HI; }
}

// The margin term ALPHA_R * R + BETA of a node box (spt_bvh.h, BvhBuild::build).
SPT_RF_HD float node_margin(const float *lo, const float *hi)
{
    double d2 = 0, mag = 0;
    for (int k = 0; k < 3; k++) {
        const float e = hi[k] - lo[k];
        const double p = (double)e * e;
        d2 = d2 + p;
        const float al = fabsf(lo[k]), ah = fabsf(hi[k]);
        const double m = (double)(al < ah ? ah : al);
        mag = mag < m ? m : mag;
    }
    const double a = (double)sptbvh::ALPHA_R * 0.5;
    const double r = a * sqrt(d2);
    const double s = r + 1e-3;
    const double t = 1e-5 * mag;
    return (float)(s + t);
}

// The record pair of a node (BvhBuild::emit): centre and half extent.
SPT_RF_HD void node_record(const float *lo, const float *hi, float *c, float *h)
{
    for (int k = 0; k < 3; k++) {
        const float s = lo[k] + hi[k], d = hi[k] - lo[k];
        c[k] = 0.5f * s;
        h[k] = 0.5f * d;
    }
}

// 2^e as a double, -1022 <= e <= 1023.
SPT_RF_HD double pow2(int e) { return rf_double((uint64_t)(e + 1023) << 52); }

// The quantisation exponent of one axis of a wide node (WideBuild::emit): the
// smallest e in [-126, 127] with 255 * 2^e >= ext (127 if none).  The builder
// counts up from -126; 255 * 2^e grows with e, so starting eight below ext's
// own exponent (where 255 * 2^e < 2^(e + 8) <= ext) finds the same e.
SPT_RF_HD int wide_exponent(float lo, float hi)
{
    const double ext = (double)hi - (double)lo;
    int e = -126;
    if (ext > 0) {
        const int e0 = (int)((rf_dbits(ext) >> 52) & 2047) - 1023 - 8;
        if (e0 > e) e = e0 > 127 ? 127 : e0;
    }
    while (e < 127 && 255.0 * pow2(e) < ext) e++;
    return e;
}

// D0, the node diagonal rounded up (WideBuild::emit).
SPT_RF_HD float wide_d0(const float *lo, const float *hi)
{
    double d2 = 0;
    for (int k = 0; k < 3; k++) {
        const double e = (double)hi[k] - lo[k];
        const double p = e * e;
        d2 = d2 + p;
    }
    const double s = sqrt(d2);
    return (float)(s * (1.0 + 1e-6));
}

// One plane of a quantised child box: floor((v - lo) / 2^e) for a low plane,
// ceil for a high one, clamped to [0, 255].
//
// Exactness.  The builder computes this in long double and then steps the
// result outward while lo + q 2^e is on the wrong side of v.  Here d = v - lo
// is formed in double, and TwoSum's error term tells whether that was exact
// (two floats whose exponents lie within 29 binades always are).  If it was,
// d 2^-e is exact too (a power-of-two scaling inside double's range: |d| is
// within [2^-149, 2^129], e within [-126, 127]), floor / ceil are exact, and
// the result is the true floor / ceil: lo + q 2^e <= v holds in exact
// arithmetic, rounding is monotone and v is representable, so the builder's
// outward steps do nothing and both give the same byte.  If d was rounded,
// floor(d 2^-e) can exceed the true floor by one (and ceil fall short by
// one), never more: the result is widened by one quantum, which keeps the box
// conservative; only there can the byte differ from the builder's.
SPT_RF_HD uint32_t quantise(float v, float lo, int e, bool high)
{
    const double a = (double)v, b = (double)lo;
    const double d = a - b;
    const double bb = d - a;
    const double t0 = d - bb, t1 = b + bb;
    const double e0 = a - t0;
    const double err = e0 - t1;                     // (a - b) - d, exactly
    const double x = d * pow2(-e);
    double q = high ? ceil(x) : floor(x);
    if (err != 0) q = high ? q + 1.0 : q - 1.0;
    if (!(q >= 0.0)) q = 0.0;                       // (a NaN too: no conversion of one)
    if (q > 255.0) q = 255.0;
    return (uint32_t)q;
}

// ------------------------------------------------------------------ topology
constexpr int SMALL_MAX = 16;      // entries of a binary node refitted by 8 lanes
constexpr int WAVE_MAX = 4096;     // ... by one wave; anything larger by a block of 256

// What stays fixed across updates, as uploaded (ints):
//   range  [2 nn]  per binary node, its entries [lo, hi) of the hierarchy-
//                  order array (BvhBuild::idx)
//   pos    [8 nn]  pos[8 i + oct]: node i's record index in the node section
//                  (layout oct starts at oct * nn)
//   order  [nn]    the binary nodes sorted into the three size classes
//   wslot  [8 wn]  per wide node and slot, the binary node behind it (-1: empty)
struct Meta {
    int nn = 0, nb = 0, na = 0, wn = 0;
    int n_small = 0, n_wave = 0, n_block = 0;
    std::vector<int> range, pos, order, wslot;
    size_t ints() const { return range.size() + pos.size() + order.size() + wslot.size(); }
};

inline void layout_positions(const sptbvh::BvhBuild &b, int node, int oct, int &next, int base, int *pos)
{
    pos[8 * node + oct] = base + next++;
    const sptbvh::HostNode &h = b.nodes[node];
    if (h.left < 0) return;
    // the child order of BvhBuild::emit
    const sptbvh::HostNode &L = b.nodes[h.left], &R = b.nodes[h.right];
    const bool l_low = L.lo[h.axis] + L.hi[h.axis] <= R.lo[h.axis] + R.hi[h.axis];
    const bool neg = (oct >> h.axis) & 1;
    const int c0 = (l_low != neg) ? h.left : h.right;
    layout_positions(b, c0, oct, next, base, pos);
    layout_positions(b, c0 == h.left ? h.right : h.left, oct, next, base, pos);
}

// Builds the topology from the tree as the builders left it (b's boxes decide
// the octant child order) and the wide words (wn nodes; null: no wide tree).
// Returns false if a wide child's entry range matches no binary node (never,
// for words built from b).
inline bool build_meta(const sptbvh::BvhBuild &b, int nalways, const uint32_t *wwords, int wn, Meta &m)
{
    const int nn = (int)b.nodes.size();
    m = Meta();
    m.nn = nn;
    m.nb = (int)b.idx.size();
    m.na = nalways;
    m.wn = wwords ? wn : 0;
    std::vector<int> lo, hi;
    b.ranges(lo, hi);
    m.range.resize(2 * (size_t)nn);
    for (int i = 0; i < nn; i++) { m.range[2 * i] = lo[i]; m.range[2 * i + 1] = hi[i]; }
    m.pos.assign(8 * (size_t)nn, 0);
    for (int oct = 0; oct < 8 && nn; oct++) {
        int next = 0;
        layout_positions(b, 0, oct, next, oct * nn, m.pos.data());
    }
    for (int cls = 0; cls < 3; cls++)
        for (int i = 0; i < nn; i++) {
            const int len = hi[i] - lo[i];
            const int c = len <= SMALL_MAX ? 0 : (len <= WAVE_MAX ? 1 : 2);
            if (c == cls) m.order.push_back(i);
        }
    for (int i = 0; i < nn; i++) {
        const int len = hi[i] - lo[i];
        (len <= SMALL_MAX ? m.n_small : (len <= WAVE_MAX ? m.n_wave : m.n_block))++;
    }
    if (!m.wn) return true;
    // A wide child is a binary node, and a binary node is known by its range:
    // a child's range is a strict part of its parent's, so no two nodes share
    // one.  A leaf child's word holds its range; a wide child's range is the
    // union of its own children's, known once they are done (children have
    // higher indices than their parent: walk the nodes backwards).
    std::vector<std::pair<std::pair<int, int>, int>> by_range(nn);
    for (int i = 0; i < nn; i++) by_range[i] = {{lo[i], hi[i]}, i};
    std::sort(by_range.begin(), by_range.end());
    auto find = [&](int l, int h) {
        auto it = std::lower_bound(by_range.begin(), by_range.end(), std::make_pair(std::make_pair(l, h), -1));
        return (it != by_range.end() && it->first.first == l && it->first.second == h) ? it->second : -1;
    };
    m.wslot.assign(8 * (size_t)m.wn, -1);
    std::vector<int> wlo(m.wn), whi(m.wn);
    for (int w = m.wn - 1; w >= 0; w--) {
        const uint32_t *ww = wwords + (size_t)w * sptbvh::WIDE_WORDS;
        int l = 1 << 30, h = -1;
        for (int s = 0; s < 8; s++) {
            if (!((ww[3] >> (24 + s)) & 1u)) continue;
            const int32_t cw = (int32_t)ww[8 + s];
            int cl, ch;
            if (cw < 0) {
                cl = (~cw) & 0xffffff;
                ch = cl + (int)((uint32_t)(~cw) >> 24);
            } else {
                if (cw <= w || cw >= m.wn) return false;
                cl = wlo[cw];
                ch = whi[cw];
            }
            const int bn = find(cl, ch);
            if (bn < 0) return false;
            m.wslot[8 * (size_t)w + s] = bn;
            l = std::min(l, cl);
            h = std::max(h, ch);
        }
        wlo[w] = l;
        whi[w] = h;
    }
    return true;
}

// One wide node from its slots' binary boxes (nbox: two float4 per binary
// node, lo.xyz | margin and hi.xyz | 0): words 0..5 and 16..27 of w are
// rewritten, the valid mask recomputed from the slots, the child words kept.
inline void refit_wide_node(const int *slot, const float *nbox, uint32_t *w)
{
    float lo[3] = {BOX_EMPTY_LO, BOX_EMPTY_LO, BOX_EMPTY_LO}, hi[3] = {BOX_EMPTY_HI, BOX_EMPTY_HI, BOX_EMPTY_HI};
    float K = 0.f;
    uint32_t valid = 0;
    for (int s = 0; s < 8; s++) {
        if (slot[s] < 0) continue;
        const float *c = nbox + 8 * (size_t)slot[s];
        valid |= 1u << s;
        for (int k = 0; k < 3; k++) { lo[k] = rf_min(lo[k], c[k]); hi[k] = rf_max(hi[k], c[4 + k]); }
        K = rf_max(K, c[3]);
    }
    int e[3];
    for (int k = 0; k < 3; k++) e[k] = wide_exponent(lo[k], hi[k]);
    w[0] = rf_bits(lo[0]); w[1] = rf_bits(lo[1]); w[2] = rf_bits(lo[2]);
    w[3] = (uint32_t)(e[0] + 127) | ((uint32_t)(e[1] + 127) << 8) | ((uint32_t)(e[2] + 127) << 16) | (valid << 24);
    w[4] = rf_bits(wide_d0(lo, hi));
    w[5] = rf_bits(K);
    for (int a = 16; a < 28; a++) w[a] = 0;
    for (int s = 0; s < 8; s++) {
        uint32_t q[6] = {255, 255, 255, 0, 0, 0};       // an empty slot: inverted
        if (slot[s] >= 0) {
            const float *c = nbox + 8 * (size_t)slot[s];
            for (int k = 0; k < 3; k++) {
                q[k] = quantise(c[k], lo[k], e[k], false);
                q[3 + k] = quantise(c[4 + k], lo[k], e[k], true);
            }
        }
        for (int a = 0; a < 6; a++) w[16 + 6 * (s >> 2) + a] |= q[a] << (8 * (s & 3));
    }
}

// The refit on the host, over host copies of the sections spt_scene_create
// uploads: nodes (two float4 per record, eight layouts), geo (nb tree entries,
// then na always entries), ids, wide words.  Everything else (links, child
// words, ids, maxid) is left as it is.  nbox (8 floats per binary node)
// receives the canonical boxes.
inline void refit_host(const Meta &m, const rt_sphere *sp, float *nodes, float *geo, const int *ids,
                       uint32_t *wwords, std::vector<float> &nbox)
{
    const int nb = m.nb;
    std::vector<float> box(6 * (size_t)nb);
    for (int j = 0; j < nb + m.na; j++) {
        const rt_sphere &q = sp[ids[j]];
        float *g = geo + 4 * (size_t)j;
        g[0] = q.p.x; g[1] = q.p.y; g[2] = q.p.z;
        g[3] = q.rad * q.rad;                            // geomfunc.h:42 product
        if (j < nb) {
            float lo[3], hi[3];
            sphere_box(q.rad, q.p.x, q.p.y, q.p.z, lo, hi);
            for (int k = 0; k < 3; k++) { box[(size_t)k * nb + j] = lo[k]; box[(size_t)(3 + k) * nb + j] = hi[k]; }
        }
    }
    nbox.assign(8 * (size_t)m.nn, 0.f);
    for (int i = 0; i < m.nn; i++) {
        float lo[3] = {BOX_EMPTY_LO, BOX_EMPTY_LO, BOX_EMPTY_LO}, hi[3] = {BOX_EMPTY_HI, BOX_EMPTY_HI, BOX_EMPTY_HI};
        for (int j = m.range[2 * i]; j < m.range[2 * i + 1]; j++)
            for (int k = 0; k < 3; k++) {
                lo[k] = rf_min(lo[k], box[(size_t)k * nb + j]);
                hi[k] = rf_max(hi[k], box[(size_t)(3 + k) * nb + j]);
            }
        const float mg = node_margin(lo, hi);
        float c[3], h[3];
        node_record(lo, hi, c, h);
        for (int oct = 0; oct < 8; oct++) {
            float *r = nodes + 8 * (size_t)m.pos[8 * (size_t)i + oct];
            r[0] = c[0]; r[1] = c[1]; r[2] = c[2];       // r[3]: the link word, kept
            r[4] = h[0]; r[5] = h[1]; r[6] = h[2]; r[7] = mg;
        }
        float *o = &nbox[8 * (size_t)i];
        o[0] = lo[0]; o[1] = lo[1]; o[2] = lo[2]; o[3] = mg;
        o[4] = hi[0]; o[5] = hi[1]; o[6] = hi[2]; o[7] = 0.f;
    }
    for (int w = 0; w < m.wn; w++)
        refit_wide_node(&m.wslot[8 * (size_t)w], nbox.data(), wwords + (size_t)w * sptbvh::WIDE_WORDS);
}

}  // namespace sptrefit

// -------------------------------------------------------------------- kernels
#if defined(__HIPCC__)
namespace sptrefit {

// Device views of a scene's arrays and of the uploaded Meta.
struct DevRefit {
    rt_sphere *spheres;            // AoS, n (the changed range already copied in, earlier on the stream)
    float4 *soa;                   // geo | emi | col (n each) | light records
    int n;
    float4 *nodes, *geo;           // hierarchy sections (null: no hierarchy); geo holds nb + na entries
    const int *ids;
    uint32_t *wwords;              // null: no wide tree
    int nn, nb, na, wn;
    const int *range, *pos, *order, *wslot;
    int n_small, n_wave, n_block;
    float *box;                    // scratch: six planes of nb floats, entry boxes in hierarchy order
    float4 *nbox;                  // scratch: two per binary node (lo | margin, hi | 0)
};

// One lane per changed sphere, per hierarchy entry and per light record.
//   t < count:     sphere first + t -> its SoA triplet;
//   t < nb + na:   entry t, if its sphere lies in [efirst, efirst + ecount)
//                  -> geo (p, rad * rad) and, for a tree entry, its float box;
//   t < nrec:      light record t from sphere lights[t] (nlights == 0: the one
//                  zero record) -- only when the light list is rewritten.
// Every lane reads the AoS array alone, which no lane of this launch writes.
__global__ void __launch_bounds__(256) refit_gather(DevRefit v, int first, int count, int efirst, int ecount,
                                                    const int *__restrict__ lights, int nlights, int nrec)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < count) {
        const int i = first + t;
        const rt_sphere q = v.spheres[i];
        v.soa[i] = make_float4(q.p.x, q.p.y, q.p.z, q.rad * q.rad);
        v.soa[(size_t)v.n + i] = make_float4(q.e.x, q.e.y, q.e.z, __int_as_float(q.refl));
        v.soa[2 * (size_t)v.n + i] = make_float4(q.c.x, q.c.y, q.c.z, q.rad);
    }
    if (v.nodes && t < v.nb + v.na) {
        const int i = v.ids[t];
        if ((unsigned)(i - efirst) < (unsigned)ecount) {
            const rt_sphere q = v.spheres[i];
            v.geo[t] = make_float4(q.p.x, q.p.y, q.p.z, q.rad * q.rad);
            if (t < v.nb) {
                float lo[3], hi[3];
                sphere_box(q.rad, q.p.x, q.p.y, q.p.z, lo, hi);
                for (int k = 0; k < 3; k++) {
                    v.box[(size_t)k * v.nb + t] = lo[k];
                    v.box[(size_t)(3 + k) * v.nb + t] = hi[k];
                }
            }
        }
    }
    if (t < nrec) {
        float4 *gl = v.soa + 3 * (size_t)v.n + 3 * (size_t)t;
        if (nlights == 0) {
            gl[0] = gl[1] = gl[2] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
            const rt_sphere q = v.spheres[lights[t]];
            gl[0] = make_float4(q.p.x, q.p.y, q.p.z, q.rad * q.rad);
            gl[1] = make_float4(q.c.x, q.c.y, q.c.z, q.rad);
            gl[2] = make_float4(q.e.x, q.e.y, q.e.z, __int_as_float(q.refl));
        }
    }
}

// Min / max of the six planes over entries [lo, hi) by a group of G lanes
// (G = 8 or 64, `lane` within the group), then across the group: every lane
// returns the whole box.
template <int G>
__device__ __forceinline__ void reduce_range(const float *__restrict__ box, int nb, int lo, int hi, int lane,
                                             float *blo, float *bhi)
{
    for (int k = 0; k < 3; k++) { blo[k] = BOX_EMPTY_LO; bhi[k] = BOX_EMPTY_HI; }
    for (int j = lo + lane; j < hi; j += G)
        for (int k = 0; k < 3; k++) {
            blo[k] = rf_min(blo[k], box[(size_t)k * nb + j]);
            bhi[k] = rf_max(bhi[k], box[(size_t)(3 + k) * nb + j]);
        }
    constexpr int W = G < 64 ? G : 64;
    for (int m = W / 2; m >= 1; m >>= 1)
        for (int k = 0; k < 3; k++) {
            blo[k] = rf_min(blo[k], __shfl_xor(blo[k], m, W));
            bhi[k] = rf_max(bhi[k], __shfl_xor(bhi[k], m, W));
        }
}

// Lanes 0..7 of a node's group write its record into layouts 0..7; lane 0
// also writes the canonical box.
__device__ __forceinline__ void write_node(const DevRefit &v, int node, int lane, const float *lo, const float *hi)
{
    if (lane >= 8) return;
    const float mg = node_margin(lo, hi);
    float c[3], h[3];
    node_record(lo, hi, c, h);
    float *r = (float *)(v.nodes + 2 * (size_t)v.pos[8 * (size_t)node + lane]);
    r[0] = c[0]; r[1] = c[1]; r[2] = c[2];               // r[3]: the link word, kept
    v.nodes[2 * (size_t)v.pos[8 * (size_t)node + lane] + 1] = make_float4(h[0], h[1], h[2], mg);
    if (lane == 0) {
        v.nbox[2 * (size_t)node] = make_float4(lo[0], lo[1], lo[2], mg);
        v.nbox[2 * (size_t)node + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
}

// One binary node per lane group, the group sized by the node's range (the
// classes of Meta::order, split on the host): blocks [0, b_small) refit 32
// nodes each with 8 lanes a node, blocks [b_small, b_small + b_wave) four
// nodes each with a wave a node, the rest one node each.  A node's box is the
// min / max over its own range of the entry boxes refit_gather wrote: exact in
// any order, and independent of every other node of this launch.
__global__ void __launch_bounds__(256) refit_nodes(DevRefit v, int b_small, int b_wave)
{
    __shared__ float part[4][6];
    const int b = blockIdx.x, tid = threadIdx.x;
    float lo[3], hi[3];
    if (b < b_small) {
        const int k = b * 32 + (tid >> 3);
        if (k >= v.n_small) return;                      // (whole 8-lane groups leave together)
        const int node = v.order[k];
        reduce_range<8>(v.box, v.nb, v.range[2 * node], v.range[2 * node + 1], tid & 7, lo, hi);
        write_node(v, node, tid & 7, lo, hi);
    } else if (b < b_small + b_wave) {
        const int k = (b - b_small) * 4 + (tid >> 6);
        if (k >= v.n_wave) return;                       // (whole waves)
        const int node = v.order[v.n_small + k];
        reduce_range<64>(v.box, v.nb, v.range[2 * node], v.range[2 * node + 1], tid & 63, lo, hi);
        write_node(v, node, tid & 63, lo, hi);
    } else {
        const int node = v.order[v.n_small + v.n_wave + (b - b_small - b_wave)];
        reduce_range<256>(v.box, v.nb, v.range[2 * node], v.range[2 * node + 1], tid, lo, hi);
        if ((tid & 63) == 0)
            for (int k = 0; k < 3; k++) { part[tid >> 6][k] = lo[k]; part[tid >> 6][3 + k] = hi[k]; }
        __syncthreads();
        for (int w = 0; w < 4; w++)
            for (int k = 0; k < 3; k++) {
                lo[k] = rf_min(lo[k], part[w][k]);
                hi[k] = rf_max(hi[k], part[w][3 + k]);
            }
        write_node(v, node, tid, lo, hi);
    }
}

// Eight lanes per wide node, one per slot: the union of the slot boxes by
// cross-lane min / max, then the frame (every lane the same), each lane's six
// bytes, merged into words 16..27 by cross-lane ORs.  Written in place; the
// child words (8..15) and the highest-index table are not touched.
__global__ void __launch_bounds__(256) refit_wide(DevRefit v)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    const int w = t >> 3, s = t & 7;
    if (w >= v.wn) return;                               // (whole 8-lane groups)
    const int bn = v.wslot[t];
    float clo[3] = {BOX_EMPTY_LO, BOX_EMPTY_LO, BOX_EMPTY_LO}, chi[3] = {BOX_EMPTY_HI, BOX_EMPTY_HI, BOX_EMPTY_HI};
    float K = 0.f;
    uint32_t valid = 0;
    if (bn >= 0) {
        const float4 a = v.nbox[2 * (size_t)bn], c = v.nbox[2 * (size_t)bn + 1];
        clo[0] = a.x; clo[1] = a.y; clo[2] = a.z;
        chi[0] = c.x; chi[1] = c.y; chi[2] = c.z;
        K = a.w;
        valid = 1u << s;
    }
    float lo[3], hi[3];
    for (int k = 0; k < 3; k++) { lo[k] = clo[k]; hi[k] = chi[k]; }
    for (int m = 4; m >= 1; m >>= 1) {
        for (int k = 0; k < 3; k++) {
            lo[k] = rf_min(lo[k], __shfl_xor(lo[k], m, 8));
            hi[k] = rf_max(hi[k], __shfl_xor(hi[k], m, 8));
        }
        K = rf_max(K, __shfl_xor(K, m, 8));
        valid |= (uint32_t)__shfl_xor((int)valid, m, 8);
    }
    int e[3];
    for (int k = 0; k < 3; k++) e[k] = wide_exponent(lo[k], hi[k]);
    uint32_t q[6] = {255, 255, 255, 0, 0, 0};
    if (bn >= 0)
        for (int k = 0; k < 3; k++) {
            q[k] = quantise(clo[k], lo[k], e[k], false);
            q[3 + k] = quantise(chi[k], lo[k], e[k], true);
        }
    uint32_t *ww = v.wwords + (size_t)w * sptbvh::WIDE_WORDS;
    for (int a = 0; a < 6; a++) {
        uint32_t x = q[a] << (8 * (s & 3));
        x |= (uint32_t)__shfl_xor((int)x, 1, 8);
        x |= (uint32_t)__shfl_xor((int)x, 2, 8);
        if ((s & 3) == 0) ww[16 + 6 * (s >> 2) + a] = x;
    }
    if (s == 0) {
        ww[0] = rf_bits(lo[0]); ww[1] = rf_bits(lo[1]); ww[2] = rf_bits(lo[2]);
        ww[3] = (uint32_t)(e[0] + 127) | ((uint32_t)(e[1] + 127) << 8) | ((uint32_t)(e[2] + 127) << 16) | (valid << 24);
        ww[4] = rf_bits(wide_d0(lo, hi));
        ww[5] = rf_bits(K);
    }
}

}  // namespace sptrefit
#endif  // __HIPCC__

#endif
