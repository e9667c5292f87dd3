// spt_regroup.h -- re-dealing a prepared smallpt scene's spheres into the
// frozen shape of its hierarchy (spt_scene_regroup_async).  A refit
// (spt_refit.h) keeps which sphere sits at which hierarchy position; after the
// spheres have moved about, the leaves are stretched and the walks slow down.
// A regroup keeps every node's entry range [lo, hi) and split axis and
// re-sorts the entries into them, then refits.
//
// Why it cannot change a pixel: the skipping rule (spt_walk.h) asks that every
// box contains its spheres and that every margin is the builders' formula on
// that box.  A regroup is a permutation of the tree entries followed by the
// refit of spt_refit.h, whose boxes are taken from the entries as they then
// lie.  The one table that names spheres by position, the 8-wide highest-index
// table the counted any-hit walk reads, is recomputed from the new order.
//
// The definition (host statement and kernels agree on it byte for byte):
// visit the binary nodes top-down; at an inner node with range [lo, hi),
// frozen axis a and left child [lo, mid), stable-sort the entries of [lo, hi)
// ascending by centre_key(centre[a]) of their spheres.  The left child takes
// the lower part (as the builder's std::partition puts the lower bins left).
// Leaves keep the order in which their entries arrive.  No float is compared:
// a NaN centre has a place in the order like any other bit pattern.
//
// Three parts, as in spt_refit.h:
//   1. centre_key, `__host__ __device__` inline;
//   2. Topo (the per-node children and axes, built beside Meta), Plan (what
//      the launches need, built at the first regroup) and regroup_host;
//   3. the kernels (hipcc only).  A sort over a range larger than SUB_DEFAULT
//      entries is a pass of its own per tree level (keys, ranks, copy back);
//      a subtree of at most SUB_DEFAULT entries is sorted level by level in
//      LDS by one block, which reads and writes its own range of ids alone.
//      No launch reads what another workgroup of the same launch wrote.
#ifndef SPT_REGROUP_H
#define SPT_REGROUP_H

#include "spt_refit.h"

namespace sptregroup {

using sptrefit::Meta;

// ---------------------------------------------------------------- arithmetic
// The total-order integer key of a float: ascending keys are ascending floats,
// -0 below +0, negative NaNs below -inf and positive NaNs above +inf, by their
// bits.  (No conversion and no float comparison.)
SPT_RF_HD uint32_t centre_key(float c)
{
    const uint32_t bits = sptrefit::rf_bits(c);
    return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u);
}

SPT_RF_HD float centre_of(const rt_sphere &q, int axis) { return axis == 0 ? q.p.x : (axis == 1 ? q.p.y : q.p.z); }

// ------------------------------------------------------------------ topology
constexpr int SUB_MAX = sptrefit::WAVE_MAX;   // entries of a subtree one block can sort in LDS
constexpr int SUB_DEFAULT = 256;              // ... and the largest it is given (DESIGN.md section 3 has the timings)
constexpr int CHUNK = 256;                    // entries of a larger range one block ranks

// Per binary node, beside Meta (whose uploaded bytes stay as they are): the
// children (-1: a leaf), the split axis, and the node's slot 8 w + s in the
// 8-wide tree (-1: behind no slot).
struct Topo {
    std::vector<int> left, right, axis, wpos;
};

inline void build_topo(const sptbvh::BvhBuild &b, const Meta &m, Topo &t)
{
    const size_t nn = b.nodes.size();
    t.left.resize(nn); t.right.resize(nn); t.axis.resize(nn);
    for (size_t i = 0; i < nn; i++) {
        t.left[i] = b.nodes[i].left;
        t.right[i] = b.nodes[i].right;
        t.axis[i] = b.nodes[i].axis;
    }
    t.wpos.assign(nn, -1);
    for (size_t k = 0; k < m.wslot.size(); k++)
        if (m.wslot[k] >= 0) t.wpos[m.wslot[k]] = (int)k;
}

// What the launches of a regroup need, from Meta and Topo alone (the host
// learns nothing from the device): the subtree roots of the LDS tier and, per
// tree level that holds an inner node of more than sub_max entries, the
// (node, first entry) of every CHUNK of such a node.  sub_max == 0: no LDS
// tier, every level is a pass of its own (the per-level form, for A/B).
struct Plan {
    int levels = 0;                       // levels of the binary tree
    std::vector<int> sub;                 // (root node, levels below and including it that hold inner nodes) pairs
    std::vector<int> desc;                // (node, first entry) pairs, level after level
    std::vector<int> lev_first, lev_count;   // per global level, its pairs in desc
    size_t ints() const { return sub.size() + desc.size(); }
};

inline void build_plan(const Meta &m, const Topo &t, int sub_max, Plan &p)
{
    p = Plan();
    const int nn = m.nn;
    if (!nn) return;
    std::vector<int> depth(nn, 0), inner_h(nn, 0);
    for (int i = 0; i < nn; i++)                       // children have higher indices than their parent
        if (t.left[i] >= 0) depth[t.left[i]] = depth[t.right[i]] = depth[i] + 1;
    for (int i = nn - 1; i >= 0; i--)                  // levels of inner nodes in the subtree of i
        if (t.left[i] >= 0) inner_h[i] = 1 + std::max(inner_h[t.left[i]], inner_h[t.right[i]]);
    for (int i = 0; i < nn; i++) p.levels = std::max(p.levels, depth[i] + 1);
    auto len = [&](int i) { return m.range[2 * i + 1] - m.range[2 * i]; };
    std::vector<int> parent(nn, -1);
    for (int i = 0; i < nn; i++)
        if (t.left[i] >= 0) parent[t.left[i]] = parent[t.right[i]] = i;
    for (int i = 0; i < nn; i++) {
        if (t.left[i] < 0 || len(i) > sub_max) continue;
        if (parent[i] < 0 || len(parent[i]) > sub_max) { p.sub.push_back(i); p.sub.push_back(inner_h[i]); }
    }
    for (int d = 0; d < p.levels; d++) {
        const int first = (int)p.desc.size() / 2;
        for (int i = 0; i < nn; i++) {
            if (depth[i] != d || t.left[i] < 0 || len(i) <= sub_max) continue;
            for (int c = m.range[2 * i]; c < m.range[2 * i + 1]; c += CHUNK) { p.desc.push_back(i); p.desc.push_back(c); }
        }
        const int count = (int)p.desc.size() / 2 - first;
        if (count) { p.lev_first.push_back(first); p.lev_count.push_back(count); }
    }
}

// The 8-wide highest-index table from ids: maxid[8 w + s] = max(ids[lo..hi))
// of the binary node behind the slot (empty slots keep the builder's 0).
inline void maxid_host(const Meta &m, const int *ids, uint32_t *maxid)
{
    for (size_t k = 0; k < m.wslot.size(); k++) {
        const int bn = m.wslot[k];
        if (bn < 0) continue;
        int mx = -1;
        for (int j = m.range[2 * bn]; j < m.range[2 * bn + 1]; j++) mx = std::max(mx, ids[j]);
        maxid[k] = (uint32_t)mx;
    }
}

// The regroup on the host, over host copies of the five sections (see
// refit_host): ids[0 .. nb) is re-dealt by the definition above, maxid
// (null: no wide tree) recomputed from it, and everything else refitted.
inline void regroup_host(const Meta &m, const Topo &t, const rt_sphere *sp, float *nodes, float *geo, int *ids,
                         uint32_t *wwords, uint32_t *maxid, std::vector<float> &nbox)
{
    for (int i = 0; i < m.nn; i++) {                   // parents before children
        if (t.left[i] < 0) continue;
        const int a = t.axis[i];
        std::stable_sort(ids + m.range[2 * i], ids + m.range[2 * i + 1], [&](int x, int y) {
            return centre_key(centre_of(sp[x], a)) < centre_key(centre_of(sp[y], a));
        });
    }
    if (maxid && m.wn) maxid_host(m, ids, maxid);
    sptrefit::refit_host(m, sp, nodes, geo, ids, wwords, nbox);
}

}  // namespace sptregroup

// -------------------------------------------------------------------- kernels
#if defined(__HIPCC__)
namespace sptregroup {

// Device views: the scene's arrays, Meta's and Topo's uploaded ints, scratch.
struct DevRegroup {
    const rt_sphere *spheres;      // AoS, as refit_gather reads it
    int *ids;                      // hierarchy order; [0, nb) is re-dealt
    uint32_t *maxid;               // 8 per wide node (null: no wide tree)
    int nb;
    const int *range, *order;      // Meta's
    const int *left, *right, *axis, *wpos;
    int n_small, n_wave, n_block;
    uint32_t *keys;                // scratch: nb keys of the level being sorted
    int *tmp;                      // scratch: nb ids, the level's result before it is copied back
};

// ---- ranges above SUB_MAX: three launches per tree level over the same
// (node, first entry) pairs, one block per pair.
__global__ void __launch_bounds__(CHUNK) regroup_keys(DevRegroup v, const int2 *__restrict__ desc)
{
    const int2 d = desc[blockIdx.x];
    const int j = d.y + threadIdx.x, hi = v.range[2 * d.x + 1];
    if (j < hi) v.keys[j] = centre_key(centre_of(v.spheres[v.ids[j]], v.axis[d.x]));
}

// The rank of entry j among its node's entries by (key, position): the number
// of entries before it in the stable order.  The node's keys pass through LDS
// a CHUNK at a time; every lane reads the same word of it (a broadcast).
__global__ void __launch_bounds__(CHUNK) regroup_rank(DevRegroup v, const int2 *__restrict__ desc)
{
    __shared__ uint32_t s_key[CHUNK];
    const int2 d = desc[blockIdx.x];
    const int lo = v.range[2 * d.x], hi = v.range[2 * d.x + 1];
    const int tid = threadIdx.x, j = d.y + tid;
    const bool mine = j < hi;
    const uint32_t key = mine ? v.keys[j] : 0u;
    int rank = 0;
    for (int t = lo; t < hi; t += CHUNK) {
        __syncthreads();
        if (t + tid < hi) s_key[tid] = v.keys[t + tid];
        __syncthreads();
        const int cnt = min(CHUNK, hi - t);
        for (int i = 0; i < cnt; i++) {
            const uint32_t k = s_key[i];
            rank += (k < key || (k == key && t + i < j)) ? 1 : 0;
        }
    }
    if (mine) v.tmp[lo + rank] = v.ids[j];             // lo + rank < hi: a permutation of the node's range
}

__global__ void __launch_bounds__(CHUNK) regroup_copy(DevRegroup v, const int2 *__restrict__ desc)
{
    const int2 d = desc[blockIdx.x];
    const int j = d.y + threadIdx.x;
    if (j < v.range[2 * d.x + 1]) v.ids[j] = v.tmp[j];
}

// ---- subtrees of at most SUB_MAX entries: one block each, every level in LDS.
// Position p of the subtree's range holds, per level, the 64-bit word
//   (first entry of the node covering p, relative) << 44 | centre key << 12 | p
// (a position under a leaf: key 0, so it stays where it is).  The words are
// distinct, so the bitonic network sorts them into the one stable order; the
// low 12 bits then say which entry moves to p.  ids is read once and written
// once, and only over the block's own range.
__global__ void __launch_bounds__(256) regroup_subtree(DevRegroup v, const int2 *__restrict__ sub)
{
    constexpr int PER = SUB_MAX / 256;
    __shared__ uint64_t s_key[SUB_MAX];
    __shared__ int s_id[SUB_MAX];
    const int root = sub[blockIdx.x].x, height = sub[blockIdx.x].y;
    const int lo = v.range[2 * root], m = v.range[2 * root + 1] - lo;
    const int tid = threadIdx.x;
    int P = 2;
    while (P < m) P <<= 1;
    int cur[PER];
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int p = tid + 256 * q;
        cur[q] = root;
        if (p < m) s_id[p] = v.ids[lo + p];
    }
    __syncthreads();
    for (int level = 0; level < height; level++) {
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int p = tid + 256 * q;
            if (p >= P) continue;
            uint64_t w = ~0ull;                        // padding: after every entry
            if (p < m) {
                const int nd = cur[q];
                uint32_t k = 0;
                if (v.left[nd] >= 0) k = centre_key(centre_of(v.spheres[s_id[p]], v.axis[nd]));
                w = ((uint64_t)(uint32_t)(v.range[2 * nd] - lo) << 44) | ((uint64_t)k << 12) | (uint32_t)p;
            }
            s_key[p] = w;
        }
        __syncthreads();
        for (int k = 2; k <= P; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int e = tid; e < P / 2; e += 256) {
                    const int i = ((e & ~(j - 1)) << 1) | (e & (j - 1)), l = i | j;
                    const uint64_t a = s_key[i], b = s_key[l];
                    if ((a > b) == ((i & k) == 0)) { s_key[i] = b; s_key[l] = a; }
                }
                __syncthreads();
            }
        int moved[PER];
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int p = tid + 256 * q;
            moved[q] = p < m ? s_id[(int)(s_key[p] & 4095u)] : 0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; q++) {
            const int p = tid + 256 * q;
            if (p >= m) continue;
            s_id[p] = moved[q];
            const int nd = cur[q], r = v.right[nd];
            if (v.left[nd] >= 0) cur[q] = lo + p < v.range[2 * r] ? v.left[nd] : r;
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < PER; q++) {
        const int p = tid + 256 * q;
        if (p < m) v.ids[lo + p] = s_id[p];
    }
}

// ---- the highest-index table: max(ids[lo..hi)) of every binary node behind
// a wide slot, by refit_nodes' lane groups (Meta::order's size classes).
template <int G>
__device__ __forceinline__ int max_range(const int *__restrict__ ids, int lo, int hi, int lane)
{
    int mx = -1;
    for (int j = lo + lane; j < hi; j += G) mx = max(mx, ids[j]);
    constexpr int W = G < 64 ? G : 64;
    for (int s = W / 2; s >= 1; s >>= 1) mx = max(mx, __shfl_xor(mx, s, W));
    return mx;
}

__global__ void __launch_bounds__(256) regroup_maxid(DevRegroup v, int b_small, int b_wave)
{
    __shared__ int part[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b < b_small) {
        const int k = b * 32 + (tid >> 3);
        if (k >= v.n_small) return;                      // (whole 8-lane groups leave together)
        const int node = v.order[k], at = v.wpos[node];
        if (at < 0) return;
        const int mx = max_range<8>(v.ids, v.range[2 * node], v.range[2 * node + 1], tid & 7);
        if ((tid & 7) == 0) v.maxid[at] = (uint32_t)mx;
    } else if (b < b_small + b_wave) {
        const int k = (b - b_small) * 4 + (tid >> 6);
        if (k >= v.n_wave) return;                       // (whole waves)
        const int node = v.order[v.n_small + k], at = v.wpos[node];
        if (at < 0) return;
        const int mx = max_range<64>(v.ids, v.range[2 * node], v.range[2 * node + 1], tid & 63);
        if ((tid & 63) == 0) v.maxid[at] = (uint32_t)mx;
    } else {
        const int node = v.order[v.n_small + v.n_wave + (b - b_small - b_wave)], at = v.wpos[node];
        if (at < 0) return;                              // (the whole block)
        const int mx = max_range<256>(v.ids, v.range[2 * node], v.range[2 * node + 1], tid);
        if ((tid & 63) == 0) part[tid >> 6] = mx;
        __syncthreads();
        if (tid == 0) v.maxid[at] = (uint32_t)max(max(part[0], part[1]), max(part[2], part[3]));
    }
}

}  // namespace sptregroup
#endif  // __HIPCC__

#endif
