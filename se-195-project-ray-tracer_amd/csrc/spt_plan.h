// spt_plan.h -- the sample plan (spt_frame_plan_async): from a frame's colours,
// second moments (spt_scene_render_pixels_stats_async) and sample counts to
// the next call's pixel list, on the device and in stream order, so that a
// refinement loop is (plan, render) enqueued back to back with no host round
// trip.  No scene is involved.
// Two parts, as in spt_pixels.h.  The index arithmetic and the integer part of
// the decision below are plain integer code (SPT_HD, no HIP types):
// tests/native/plan_index_check.cpp includes this header under g++ and sweeps
// them.  The kernels (under __HIPCC__) are not stand-alone: smallpt.hip
// includes this header inside namespace rt::smallpt.
#ifndef SPT_PLAN_H
#define SPT_PLAN_H

#include <stdint.h>
#include "spt_policy.h"     // SPT_HD (smallpt.hip has it in already)

// ---------------------------------------------------------------------------
// Tiles, lanes, pixels.  The frame is cut into 8 x 8 tiles, row by row; one
// wave takes one tile, lane l its pixel (l >> 3, l & 7) (row, column), so the
// order budget_list(order="tile") sorts by -- key ((y >> 3) * tiles_x +
// (x >> 3)) * 64 + (y & 7) * 8 + (x & 7) -- is tile * 64 + lane: a listed
// pixel's rank is the listed pixels of the tiles before its own (a prefix sum
// over per-tile counts) plus the listed lanes below it (ballot, mbcnt).
// Coordinates are unsigned: a lane of the last tile column lies up to 6 past
// w, which need not fit an int when w is near INT32_MAX.
// ---------------------------------------------------------------------------
constexpr int PLAN_WPB = 4;                 // waves (tiles) per block of the count and scatter kernels
constexpr int PLAN_SCAN_THREADS = 1024;     // the scan block
constexpr int PLAN_SCAN_ITEMS = 4;          // consecutive tiles per thread
constexpr int PLAN_SCAN_TRIP = PLAN_SCAN_THREADS * PLAN_SCAN_ITEMS;     // tiles per trip of the block

SPT_HD constexpr int plan_tiles_x(int w) { return (int)(((unsigned)w + 7u) >> 3); }
SPT_HD constexpr int plan_tiles_y(int h) { return (int)(((unsigned)h + 7u) >> 3); }
// (at most w * h, since ceil(w / 8) <= w: an int where w * h is one)
SPT_HD constexpr int plan_tiles(int w, int h) { return plan_tiles_x(w) * plan_tiles_y(h); }
SPT_HD constexpr unsigned plan_x(int tile, int lane, int w) { return (unsigned)(tile % plan_tiles_x(w)) * 8u + (unsigned)(lane & 7); }
SPT_HD constexpr unsigned plan_y(int tile, int lane, int w) { return (unsigned)(tile / plan_tiles_x(w)) * 8u + (unsigned)(lane >> 3); }
// A lane past the frame's right or bottom edge has no pixel and is never listed.
SPT_HD constexpr bool plan_inside(unsigned x, unsigned y, int w, int h) { return x < (unsigned)w && y < (unsigned)h; }
// (inside only) the index d_list and d_pixels use, and the slot of colours, m2, done and error
SPT_HD constexpr int plan_pixel(unsigned x, unsigned y, int w) { return (int)(y * (unsigned)w + x); }
SPT_HD constexpr int plan_slot(unsigned x, unsigned y, int w, int h) { return (int)(((unsigned)h - y - 1u) * (unsigned)w + x); }
SPT_HD constexpr long long plan_key(int tile, int lane) { return (long long)tile * 64 + lane; }

// The decision's integer part.  Below min_samples a pixel is brought up to it
// (a count that is not one -- negative -- saturates instead of overflowing);
// from there on it takes `step` more while its error is above the tolerance,
// never past max_samples.
SPT_HD constexpr int plan_take_bootstrap(int n, int min_samples)
{
    const long long t = (long long)min_samples - n;
    return t > 0x7fffffffll ? 0x7fffffff : (int)t;
}
SPT_HD constexpr int plan_take_step(int n, bool above, int step, int max_samples)
{
    return above && n < max_samples ? (step < max_samples - n ? step : max_samples - n) : 0;
}

// d_scratch: two 64-bit words (the listed count, spare), a 64-bit take sum per
// tile, then a 32-bit count per tile that the scan turns into the tile's
// offset in place.
SPT_HD constexpr size_t plan_scratch_bytes(int ntiles) { return (16 + (size_t)ntiles * 12 + 15) & ~(size_t)15; }
inline unsigned long long *plan_scratch_head(void *scratch) { return (unsigned long long *)scratch; }
inline unsigned long long *plan_scratch_sums(void *scratch) { return (unsigned long long *)scratch + 2; }
inline unsigned *plan_scratch_counts(void *scratch, int ntiles) { return (unsigned *)(plan_scratch_sums(scratch) + ntiles); }

#ifdef __HIPCC__
// ---------------------------------------------------------------------------
// The kernels.  Three launches in stream order and nothing else orders them:
// no block waits for another, no flag, no atomic.
//   plan_count_kernel    a wave per tile: the decision per lane, d_error, the
//                        tile's listed count and take sum
//   plan_scan_kernel     one block: the exclusive prefix sum of the counts, in
//                        place, PLAN_SCAN_TRIP tiles a trip (PLAN_SCAN_ITEMS
//                        consecutive ones per thread) with a running carry;
//                        the totals
//   plan_scatter_kernel  a wave per tile again: the same decision from the
//                        same inputs, the listed lanes to offset + rank; then
//                        every thread pads [listed, cap) grid-stride
// plan_decide is the one statement of the decision; both passes call it, so
// the counts and the scatter cannot disagree.
// The block shapes are template parameters (the host passes PLAN_WPB and
// PLAN_SCAN_ITEMS): as templates the three kernels are emitted behind every
// other kernel of smallpt.hip's code object, which keeps the renderer's
// kernels at the addresses they had (a plain kernel defined here goes in front
// of them and moves them all; the flagship frame then measured 0.15 % slower).
// ---------------------------------------------------------------------------
struct PlanArgs {
    const float *colors;          // 3 floats per slot
    const float *m2;              // 1 float per slot
    const int32_t *done;          // 1 count per slot
    int w, h, ntiles;
    spt_plan_params p;
    int32_t *list, *take;         // cap entries each (cap == 0: not touched)
    int cap;
    float *error;                 // null, or 1 float per slot
    uint64_t *totals;             // null, or 2 words
    unsigned long long *head, *sums;    // d_scratch's parts (above)
    unsigned *counts;
};

struct PlanPick {
    int take;
    float e;
};

// Every lane calls it (sqrt_exact votes); a lane without a pixel passes
// n = min_samples and zeros and drops the result.
__device__ __forceinline__ PlanPick plan_decide(const spt_plan_params &p, int n, float cx, float cy, float cz, float m2)
{
    const float mean2 = (cx * cx + cy * cy) + cz * cz;
    float var = m2 - mean2;
    var = var > 0.f ? var : 0.f;                                // (a NaN too)
    const float e = sqrt_exact(var / ((float)n * (mean2 + p.floor)));
    if (n < p.min_samples) return PlanPick{plan_take_bootstrap(n, p.min_samples), __builtin_inff()};
    return PlanPick{plan_take_step(n, e > p.tol, p.step, p.max_samples), e};    // (a NaN e is not above)
}

// The wave's tile, the lane's pixel and its decision: what both passes share.
struct PlanLane {
    bool inside;
    int pixel, slot;
    PlanPick pick;
};

__device__ __forceinline__ PlanLane plan_lane(const PlanArgs &a, int tile, int lane)
{
    PlanLane L;
    const unsigned x = plan_x(tile, lane, a.w), y = plan_y(tile, lane, a.w);
    L.inside = plan_inside(x, y, a.w, a.h);
    L.pixel = L.inside ? plan_pixel(x, y, a.w) : 0;
    L.slot = L.inside ? plan_slot(x, y, a.w, a.h) : 0;
    int n = a.p.min_samples;
    float cx = 0.f, cy = 0.f, cz = 0.f, m2 = 0.f;
    if (L.inside) {
        n = a.done[L.slot];
        cx = a.colors[3 * (size_t)L.slot];
        cy = a.colors[3 * (size_t)L.slot + 1];
        cz = a.colors[3 * (size_t)L.slot + 2];
        m2 = a.m2[L.slot];
    }
    L.pick = plan_decide(a.p, n, cx, cy, cz, m2);
    if (!L.inside) L.pick.take = 0;
    return L;
}

template <int WPB>
__global__ void __launch_bounds__(64 * WPB) plan_count_kernel(PlanArgs a)
{
    const int lane = (int)(threadIdx.x & 63);
    const long long t = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (t >= a.ntiles) return;                                  // (the whole wave)
    const int tile = (int)t;
    const PlanLane L = plan_lane(a, tile, lane);
    if (L.inside && a.error) a.error[L.slot] = L.pick.e;
    const unsigned long long listed = __builtin_amdgcn_ballot_w64(L.pick.take > 0);
    unsigned long long sum = L.pick.take > 0 ? (unsigned long long)L.pick.take : 0ull;
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) {
        a.counts[tile] = (unsigned)__builtin_popcountll(listed);
        a.sums[tile] = sum;
    }
}

template <int ITEMS>
__global__ void __launch_bounds__(PLAN_SCAN_THREADS) plan_scan_kernel(PlanArgs a)
{
    constexpr int NW = PLAN_SCAN_THREADS / 64;
    __shared__ unsigned wtot[NW];
    __shared__ unsigned long long wsum[NW];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned carry = 0;                                         // the listed pixels of the trips before (<= w * h)
    unsigned long long sum = 0;
    for (long long base = 0; base < a.ntiles; base += (PLAN_SCAN_THREADS * ITEMS)) {
        const long long i0 = base + (long long)tid * ITEMS;
        unsigned c[ITEMS], mine = 0;
#pragma unroll
        for (int j = 0; j < ITEMS; j++) {
            const bool in = i0 + j < a.ntiles;
            c[j] = in ? a.counts[i0 + j] : 0u;
            if (in) sum += a.sums[i0 + j];
            mine += c[j];
        }
        unsigned incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned v = __shfl_up(incl, d, 64);
            if (lane >= d) incl += v;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        unsigned before = 0, total = 0;
        for (int j = 0; j < NW; j++) {
            const unsigned v = wtot[j];
            before += j < wave ? v : 0u;
            total += v;
        }
        unsigned off = carry + before + (incl - mine);
#pragma unroll
        for (int j = 0; j < ITEMS; j++) {
            if (i0 + j < a.ntiles) a.counts[i0 + j] = off;
            off += c[j];
        }
        carry += total;
        __syncthreads();
    }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long takes = 0;
        for (int j = 0; j < NW; j++) takes += wsum[j];
        a.head[0] = carry;
        a.head[1] = takes;
        if (a.totals) {
            a.totals[0] = carry;
            a.totals[1] = takes;
        }
    }
}

template <int WPB>
__global__ void __launch_bounds__(64 * WPB) plan_scatter_kernel(PlanArgs a)
{
    const int lane = (int)(threadIdx.x & 63);
    const long long t = (long long)blockIdx.x * WPB + (threadIdx.x >> 6);
    if (t < a.ntiles) {                                         // (the whole wave)
        const int tile = (int)t;
        const PlanLane L = plan_lane(a, tile, lane);
        const bool want = L.pick.take > 0;
        const unsigned long long listed = __builtin_amdgcn_ballot_w64(want);
        const unsigned rank = __builtin_amdgcn_mbcnt_hi((unsigned)(listed >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)listed, 0u));
        const unsigned pos = a.counts[tile] + rank;             // (<= w * h)
        if (want && pos < (unsigned)a.cap) {
            a.list[pos] = L.pixel;
            a.take[pos] = L.pick.take;
        }
    }
    // the padding: every position from the number written up to cap
    const unsigned long long total = a.head[0];
    const long long first = total < (unsigned long long)a.cap ? (long long)total : (long long)a.cap;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long j = first + (long long)blockIdx.x * blockDim.x + threadIdx.x; j < a.cap; j += stride) {
        a.list[j] = -1;
        a.take[j] = 0;
    }
}
#endif  // __HIPCC__

#endif  // SPT_PLAN_H
