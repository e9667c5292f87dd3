// spt_sched.h -- host state a prepared smallpt scene keeps between launches:
// the adaptive dispatch order of its tile groups (SptSched) and the ring of
// work counters of its persistent launches (WorkRing).  Host code over the
// HIP runtime; smallpt.hip's spt_scene holds both and scene_render drives them.
#ifndef SPT_SCHED_H
#define SPT_SCHED_H

#include <string.h>
#include <algorithm>
#include <mutex>
#include <vector>
#include "rt_runtime.h"
#include "spt_policy.h"

namespace sptsched {

// Adaptive dispatch order of a scene's tile groups (scene_render): the first
// launch for a given window / camera / sample count records each group's
// wave time; once that is back on the host, later launches of the same key
// dispatch the groups heaviest first, so the long tiles of a non-uniform
// scene (configs[4]: per-wave work varies 6x) start at once instead of
// setting the frame's tail.  Scheduling only: every pixel's computation is
// unchanged.
struct SchedKey {
    int w = 0, h = 0, r0 = 0, r1 = 0, gstride = 0, ns = -1, mode = -1, nslots = 0;
    rt_camera cam = {};
    bool operator==(const SchedKey &o) const
    {
        return w == o.w && h == o.h && r0 == o.r0 && r1 == o.r1 && gstride == o.gstride && ns == o.ns &&
               mode == o.mode && nslots == o.nslots && memcmp(&cam, &o.cam, sizeof(cam)) == 0;
    }
};
struct SptSched {
    SchedKey key;
    int state = 0;                    // 0: none, 1: costs recorded (copy in flight), 2: order set
    int cap = 0;
    unsigned *d_cost = nullptr, *h_cost = nullptr;   // h_*: pinned
    int *d_order = nullptr, *h_order = nullptr;
    hipEvent_t ev = nullptr;
    // d_order is never rewritten or freed once a stream capture has used it
    // (the graph holds its address): it is retired instead and freed with
    // the scene, and a fresh buffer takes the next order.
    bool order_captured = false;
    std::vector<int *> retired;
};

// The order for one launch with this key (key.nslots = g.nslots): sets
// g.order / g.cost; returns true if the caller must queue the cost read-back
// (sched_after) after the launch.
inline bool sched_before(SptSched &q, sptpolicy::Shape &g, hipStream_t s, const SchedKey &key)
{
    const char *e = getenv("RT_SPT_SCHED");
    if (e && atoi(e) == 0) return false;
    const int nslots = key.nslots;
    if (!(q.key == key)) {
        q.key = key;
        q.state = 0;
    }
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) {
        if (q.state == 2) {                            // a device pointer, kept alive and unchanged from now on
            g.order = q.d_order;
            q.order_captured = true;
        }
        return false;
    }
    if (nslots > q.cap) {                               // grow (the old buffers may still be read)
        if (q.ev && hipEventSynchronize(q.ev) != hipSuccess) return false;
        if (hipStreamSynchronize(s) != hipSuccess) return false;
        if (q.d_cost) (void)hipFree(q.d_cost);
        if (q.d_order && q.order_captured) q.retired.push_back(q.d_order);
        else if (q.d_order) (void)hipFree(q.d_order);
        q.order_captured = false;
        if (q.h_cost) (void)hipHostFree(q.h_cost);
        if (q.h_order) (void)hipHostFree(q.h_order);
        q.d_cost = q.h_cost = nullptr;
        q.d_order = q.h_order = nullptr;
        q.cap = 0;
        if (hipMalloc(&q.d_cost, sizeof(unsigned) * nslots) != hipSuccess ||
            hipMalloc(&q.d_order, sizeof(int) * nslots) != hipSuccess ||
            hipHostMalloc(&q.h_cost, sizeof(unsigned) * nslots) != hipSuccess ||
            hipHostMalloc(&q.h_order, sizeof(int) * nslots) != hipSuccess)
            return false;                               // plain launches (the frees above are safe)
        if (!q.ev && hipEventCreateWithFlags(&q.ev, hipEventDisableTiming) != hipSuccess) return false;
        q.cap = nslots;
        q.state = 0;
    }
    if (q.state == 1 && hipEventQuery(q.ev) == hipSuccess) {
        // heaviest first; ties (and the groups past the window: no tiles, 0)
        // in slot order
        std::vector<int> idx(nslots);
        for (int i = 0; i < nslots; i++) idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return q.h_cost[a] > q.h_cost[b]; });
        memcpy(q.h_order, idx.data(), sizeof(int) * nslots);
        if (q.order_captured) {                        // a graph reads the old order: keep it, take a new buffer
            int *fresh = nullptr;
            if (hipMalloc(&fresh, sizeof(int) * q.cap) != hipSuccess) return false;
            q.retired.push_back(q.d_order);
            q.d_order = fresh;
            q.order_captured = false;
        }
        if (hipMemcpyAsync(q.d_order, q.h_order, sizeof(int) * nslots, hipMemcpyHostToDevice, s) != hipSuccess)
            return false;
        q.state = 2;
    }
    if (q.state == 2) {
        g.order = q.d_order;
        return false;
    }
    if (q.state == 0) {
        if (hipMemsetAsync(q.d_cost, 0, sizeof(unsigned) * nslots, s) != hipSuccess) return false;
        g.cost = q.d_cost;
        // The order key is a group's longest tile (its slowest pixel chain),
        // not the sum of its four: the heavy-tile treatment (cooperative or
        // routed tiles) goes to the first groups in order, and a group with
        // one very long tile outranks four middling ones (configs[4] N = 4
        // interleaved windows 17.1 -> 16.3 ms; the full frame level).
        g.cost_max = true;
        return true;
    }
    return false;                                       // state 1, read-back in flight: plain launch
}

inline void sched_after(SptSched &q, hipStream_t s)
{
    if (hipMemcpyAsync(q.h_cost, q.d_cost, sizeof(unsigned) * q.key.nslots, hipMemcpyDeviceToHost, s) == hipSuccess &&
        hipEventRecord(q.ev, s) == hipSuccess)
        q.state = 1;
}

// Frees what the order holds (the scene's device is current and idle).
inline void sched_release(SptSched &q)
{
    if (q.d_cost) (void)hipFree(q.d_cost);
    if (q.d_order) (void)hipFree(q.d_order);
    for (int *p : q.retired) (void)hipFree(p);
    if (q.h_cost) (void)hipHostFree(q.h_cost);
    if (q.h_order) (void)hipHostFree(q.h_order);
    if (q.ev) (void)hipEventDestroy(q.ev);
    q = SptSched();
}

// Work counters of the persistent (8-wide hierarchy) launches: a ring,
// one zeroed quad (rest, routed heavy, cooperative, unused) per launch, so
// launches in flight on several streams do not share one.
// An entry a stream capture used is baked into that graph, which may be
// replayed at any time: it is never handed out again (captured).
// spt_scene_release_captures hands those entries out again once the
// caller has destroyed the graphs.  mu guards the ring's host state
// (launches of one scene from several host threads).
struct WorkRing {
    static constexpr int N = 64;
    int *d = nullptr;                 // N quads (device)
    std::mutex mu;
    int next = 0;
    unsigned long long captured = 0;
};

// A zeroed work-counter quad of the ring for one persistent launch on `s`
// (nullptr + rt error: none left).
inline int *work_entry(WorkRing &r, hipStream_t s)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    std::lock_guard<std::mutex> lk(r.mu);
    for (int tries = 0; tries < WorkRing::N; tries++) {
        const int k = r.next++ % WorkRing::N;
        if ((r.captured >> k) & 1ull) continue;
        if (capturing) r.captured |= 1ull << k;
        int *work = r.d + 4 * k;
        if (hipMemsetAsync(work, 0, 4 * sizeof(int), s) != hipSuccess) return nullptr;   // (check_launch reports it)
        return work;
    }
    rtrt::fail(RT_ERR_INVALID, "spt render: every work-counter entry of the scene is held by a captured graph");
    return nullptr;
}

}  // namespace sptsched

#endif
