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
#include "spt_streams.h"

namespace sptsched {

// Adaptive dispatch order of a scene's tile groups (scene_render): the first
// launch for a given window / camera / sample count records each group's
// wave time; once that is back on the host, later launches of the same key
// dispatch the groups heaviest first, so the long tiles of a non-uniform
// scene (configs[4]: per-wave work varies 6x) start at once instead of
// setting the frame's tail.  Scheduling only: every pixel's computation is
// unchanged.
// Several streams: launches of the scene may be in flight on several streams
// (issued by one host thread at a time) and dispatch by the one learnt
// order.  Every uncaptured launch that reads an order buffer records its
// stream's reader event after it (spt_streams.h, Readers).  A new order goes
// into the current buffer if no launch on another stream is still reading it
// (event queries), else into the second buffer, and only if both are being
// read does the uploading stream wait (hipStreamWaitEvent) for the current
// one's readers; a reader on another stream than the upload's waits for the
// upload (up_ev).  The pinned h_order is the upload's source until the upload
// has run: it is not rebuilt before up_ev is complete (the launch goes out
// plain and the next one tries again).  The host never blocks and nothing is
// allocated.  d_cost and h_cost are shared without ordering: they feed only
// the order, and any order gives the same bits.
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
    int *h_order = nullptr;
    hipEvent_t ev = nullptr;
    struct OrderBuf {
        int *d = nullptr;
        sptstreams::Readers readers;  // the streams reading d since its last upload
        hipEvent_t rd_ev[sptstreams::Readers::K] = {};
    };
    OrderBuf ord[2];                  // ord[cur] holds the order in use
    int cur = 0;
    hipEvent_t up_ev = nullptr;       // the last upload (into ord[cur])
    bool uploaded = false;
    hipEvent_t rd_pending = nullptr;  // sched_before -> sched_used: the reader event of the launch being issued
    // ord[cur].d is never rewritten or freed once a stream capture has used it
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
            g.order = q.ord[q.cur].d;
            q.order_captured = true;
        }
        return false;
    }
    if (nslots > q.cap) {                               // grow (the old buffers may still be read)
        if (q.ev && hipEventSynchronize(q.ev) != hipSuccess) return false;
        if (hipStreamSynchronize(s) != hipSuccess) return false;
        for (SptSched::OrderBuf &b : q.ord) {              // (readers and uploads on other streams)
            for (int i = 0; i < sptstreams::Readers::K; i++)
                if (((b.readers.live >> i) & 1u) && hipEventSynchronize(b.rd_ev[i]) != hipSuccess) return false;
            b.readers = sptstreams::Readers();
        }
        if (q.uploaded && hipEventSynchronize(q.up_ev) != hipSuccess) return false;
        q.uploaded = false;
        if (q.d_cost) (void)hipFree(q.d_cost);
        if (q.ord[q.cur].d && q.order_captured) q.retired.push_back(q.ord[q.cur].d);
        else if (q.ord[q.cur].d) (void)hipFree(q.ord[q.cur].d);
        if (q.ord[q.cur ^ 1].d) (void)hipFree(q.ord[q.cur ^ 1].d);
        q.order_captured = false;
        if (q.h_cost) (void)hipHostFree(q.h_cost);
        if (q.h_order) (void)hipHostFree(q.h_order);
        q.d_cost = q.h_cost = nullptr;
        q.ord[0].d = q.ord[1].d = q.h_order = nullptr;
        q.cap = 0;
        if (hipMalloc(&q.d_cost, sizeof(unsigned) * nslots) != hipSuccess ||
            hipMalloc(&q.ord[0].d, sizeof(int) * nslots) != hipSuccess ||
            hipMalloc(&q.ord[1].d, sizeof(int) * nslots) != hipSuccess ||
            hipHostMalloc(&q.h_cost, sizeof(unsigned) * nslots) != hipSuccess ||
            hipHostMalloc(&q.h_order, sizeof(int) * nslots) != hipSuccess)
            return false;                               // plain launches (the frees above are safe)
        if (!q.ev && hipEventCreateWithFlags(&q.ev, hipEventDisableTiming) != hipSuccess) return false;
        if (!q.up_ev && hipEventCreateWithFlags(&q.up_ev, hipEventDisableTiming) != hipSuccess) return false;
        for (SptSched::OrderBuf &b : q.ord)
            for (hipEvent_t &e : b.rd_ev)
                if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
        q.cap = nslots;
        q.state = 0;
    }
    // (the last upload still reads h_order until it has run: try again at the next launch)
    if (q.state == 1 && hipEventQuery(q.ev) == hipSuccess && (!q.uploaded || hipEventQuery(q.up_ev) == hipSuccess)) {
        // heaviest first; ties (and the groups past the window: no tiles, 0)
        // in slot order
        std::vector<int> idx(nslots);
        for (int i = 0; i < nslots; i++) idx[i] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return q.h_cost[a] > q.h_cost[b]; });
        memcpy(q.h_order, idx.data(), sizeof(int) * nslots);
        if (q.order_captured) {                        // a graph reads the old order: keep it, take a new buffer
            int *fresh = nullptr;
            if (hipMalloc(&fresh, sizeof(int) * q.cap) != hipSuccess) return false;
            q.retired.push_back(q.ord[q.cur].d);
            q.ord[q.cur].d = fresh;
            q.order_captured = false;
            q.ord[q.cur].readers = sptstreams::Readers();   // (nothing reads the fresh buffer yet)
        }
        // Launches on other streams may still dispatch by the order this
        // replaces: the buffer none of them reads takes the new one.
        unsigned busy[2];
        for (int b = 0; b < 2; b++) {
            busy[b] = sptstreams::write_waits(q.ord[b].readers, s);
            for (int i = 0; i < sptstreams::Readers::K; i++)
                if (((busy[b] >> i) & 1u) && hipEventQuery(q.ord[b].rd_ev[i]) != hipErrorNotReady) busy[b] &= ~(1u << i);
        }
        q.cur = sptstreams::write_target(q.cur, busy[q.cur], busy[q.cur ^ 1]);
        SptSched::OrderBuf &o = q.ord[q.cur];
        for (int i = 0; i < sptstreams::Readers::K; i++)
            if (((busy[q.cur] >> i) & 1u) && hipStreamWaitEvent(s, o.rd_ev[i], 0) != hipSuccess) return false;
        if (hipMemcpyAsync(o.d, q.h_order, sizeof(int) * nslots, hipMemcpyHostToDevice, s) != hipSuccess ||
            hipEventRecord(q.up_ev, s) != hipSuccess)
            return false;
        sptstreams::written(o.readers, s);
        q.uploaded = true;
        q.state = 2;
    }
    if (q.state == 2) {
        SptSched::OrderBuf &o = q.ord[q.cur];
        const sptstreams::ReaderSlot r = sptstreams::reader_slot(o.readers, s);
        if ((r.wait_slot && hipStreamWaitEvent(s, o.rd_ev[r.slot], 0) != hipSuccess) ||
            (r.wait_write && hipStreamWaitEvent(s, q.up_ev, 0) != hipSuccess))
            return false;
        q.rd_pending = o.rd_ev[r.slot];                 // sched_used records it after the launch
        g.order = o.d;
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

// After an uncaptured launch that sched_before gave the learnt order: the
// stream's reader event (the next upload looks at it).
inline void sched_used(SptSched &q, hipStream_t s)
{
    if (q.rd_pending) (void)hipEventRecord(q.rd_pending, s);
    q.rd_pending = nullptr;
}

// Frees what the order holds (the scene's device is current and idle).
inline void sched_release(SptSched &q)
{
    if (q.d_cost) (void)hipFree(q.d_cost);
    for (SptSched::OrderBuf &b : q.ord) {
        if (b.d) (void)hipFree(b.d);
        for (hipEvent_t e : b.rd_ev)
            if (e) (void)hipEventDestroy(e);
    }
    for (int *p : q.retired) (void)hipFree(p);
    if (q.h_cost) (void)hipHostFree(q.h_cost);
    if (q.h_order) (void)hipHostFree(q.h_order);
    if (q.ev) (void)hipEventDestroy(q.ev);
    if (q.up_ev) (void)hipEventDestroy(q.up_ev);
    q = SptSched();
}

// Work counters of the persistent (8-wide hierarchy) launches: a ring,
// one zeroed quad (rest, routed heavy, cooperative, unused) per launch, so
// launches in flight on several streams do not share one.  After 64 further
// launches an entry comes round again: each uncaptured launch records its
// entry's event after it, and a launch on another stream takes the entry
// only once that event is complete (work_entry; spt_streams.h, RingBook).
// An entry a stream capture used is baked into that graph, which may be
// replayed at any time: it is never handed out again (captured).
// spt_scene_release_captures hands those entries out again once the
// caller has destroyed the graphs.  mu guards the ring's host state
// (launches of one scene from several host threads).
struct WorkRing {
    static constexpr int N = 64;
    int *d = nullptr;                 // N quads (device)
    std::mutex mu;
    sptstreams::RingBook book;
    hipEvent_t ev[N] = {};            // the last uncaptured launch of each entry
    static_assert(N == sptstreams::RingBook::N, "one event per entry");
};

// The ring's device and event storage (scene creation / destruction).
inline hipError_t ring_create(WorkRing &r)
{
    hipError_t e = hipMalloc(&r.d, 4 * sizeof(int) * WorkRing::N);
    for (int k = 0; k < WorkRing::N && e == hipSuccess; k++) e = hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming);
    return e;
}

inline void ring_release(WorkRing &r)
{
    if (r.d) (void)hipFree(r.d);
    for (hipEvent_t e : r.ev)
        if (e) (void)hipEventDestroy(e);
}

// A zeroed work-counter quad of the ring for one persistent launch on `s`
// (nullptr + rt error: none left).
inline int *work_entry(WorkRing &r, hipStream_t s)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
    std::lock_guard<std::mutex> lk(r.mu);
    sptstreams::RingTake t = sptstreams::ring_take(r.book, s, capturing);
    // An entry whose last launch, on another stream, is still running is
    // passed over (an event query; the host does not wait) -- unless every
    // entry is such: then the stream waits for the last one looked at.
    for (int tries = 1; tries < WorkRing::N && t.entry >= 0 && t.wait && hipEventQuery(r.ev[t.entry]) == hipErrorNotReady;
         tries++)
        t = sptstreams::ring_take(r.book, s, capturing);
    if (t.entry < 0) {
        rtrt::fail(RT_ERR_INVALID, "spt render: every work-counter entry of the scene is held by a captured graph");
        return nullptr;
    }
    int *work = r.d + 4 * t.entry;
    if (t.wait && hipStreamWaitEvent(s, r.ev[t.entry], 0) != hipSuccess) return nullptr;   // (check_launch reports it)
    if (hipMemsetAsync(work, 0, 4 * sizeof(int), s) != hipSuccess) return nullptr;
    return work;
}

// After the persistent launch on `s` that uses `work`: the entry's event
// (nothing for a captured launch: its entry is never handed out again).
inline void work_launched(WorkRing &r, const int *work, hipStream_t s)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return;
    std::lock_guard<std::mutex> lk(r.mu);
    const int k = (int)(work - r.d) / 4;
    if (hipEventRecord(r.ev[k], s) == hipSuccess) sptstreams::ring_recorded(r.book, k, s);
}

}  // namespace sptsched

#endif
