// rt_levelpass.h -- host plumbing the two level-pass tracers share (whitted.hip,
// queue.hip): the wait for the previous frame, arena carving, the frame
// bracket (ordering after the previous frame, fork to / join from the second
// stream), the equal-slab row split and the blocking entry points' staging.
// Policy -- slab sizes, pool fractions, when to use two streams, the kernel
// launch sequences -- stays in the tracers.  Host-only.
#ifndef RT_LEVELPASS_H
#define RT_LEVELPASS_H

#include <stdio.h>
#include "rt_runtime.h"

namespace rtrt {

// Host wait for the previous frame (its arena, tables and staging slots).
inline int wait_frame(DeviceState &st, const char *what)
{
    hipError_t e = hipEventSynchronize(st.wf_done);
    if (e != hipSuccess) return fail_hip(e, what);
    st.wf_pending = false;
    return RT_OK;
}

// Device slot of at least `bytes` that the previous frame may still read:
// regrowing frees it, so wait for that frame first.
inline int frame_scratch(DeviceState &st, int slot, size_t bytes, void **out)
{
    if (st.cap[slot] < bytes && st.wf_pending) {
        int rc = wait_frame(st, "level pass frame wait");
        if (rc) return rc;
    }
    return scratch(st, slot, bytes, out);
}

// Resident blocks of a 256-thread kernel on this device (persistent grids).
template <class K>
int resident_blocks(K kernel)
{
    int dev = 0, cus = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 1024;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 1024;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, 256, 0) != hipSuccess || per < 1) per = 1;
    return cus * per;
}

// An arena's parts, each rounded to 256 B, in the order they are taken.
// Without a base it only adds the sizes up; carve_arena runs the tracer's
// list of parts once that way and once over the slot, so the size and the
// layout cannot disagree.
struct Arena {
    char *base = nullptr;
    size_t used = 0;
    template <class T>
    void take(T *&part, size_t bytes)
    {
        if (base) part = (T *)(base + used);
        used += (bytes + 255) & ~(size_t)255;
    }
};

// Scratch slot `slot` (grow-only) carved into `parts(Arena &)`.
template <class Parts>
int carve_arena(DeviceState &st, int slot, Parts parts)
{
    Arena sizing;
    parts(sizing);
    void *base = nullptr;
    int rc = frame_scratch(st, slot, sizing.used, &base);
    if (rc) return rc;
    Arena a;
    a.base = (char *)base;
    parts(a);
    return RT_OK;
}

// 16-B words of `bytes` (prep_kernel's zero fill: the arena rounds every part
// to 256 B).
inline int words16(size_t bytes) { return (int)((bytes + 15) / 16); }

// Rows of slab k of n equal slabs that interleave in 16-row groups over
// `ngroups` groups (k = 0: the largest).
inline int slab_rows(int ngroups, int k, long long n) { return (int)((ngroups - k + n - 1) / n) * 16; }

// One asynchronous level-pass frame on the caller's stream s.  The arenas
// (and Whitted's view tables) belong to the device, so begin() orders the
// frame after the previous level-pass frame, whatever stream that ran on;
// fork() brings in the state's second stream for frames whose slabs alternate
// between two; after it, an error return goes through bail(), which still
// joins the second stream back; end() joins it and records wf_done.
struct Frame {
    DeviceState &st;
    hipStream_t s;
    const char *name;              // the entry point, for error texts
    hipStream_t ss[2];             // stream of slab k: ss[k % nstream]
    int nstream = 1;

    Frame(DeviceState &st_, hipStream_t s_, const char *name_) : st(st_), s(s_), name(name_), ss{s_, s_} {}
    int hip_error(hipError_t e, const char *step)
    {
        char what[96];
        snprintf(what, sizeof(what), "%s %s", name, step);
        return fail_hip(e, what);
    }
    int begin()
    {
        if (!st.wf_pending) return RT_OK;
        hipError_t e = hipStreamWaitEvent(s, st.wf_done, 0);
        return e == hipSuccess ? RT_OK : hip_error(e, "wait");
    }
    int fork()
    {
        int rc = aux_stream(st);
        if (rc) return rc;
        hipError_t e = hipEventRecord(st.fork_ev, s);
        if (e == hipSuccess) e = hipStreamWaitEvent(st.aux, st.fork_ev, 0);
        if (e != hipSuccess) return hip_error(e, "fork");
        ss[1] = st.aux;
        nstream = 2;
        return RT_OK;
    }
    int bail(int rc) { return nstream == 2 ? join_aux_on_error(st, s, rc) : rc; }
    int end()
    {
        if (nstream == 2) {
            hipError_t e = hipEventRecord(st.join_ev, st.aux);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, st.join_ev, 0);
            if (e != hipSuccess) return bail(hip_error(e, "join"));
        }
        hipError_t e = hipEventRecord(st.wf_done, s);
        if (e != hipSuccess) return hip_error(e, "record");
        st.wf_pending = true;
        return RT_OK;
    }
};

// A blocking entry point around an asynchronous one: the primitives copied
// up (scratch slot 0), the four work counters zeroed (slot 2, when asked
// for), issue(d_prims, d_frame, d_counters, stream) run on the state's
// stream over a w x h frame in slot 1, rows [row_begin, row_end) of it and
// the counters copied back, and the stream synchronised.  Rows outside the
// window are left untouched in `out`.
template <class Prim, class Issue>
int render_blocking(const char *name, const Prim *prims, int nprims, uint32_t *out, int w, int h, int row_begin,
                    int row_end, uint64_t *counters, Issue issue)
{
    DeviceState *st;
    int rc = state(&st);
    if (rc) return rc;
    std::lock_guard<std::recursive_mutex> lk(st->mu);
    // slots 0..2 may still feed a frame issued on another stream
    if (st->wf_pending && (rc = wait_frame(*st, name))) return rc;
    void *d_prims, *d_frame, *d_cnt;
    if ((rc = scratch(*st, 0, sizeof(Prim) * nprims, &d_prims))) return rc;
    if ((rc = scratch(*st, 1, sizeof(uint32_t) * (size_t)w * h, &d_frame))) return rc;
    if ((rc = scratch(*st, 2, 4 * sizeof(uint64_t), &d_cnt))) return rc;
    hipStream_t s = st->stream;
    char what[96];
    snprintf(what, sizeof(what), "%s H2D", name);
    hipError_t e = hipMemcpyAsync(d_prims, prims, sizeof(Prim) * nprims, hipMemcpyHostToDevice, s);
    if (e == hipSuccess && counters) e = hipMemsetAsync(d_cnt, 0, 4 * sizeof(uint64_t), s);
    if (e != hipSuccess) return fail_hip(e, what);
    if ((rc = issue((const Prim *)d_prims, (uint32_t *)d_frame, counters ? (uint64_t *)d_cnt : nullptr, s))) return rc;
    const size_t off = sizeof(uint32_t) * (size_t)row_begin * w, len = sizeof(uint32_t) * (size_t)(row_end - row_begin) * w;
    snprintf(what, sizeof(what), "%s D2H", name);
    e = hipMemcpyAsync((char *)out + off, (char *)d_frame + off, len, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess && counters)
        e = hipMemcpyAsync(counters, d_cnt, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail_hip(e, what);
    return RT_OK;
}

}  // namespace rtrt

#endif
