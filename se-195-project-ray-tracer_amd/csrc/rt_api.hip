// rt_api.hip -- runtime part of the C-ABI (include/rt_hip.h): device
// selection, error reporting, cached device buffers.  The reference's OpenCL
// hosts print and exit(-1) on any failure (openCLcode.cpp:52-55,
// smallptGPU.cpp:77-81); this boundary returns status codes instead and the
// drop-in shims (shim_*.cpp) restore the print-and-exit behaviour.
#include <mutex>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>
#include "rt_runtime.h"

namespace rtrt {

namespace {
thread_local char g_err[512] = "";
thread_local int g_dev = -1;
std::mutex g_mu;
DeviceState *g_states[64] = {};

void release_state(DeviceState *st)
{
    if (!st) return;
    (void)hipSetDevice(st->device);
    if (st->stream) (void)hipStreamSynchronize(st->stream);
    if (st->aux) (void)hipStreamSynchronize(st->aux);     // slabs of a frame that failed before its join
    if (st->wf_done) (void)hipEventSynchronize(st->wf_done);
    for (int i = 0; i < NSCRATCH; i++)
        if (st->buf[i]) (void)hipFree(st->buf[i]);
    if (st->pool_ovf) (void)hipHostFree(st->pool_ovf);   // host-mapped overflow flags
    if (st->wf_done) (void)hipEventDestroy(st->wf_done);
    if (st->fork_ev) (void)hipEventDestroy(st->fork_ev);
    if (st->join_ev) (void)hipEventDestroy(st->join_ev);
    if (st->aux) (void)hipStreamDestroy(st->aux);
    if (st->stream) (void)hipStreamDestroy(st->stream);
    delete st;
}
}  // namespace

int aux_stream(DeviceState &st)
{
    if (st.aux) return RT_OK;
    hipError_t e = hipEventCreateWithFlags(&st.fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&st.join_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.aux, hipStreamNonBlocking);
    if (e != hipSuccess) {
        if (st.fork_ev) (void)hipEventDestroy(st.fork_ev);
        if (st.join_ev) (void)hipEventDestroy(st.join_ev);
        st.fork_ev = st.join_ev = nullptr;
        st.aux = nullptr;
        return fail_hip(e, "aux stream");
    }
    return RT_OK;
}

int join_aux_on_error(DeviceState &st, hipStream_t s, int rc)
{
    // Work already queued on aux keeps running: the caller's stream (and the
    // next frame, through wf_done) must still wait for it.  The error text
    // of rc is kept (rt_last_error).
    if (st.aux && hipEventRecord(st.join_ev, st.aux) == hipSuccess &&
        hipStreamWaitEvent(s, st.join_ev, 0) == hipSuccess && hipEventRecord(st.wf_done, s) == hipSuccess)
        st.wf_pending = true;
    else if (st.aux)
        (void)hipStreamSynchronize(st.aux);
    return rc;
}

int fail(int code, const char *msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return code;
}

int fail_hip(hipError_t e, const char *what)
{
    snprintf(g_err, sizeof(g_err), "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
    return RT_ERR_HIP;
}

int check_launch(const char *what)
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? RT_OK : fail_hip(e, what);
}

int state(DeviceState **out)
{
    int dev = g_dev;
    if (dev < 0) {
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return fail_hip(e, "hipGetDevice");
    }
    if (dev < 0 || dev >= 64) return fail(RT_ERR_NODEVICE, "device index out of range");
    std::lock_guard<std::mutex> lk(g_mu);
    DeviceState *st = g_states[dev];
    if (!st) {
        hipError_t e = hipSetDevice(dev);
        if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
        hipDeviceProp_t prop;
        e = hipGetDeviceProperties(&prop, dev);
        if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            char m[160];
            snprintf(m, sizeof(m), "device %d is %s; these kernels are built for gfx950 only", dev,
                     prop.gcnArchName);
            return fail(RT_ERR_NODEVICE, m);
        }
        st = new DeviceState();
        st->device = dev;
        st->cus = prop.multiProcessorCount;
        e = hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete st; return fail_hip(e, "hipStreamCreate"); }
        e = hipEventCreateWithFlags(&st->wf_done, hipEventDisableTiming);
        if (e != hipSuccess) {
            (void)hipStreamDestroy(st->stream);
            delete st;
            return fail_hip(e, "hipEventCreate");
        }
        e = hipHostMalloc((void **)&st->pool_ovf, POOL_OVF_FLAGS * sizeof(int), hipHostMallocMapped | hipHostMallocCoherent);
        if (e == hipSuccess) e = hipHostGetDevicePointer((void **)&st->pool_ovf_dev, st->pool_ovf, 0);
        if (e != hipSuccess) {
            (void)hipEventDestroy(st->wf_done);
            (void)hipStreamDestroy(st->stream);
            if (st->pool_ovf) (void)hipHostFree(st->pool_ovf);
            delete st;
            return fail_hip(e, "hipHostMalloc");
        }
        memset(st->pool_ovf, 0, POOL_OVF_FLAGS * sizeof(int));
        g_states[dev] = st;
        // The second stream (two-slab level-pass frames) is created with the
        // state, not at its first use: created mid-run it ran the 1080p
        // queue frame's second slab measurably less concurrently (1.43-1.45
        // -> 1.36-1.40 ms; Whitted 1080p best 1.49-1.50 -> 1.47-1.48 ms,
        // profiles/r06/aux_stream_at_state_ab.log).  Not fatal here: a later
        // aux_stream() call retries and reports.
        (void)aux_stream(*st);
    } else {
        hipError_t e = hipSetDevice(dev);
        if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    }
    *out = st;
    return RT_OK;
}

int scratch(DeviceState &st, int slot, size_t bytes, void **out)
{
    if (slot < 0 || slot >= NSCRATCH) return fail(RT_ERR_INVALID, "scratch slot");
    if (bytes == 0) bytes = 16;
    if (st.cap[slot] < bytes) {
        if (st.buf[slot]) {
            hipError_t e = hipStreamSynchronize(st.stream);
            if (e == hipSuccess && st.aux) e = hipStreamSynchronize(st.aux);
            if (e != hipSuccess) return fail_hip(e, "scratch sync");
            (void)hipFree(st.buf[slot]);
            st.cached_bytes -= st.cap[slot];
            st.buf[slot] = nullptr;
            st.cap[slot] = 0;
        }
        hipError_t e = hipMalloc(&st.buf[slot], bytes);
        if (e != hipSuccess) { st.buf[slot] = nullptr; return fail_hip(e, "hipMalloc"); }
        st.cap[slot] = bytes;
        st.cached_bytes += bytes;
    }
    *out = st.buf[slot];
    return RT_OK;
}

// RT_POOL_FRAC (test hook: a small first pool, which overflows) over `initial`.
static double first_fraction(double initial)
{
    if (const char *e = getenv("RT_POOL_FRAC")) {
        const double v = atof(e);
        if (v > 0.0 && v < POOL_FRAC_MAX) return v;
    }
    return initial;
}

double pool_fraction(DeviceState &st, int which, long long trees, double initial, int **flag_dev)
{
    if (which == POOL_WHITTED_TRACE || which == POOL_QUEUE_TRACE) {
        const int k = which == POOL_QUEUE_TRACE ? 1 : 0;
        double *frac = st.trace_frac[k];
        int b = 0;
        while (b < POOL_TRACE_BUCKETS - 1 && (1LL << b) < trees) b++;
        const int slot = POOL_FITS + k * POOL_TRACE_BUCKETS + b;
        volatile int *flag = st.pool_ovf + slot;
        if (frac[b] == 0.0) {
            frac[b] = first_fraction(initial);
        } else if (*flag) {
            const double f = frac[b] * 1.25;
            frac[b] = f < POOL_FRAC_MAX ? f : POOL_FRAC_MAX;
        }
        *flag = 0;
        *flag_dev = st.pool_ovf_dev + slot;
        return frac[b];
    }
    int i = 0;
    while (i < POOL_FITS && !(st.pool_fit[i].which == which && st.pool_fit[i].trees == trees)) i++;
    volatile int *flag;
    if (i == POOL_FITS) {                          // a new size: replace the oldest entry
        // A frame of the evicted size may still be in flight and raise the
        // slot's flag after it is cleared (a spurious growth of the new
        // entry): wait for it first (eviction is rare).
        if (st.wf_pending) {
            (void)hipEventSynchronize(st.wf_done);
            st.wf_pending = false;
        }
        i = st.pool_fit_next;
        st.pool_fit_next = (i + 1) % POOL_FITS;
        st.pool_fit[i].which = which;
        st.pool_fit[i].trees = trees;
        st.pool_fit[i].frac = first_fraction(initial);
        flag = st.pool_ovf + i;
        *flag = 0;
    } else {
        flag = st.pool_ovf + i;
        if (*flag) {
            *flag = 0;
            const double f = st.pool_fit[i].frac * 1.25;
            st.pool_fit[i].frac = f < POOL_FRAC_MAX ? f : POOL_FRAC_MAX;
        }
    }
    *flag_dev = st.pool_ovf_dev + i;
    return st.pool_fit[i].frac;
}

int thread_device() { return g_dev; }

DeviceScope::DeviceScope() : saved_rt(g_dev) { (void)hipGetDevice(&saved_hip); }

DeviceScope::~DeviceScope()
{
    g_dev = saved_rt;
    (void)hipSetDevice(saved_hip);
}

int DeviceScope::select(int device)
{
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail_hip(e, "hipSetDevice");
    g_dev = device;
    return RT_OK;
}

}  // namespace rtrt

extern "C" const char *rt_last_error(void) { return rtrt::g_err; }

extern "C" int rt_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return rtrt::fail_hip(e, "hipGetDeviceCount");
    return n;
}

extern "C" int rt_set_device(int device)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return rtrt::fail_hip(e, "hipGetDeviceCount");
    if (device < 0 || device >= n) return rtrt::fail(RT_ERR_NODEVICE, "rt_set_device: no such device");
    e = hipSetDevice(device);
    if (e != hipSuccess) return rtrt::fail_hip(e, "hipSetDevice");
    rtrt::g_dev = device;
    return RT_OK;
}

extern "C" int rt_release(void)
{
    rtrt::release_cached_multi();
    rtrt::release_cached_scenes();        // under each device state's lock
    std::lock_guard<std::mutex> lk(rtrt::g_mu);
    for (int d = 0; d < 64; d++) {
        if (rtrt::g_states[d]) {
            rtrt::release_state(rtrt::g_states[d]);
            rtrt::g_states[d] = nullptr;
        }
    }
    return RT_OK;
}

extern "C" size_t rt_cached_bytes(void)
{
    std::lock_guard<std::mutex> lk(rtrt::g_mu);
    size_t s = 0;
    for (int d = 0; d < 64; d++)
        if (rtrt::g_states[d]) s += rtrt::g_states[d]->cached_bytes;
    return s;
}

extern "C" int rt_host_alloc(size_t bytes, void **out)
{
    if (!out || bytes == 0) return rtrt::fail(RT_ERR_INVALID, "rt_host_alloc: bad arguments");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return rtrt::fail_hip(e, "rt_host_alloc");
    return RT_OK;
}

extern "C" int rt_host_free(void *p)
{
    if (!p) return RT_OK;
    hipError_t e = hipHostFree(p);
    if (e != hipSuccess) return rtrt::fail_hip(e, "rt_host_free");
    return RT_OK;
}

extern "C" void spt_seed_fill(uint32_t *seeds, size_t n, unsigned seed)
{
    srand(seed);
    for (size_t i = 0; i < n; i++) {
        seeds[i] = (uint32_t)rand();
        if (seeds[i] < 2) seeds[i] = 2;
    }
}
