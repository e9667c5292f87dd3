// tests/native/gpu_rng_draw_check.hip -- the device build of GetRandom's
// stream update as smallpt.hip's get_random_f runs it (csrc/spt_rng.h
// mwc_step<true>: a shift and v_mad_u32_u16) against the reference's
// expression A * (s & 65535) + (s >> 16) in plain integer code in the same
// kernel, for all 2^32 values of s and both multipliers; and the float a draw
// is assembled into (sptrng::draw<true>) against the plain form for 2^24
// state pairs: 2^16 hashed starting pairs followed for 256 draws each, both
// forms advancing their own copy of the state.  Built by
// tests/test_gpu_rng_draw.py.  One launch each; prints "name checked
// mismatches first_bad" for s0, s1 (first_bad: the value of s), draw and state
// (first_bad: the draw's index), then "ok (0 failures)" or "FAILED (<n>
// failures)"; exit status 0 / 1, 2 on a HIP error.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "spt_rng.h"

namespace {

namespace rng = rt::sptrng;

struct Tally { unsigned long long bad[4]; unsigned long long first[4]; };

__device__ void note(Tally *t, int k, unsigned bad, unsigned long long first)
{
    if (bad) {
        atomicAdd(&t->bad[k], (unsigned long long)bad);
        atomicMin(&t->first[k], first);
    }
}

// thread i of 2^20 takes s = i, i + 2^20, ...: 4096 values
constexpr unsigned STEP_THREADS = 1u << 20;
__global__ void step_kernel(Tally *t)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned bad0 = 0, bad1 = 0;
    unsigned long long f0 = ~0ull, f1 = ~0ull;
    for (uint32_t r = 0; r < 4096u; r++) {
        const uint32_t s = i + r * STEP_THREADS;
        const uint32_t want0 = 36969u * (s & 65535u) + (s >> 16);
        const uint32_t want1 = 18000u * (s & 65535u) + (s >> 16);
        if (rng::mwc_step<true>(rng::MWC_A0, s) != want0) { bad0++; if (s < f0) f0 = s; }
        if (rng::mwc_step<true>(rng::MWC_A1, s) != want1) { bad1++; if (s < f1) f1 = s; }
    }
    note(t, 0, bad0, f0);
    note(t, 1, bad1, f1);
}

__device__ uint32_t hash32(uint32_t x)
{
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

constexpr unsigned DRAW_THREADS = 1u << 16, DRAW_CHAIN = 256;
__global__ void draw_kernel(Tally *t)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t a0 = hash32(2 * i + 1), a1 = hash32(2 * i + 2);        // the new form's state
    if (i == 0) { a0 = 0; a1 = 0; }
    if (i == 1) { a0 = ~0u; a1 = ~0u; }
    if (i == 2) { a0 = 0xffffu; a1 = 0xffff0000u; }
    uint32_t b0 = a0, b1 = a1;                                      // the plain form's
    unsigned badf = 0, bads = 0;
    unsigned long long ff = ~0ull, fs = ~0ull;
    for (uint32_t r = 0; r < DRAW_CHAIN; r++) {
        const uint32_t got = rng::draw<true>(a0, a1);
        b0 = 36969u * (b0 & 65535u) + (b0 >> 16);                   // simplernd.h:34-48
        b1 = 18000u * (b1 & 65535u) + (b1 >> 16);
        const uint32_t ires = (b0 << 16) + b1;
        const uint32_t want = (ires & 0x007fffffu) | 0x40000000u;
        const unsigned long long at = (unsigned long long)i * DRAW_CHAIN + r;
        if (got != want) { badf++; if (at < ff) ff = at; }
        if (a0 != b0 || a1 != b1) { bads++; if (at < fs) fs = at; }
    }
    note(t, 2, badf, ff);
    note(t, 3, bads, fs);
}

}  // namespace

int main()
{
    Tally h, *d = nullptr;
    for (int k = 0; k < 4; k++) { h.bad[k] = 0; h.first[k] = ~0ull; }
    if (hipMalloc(&d, sizeof(Tally)) != hipSuccess) return 2;
    bool ok = hipMemcpy(d, &h, sizeof(Tally), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        hipLaunchKernelGGL(step_kernel, dim3(STEP_THREADS / 256), dim3(256), 0, 0, d);
        hipLaunchKernelGGL(draw_kernel, dim3(DRAW_THREADS / 256), dim3(256), 0, 0, d);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(&h, d, sizeof(Tally), hipMemcpyDeviceToHost) == hipSuccess;
    }
    (void)hipFree(d);
    if (!ok) {
        fprintf(stderr, "HIP error\n");
        return 2;
    }
    const char *const names[4] = {"s0", "s1", "draw", "state"};
    const unsigned long long checked[4] = {1ull << 32, 1ull << 32, (unsigned long long)DRAW_THREADS * DRAW_CHAIN,
                                           (unsigned long long)DRAW_THREADS * DRAW_CHAIN};
    unsigned long long failures = 0;
    for (int k = 0; k < 4; k++) {
        printf("%s %llu %llu 0x%08llx\n", names[k], checked[k], h.bad[k], h.bad[k] ? h.first[k] : 0ull);
        failures += h.bad[k];
    }
    printf(failures ? "FAILED (%llu failures)\n" : "ok (%llu failures)\n", failures);
    return failures ? 1 : 0;
}
