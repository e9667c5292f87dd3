// tests/native/gpu_sincos_draw_check.hip -- the device build of
// rtm::sincos_2pi_draw (csrc/rt_glibc_math.h) and rt::sqrt_nr(1 - u)
// (csrc/rt_common.h) on every GetRandom draw u = m * 2^-23, 0 <= m < 2^23,
// against the host libm.  Built by tests/test_gpu_sincos_draw.py.
// One launch; prints "name checked mismatches first_bad_m" for sin, cos,
// bits_sin, bits_cos (sincos_2pi_draw_bits fed the [2, 4) float's bits, as
// smallpt.hip's pass B calls it) and sqrt, then "ok (0 failures)" or "FAILED
// (<n> failures)"; exit status 0 / 1, 2 on a HIP error.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <thread>
#include <vector>
#include "rt_glibc_math.h"
#include "rt_common.h"

namespace {

constexpr uint32_t N = 1u << 23;
constexpr float PI_F = 3.14159265358979323846f;
constexpr int NOUT = 5, T = 16;

struct Out { uint32_t v[NOUT]; };

__global__ void draw_kernel(Out *out)
{
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= N) return;
    const float f = __uint_as_float(m | 0x40000000u);           // get_random_f
    const float u = __builtin_fmaf(f, .5f, -1.f);               // get_random
    float sn, cs, a, b;
    rtm::sincos_2pi_draw(u, sn, cs);
    rtm::sincos_2pi_draw_bits(__float_as_uint(f), u, a, b);
    Out o;
    o.v[0] = rtm::f2u(sn);
    o.v[1] = rtm::f2u(cs);
    o.v[2] = rtm::f2u(a);
    o.v[3] = rtm::f2u(b);
    o.v[4] = rtm::f2u(rt::sqrt_nr(1 - u));
    out[m] = o;
}

}  // namespace

int main()
{
    Out *d = nullptr;
    std::vector<Out> h(N);
    if (hipMalloc(&d, sizeof(Out) * N) != hipSuccess) return 2;
    hipLaunchKernelGGL(draw_kernel, dim3(N / 256), dim3(256), 0, 0, d);
    const bool ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(h.data(), d, sizeof(Out) * N, hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(d);
    if (!ok) {
        fprintf(stderr, "HIP error\n");
        return 2;
    }
    unsigned long long bad[T][NOUT] = {};
    uint32_t first[T][NOUT];
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++)
        th.emplace_back([&, t]() {
            for (int p = 0; p < NOUT; p++) first[t][p] = ~0u;
            for (uint32_t m = N / T * t; m < N / T * (t + 1); m++) {
                const float u = (float)m * 0x1p-23f;
                const float phi = 2.f * PI_F * u;
                const uint32_t want[NOUT] = {rtm::f2u(::sinf(phi)), rtm::f2u(::cosf(phi)), rtm::f2u(::sinf(phi)),
                                             rtm::f2u(::cosf(phi)), rtm::f2u(::sqrtf(1 - u))};
                for (int p = 0; p < NOUT; p++)
                    if (h[m].v[p] != want[p]) { bad[t][p]++; if (m < first[t][p]) first[t][p] = m; }
            }
        });
    for (auto &x : th) x.join();
    const char *const names[NOUT] = {"sin", "cos", "bits_sin", "bits_cos", "sqrt"};
    unsigned long long failures = 0;
    for (int p = 0; p < NOUT; p++) {
        unsigned long long b = 0;
        uint32_t f = ~0u;
        for (int t = 0; t < T; t++) { b += bad[t][p]; if (first[t][p] < f) f = first[t][p]; }
        printf("%s %u %llu 0x%06x\n", names[p], N, b, f == ~0u ? 0u : f);
        failures += b;
    }
    printf(failures ? "FAILED (%llu failures)\n" : "ok (%llu failures)\n", failures);
    return failures ? 1 : 0;
}
