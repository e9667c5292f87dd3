// spt_rng.h -- GetRandom's two multiply-with-carry streams (simplernd.h:34-48)
// and the [2, 4) float a draw is assembled into.
//
// One stream update is s' = A * (s & 65535) + (s >> 16) with A = 36969 (s0) or
// 18000 (s1).  The compiler writes it as v_and_b32 0xffff, v_lshrrev_b32 16,
// v_mad_u32_u24: three VALU.  gfx950's v_mad_u32_u16 computes
// D = S0[15:0] * S1[15:0] + S2 in 32 bits: it reads the low half itself, so
// the mask goes and an update is two VALU (the compiler does not pick the
// instruction).  A <= 36969 and the low half <= 65535 give a product below
// 2^32, and the 32-bit sum wraps as the C expression's does.  MAD16 = false
// (and every host build) keeps the plain expression.  Checked on the device
// for all 2^32 values of either stream (tests/test_gpu_rng_draw.py).
#ifndef SPT_RNG_H
#define SPT_RNG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rt {
namespace sptrng {

constexpr uint32_t MWC_A0 = 36969u, MWC_A1 = 18000u;

__host__ __device__ constexpr uint32_t mwc_step_plain(uint32_t a, uint32_t s) { return a * (s & 65535u) + (s >> 16); }

template <bool MAD16>
__host__ __device__ __forceinline__ uint32_t mwc_step(uint32_t a, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (MAD16) {
        uint32_t d;
        asm("v_mad_u32_u16 %0, %1, %2, %3" : "=v"(d) : "v"(s), "s"(a), "v"(s >> 16));
        return d;
    }
#endif
    return mwc_step_plain(a, s);
}

// The draw's float in [2, 4): the reference maps it to (f - 2) / 2.
__host__ __device__ constexpr uint32_t draw_bits(uint32_t s0, uint32_t s1)
{
    return (((s0 << 16) + s1) & 0x007fffffu) | 0x40000000u;
}

// Advances both streams and returns the draw's float bits.
template <bool MAD16>
__host__ __device__ __forceinline__ uint32_t draw(uint32_t &s0, uint32_t &s1)
{
    s0 = mwc_step<MAD16>(MWC_A0, s0);
    s1 = mwc_step<MAD16>(MWC_A1, s1);
    return draw_bits(s0, s1);
}

}  // namespace sptrng
}  // namespace rt

#endif
