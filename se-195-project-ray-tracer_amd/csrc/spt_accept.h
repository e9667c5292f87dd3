// spt_accept.h -- the accept tests of smallpt's branch-free sphere loops
// (smallpt.hip: query_bf, shadow_bf), restated on an order-preserving integer
// key so that a sphere's two roots, the "> EPS" tests and the running bound
// fold into one unsigned three-way minimum.  Host and device include this
// header; tests/native/accept_key_check.cpp proves every statement below on
// the CPU, the first three for all 2^32 bit patterns.
//
//   key(x) = bits(x) - (bits(EPS) + 1)   as uint32_t,   KEY_INF = key(+inf)
//
// A *candidate* root is a finite x > EPS.
//   1. A candidate has key(x) < KEY_INF, and key is strictly increasing over
//      the candidates (positive floats order as their bit patterns).
//   2. Everything else -- x <= EPS, +-0, negative, -inf, +inf, NaN -- has
//      key(x) >= KEY_INF: below bits(EPS) + 1 the subtraction wraps to at
//      least 2^32 - bits(EPS) - 1, and a set sign bit leaves at least 2^31 -
//      bits(EPS) - 1; both exceed KEY_INF.
//   3. A running bound is a limit key L = limit_key(t): key(t) for t > EPS
//      (a finite bound, or +inf: every candidate passes), 0 for t <= EPS or
//      NaN (nothing passes).  Then  x > EPS && x < t  <=>  key(x) < L  for
//      every x, and for two candidates d < t <=> key(d) < key(t).
//   4. The roots are t1 = b - sd, t2 = b + sd with sd >= 0 or NaN (sqrt_nr),
//      so t1 <= t2, or neither is a candidate.  SphereIntersect's distance
//      (geomfunc.h:32-59) is t1 if t1 > EPS, else t2 if t2 > EPS, else a
//      miss; min(key(t1), key(t2)) is that distance's key, or >= KEY_INF on
//      a miss (a t2 = +inf behind a non-candidate t1 is no hit for any caller:
//      "+inf < t" fails for their finite t).
//   5. Nearest hit (Intersect, :71-92): with the bound kept as a key tb,
//      tb' = min(tb, key(t1), key(t2)) and take = tb' != tb is "d != 0 &&
//      d < t" -- strict, so a tie keeps the earlier (higher) index.  The
//      distance comes back once per query as unkey(tb).
//   6. Any hit (IntersectP, :94-110): "some root in (EPS, maxt)" is "the
//      reference's d in (EPS, maxt)" (d is the smaller candidate), so
//      acc = min over all spheres and roots of key, occluded = acc < L(maxt).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPT_ACCEPT_HD __host__ __device__ __forceinline__
#else
#define SPT_ACCEPT_HD inline
#endif

namespace rt {
namespace sptaccept {

constexpr float EPS = 0.01f;                              // geom.h:29
constexpr uint32_t EPS_BITS = 0x3c23d70au;
constexpr uint32_t KEY_BIAS = EPS_BITS + 1u;              // bits of the smallest candidate
constexpr uint32_t KEY_INF = 0x7f800000u - KEY_BIAS;
constexpr uint32_t KEY_NONE = 0xffffffffu;                // start of an any-hit minimum
static_assert(__builtin_bit_cast(uint32_t, EPS) == EPS_BITS, "EPS_BITS is not bits(EPS)");

SPT_ACCEPT_HD uint32_t key(float x) { return __builtin_bit_cast(uint32_t, x) - KEY_BIAS; }
SPT_ACCEPT_HD float unkey(uint32_t k) { return __builtin_bit_cast(float, k + KEY_BIAS); }

// The limit a root's key must stay below to lie in (EPS, t).
SPT_ACCEPT_HD uint32_t limit_key(float t) { return t > EPS ? key(t) : 0u; }

// On the device the three-way minimum is stated as the one instruction it
// is: from the C++ form the compiler derives "taken" from min(k1, k2) < tb
// and lowers the bound with a second two-way minimum -- one VALU operation
// more per sphere.
SPT_ACCEPT_HD uint32_t min3(uint32_t a, uint32_t b, uint32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t m;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
#else
    const uint32_t m = b < c ? b : c;
    return a < m ? a : m;
#endif
}

// One sphere of the nearest-hit loop: lowers the bound tb to the sphere's
// distance and returns true iff it is taken (d != 0 && d < t).
SPT_ACCEPT_HD bool nearest_accept(uint32_t &tb, float t1, float t2)
{
    const uint32_t nb = min3(tb, key(t1), key(t2));
    const bool take = nb != tb;
    tb = nb;
    return take;
}

// The distance a nearest-hit query returns: the bound's float.  A t_in > EPS
// that nothing lowered comes back as itself (unkey(key(t_in)), +inf too); a
// t_in <= EPS or NaN, whose limit key 0 is no float's key, is passed through.
SPT_ACCEPT_HD float nearest_result(uint32_t tb, float t_in) { return t_in > EPS ? unkey(tb) : t_in; }

// One sphere of the any-hit loop (acc starts at KEY_NONE), and its outcome.
SPT_ACCEPT_HD void any_accept(uint32_t &acc, float t1, float t2) { acc = min3(acc, key(t1), key(t2)); }
SPT_ACCEPT_HD bool any_result(uint32_t acc, float maxt) { return acc < limit_key(maxt); }

}  // namespace sptaccept
}  // namespace rt
