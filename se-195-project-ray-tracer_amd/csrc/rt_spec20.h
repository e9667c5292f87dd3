// rt_spec20.h -- the queue tracer's specular factor (queue.hip), host and
// device, so that its rounding certificate can be checked on both against
// the double pow it stands for (tests/test_glibc_math.py on the host,
// tests/test_gpu_math.py on the device).
#ifndef RT_SPEC20_H
#define RT_SPEC20_H

#include "rt_glibc_math.h"

namespace rt {
namespace queue {

// The specular factor (float)(pow((double)dp, 20.0) * (double)pspec) of
// raytracer_non_OpenCL.c:270 -- g++'s promoting std::pow, i.e. glibc's double
// pow -- without the table-driven pow.  x^20 by repeated squaring in double is within 2^-50 of
// x^20 (a float x squares exactly; four more roundings), and glibc's pow is
// within 0.52 ulp of it, so the double product glibc's value gives lies
// within 2^-49 of d = p * pspec.  If d * (1 - 2^-48) and d * (1 + 2^-48)
// round to the same float, so does that product (rounding is monotonic):
// that float is the reference's.  Otherwise (a float rounding boundary within
// 2^-48 of d, about one evaluation in 2^24) `amb` is set and the caller
// re-evaluates the node with rtm::pow_d (EXACT).  UNCERT (test hook,
// RT_QUEUE_EXACT_ALL=1): no term is certified, every one takes that path.
template <bool EXACT, bool UNCERT = false>
RTM_HD float spec20(float dp, float pspec, bool &amb)
{
    if (EXACT) return (float)(rtm::pow_d((double)dp, 20.0) * (double)pspec);
    const double x = (double)dp, x2 = x * x, x4 = x2 * x2, x8 = x4 * x4, x16 = x8 * x8;
    const double d = (x16 * x4) * (double)pspec;
    const float lo = (float)(d * (1.0 - 0x1p-48)), hi = (float)(d * (1.0 + 0x1p-48));
    amb |= lo != hi || UNCERT;
    return lo;
}

// The same factor for a light the shadow ray found occluded: the reference
// still evaluates (float)(pow((double)dp, 20.0) * (double)pspec * 0.0), which
// is +0 while the product is finite and NaN once it is not (inf * 0).  For
// 0 < dp <= 2^25 and a finite pspec > 0 the product is below 2^501 * 2^128:
// finite, so +0 without any pow.  Everything else (a normal of length 5 and a
// non-unit ray can give dp far above 2; m_spec may be inf) is left to the
// exact path, like an uncertified term.
template <bool EXACT, bool UNCERT = false>
RTM_HD float spec20_occluded(float dp, float pspec, bool &amb)
{
    if (EXACT) return (float)(rtm::pow_d((double)dp, 20.0) * (double)pspec * 0.0);
    amb |= !(dp <= 0x1p25f && pspec <= 3.40282347e38f) || UNCERT;
    return 0.0f;
}

}  // namespace queue
}  // namespace rt

#endif
