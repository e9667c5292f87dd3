"""GPU check of rt_glibc_math.h: device powf/expf/sinf/cosf (v_fma_f64 ...)
vs the host glibc, exhaustively over the hot path's input domains; of
rt_common.h's cvt_i32_x86 for every float; and of rt_spec20.h's rounding
certificate against rtm::pow_d on the device."""
import pytest

pytestmark = pytest.mark.gpu


def test_device_math_matches_host_glibc():
    import gpu_native
    res = gpu_native.math_check()
    bad = {k: v for k, v in res.items() if v[1] != 0}
    assert not bad, bad


def test_device_pow_d_matches_host_glibc():
    """The 3.2.03 queue tracer's pow(float, 20) (g++: glibc double pow)."""
    import gpu_native
    n, bad, first = gpu_native.pow20_check()
    assert n > 1.08e9 and bad == 0, (bad, first)


def test_device_pow_d_matches_host_glibc_above_two():
    """The same for every float in (2, +inf]: the queue tracer calls it with
    any dot > 0 (a plane normal of length 5 gives dots far above 2)."""
    import gpu_native
    n, bad, first = gpu_native.pow20_check(0x40000001, 0x7f800000)
    assert n == 0x7f800000 - 0x40000001 + 1 and bad == 0, (bad, first)


def test_device_cvt_i32_x86_matches_host_conversion():
    """(int)f as x86-64 converts it (cvttss2si: INT_MIN for NaN and overflow),
    every one of the 2^32 float bit patterns, compared as integers."""
    import gpu_native
    n, bad, first = gpu_native.cvt_check()
    assert n == 2 ** 32 and bad == 0, (bad, first)


def _spec20_report_and_check(res, cap, max_uncertified):
    for b, r in sorted(res.items()):
        print("spec20 pspec 0x%08x: certified-but-different %d %s, uncertified device %d %s, host %d %s"
              % (b, r["wrong"][0], [hex(u) for u in r["wrong"][1]], r["uncertified"][0],
                 [hex(u) for u in r["uncertified"][1][:8]], r["host_uncertified"][0],
                 [hex(u) for u in r["host_uncertified"][1][:8]]))
    for b, r in sorted(res.items()):
        assert r["wrong"][0] == 0, (hex(b), r["wrong"])
        # The same inputs: the counts always, and the inputs themselves while
        # the 256-entry lists hold them all.  Past that cap (pspec = +inf on
        # (0, 2]: 613,955,568 inputs whose x^20 underflows to 0, 0 * inf) the
        # device keeps any 256 of them and the host the smallest, so there
        # only the counts are compared, no longer input for input.
        assert r["uncertified"][0] == r["host_uncertified"][0], (hex(b), r["uncertified"][0], r["host_uncertified"][0])
        if r["uncertified"][0] <= cap:
            assert r["uncertified"] == r["host_uncertified"], (hex(b), r)
        assert r["uncertified_hi"] <= max_uncertified, (hex(b), r["uncertified_hi"])
    assert any(r["uncertified"][0] > 0 for r in res.values())


def test_device_spec20_certificate():
    """The queue tracer's specular shortcut on the device (v_mul_f64,
    v_cvt_f32_f64): for every float dp in (0, 2] and every pspec of
    test_glibc_math.spec20_pspec(), a certified spec20<false> equals
    spec20<true> (rtm::pow_d, pinned to glibc's pow above) bit for bit, the
    device leaves uncertified exactly the inputs the host does, and -- so that
    certifying nothing cannot pass -- at most 2^-20 of the dp bit patterns
    [0x3c000000, 0x40000000], and at least one input for some pspec."""
    import gpu_native
    from test_glibc_math import SPEC20_MAX_UNCERTIFIED, spec20_pspec
    res = gpu_native.spec20_check(spec20_pspec())
    _spec20_report_and_check(res, gpu_native.lib().gmc_spec20_cap(), SPEC20_MAX_UNCERTIFIED)


def test_device_spec20_certificate_above_two():
    """The same three assertions for every float dp in (2, +inf] -- what a
    non-unit normal gives -- and every pspec > 0 of spec20_pspec() (queue.hip
    evaluates the factor only where m_spec > 0), +inf, 3e38 and 1e-42 among
    them; the cap is 2^-20 of this range's bit patterns."""
    import gpu_native
    from test_glibc_math import SPEC20_ABOVE2, SPEC20_ABOVE2_MAX_UNCERTIFIED, spec20_pspec_positive
    res = gpu_native.spec20_check(spec20_pspec_positive(), *SPEC20_ABOVE2)
    _spec20_report_and_check(res, gpu_native.lib().gmc_spec20_cap(), SPEC20_ABOVE2_MAX_UNCERTIFIED)
