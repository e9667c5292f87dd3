"""Host check that se-195-project-ray-tracer_amd/csrc/rt_glibc_math.h returns
the host glibc's bits for powf/expf/sinf/cosf/sincosf over the hot path's
input domains (exhaustive: ~1e9 inputs per domain, ~40 s on 8 cores), and
the double pow(x, 20) of the 3.2.03 queue tracer for every float x in (0, 4];
and that rt_spec20.h's rounding certificate (the queue tracer's specular
factor without that pow) never certifies a float the host's pow does not give,
for every float dp in (0, 2] and every pspec of SPEC20_PSPEC."""
import os
import struct
import subprocess

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def spec20_pspec():
    """Every m_spec of the two reference scenes, and 1.0, 1.7, 0.0123 (float32
    bit patterns, ascending)."""
    import oracle_lib as O
    W, nw = O.whitted_scene()
    Q, nq = O.queue_scene()
    vals = [W[i].m_Spec for i in range(nw)] + [Q[i].m_spec for i in range(nq)] + [1.0, 1.7, 0.0123]
    return sorted({f32_bits(v) for v in vals})


# The share of uncertified inputs among the dp bit patterns [0x3c000000,
# 0x40000000] (below them the results underflow) that the certificate may
# leave to the exact path: 2^-20, so that "certify nothing" cannot pass.
SPEC20_RANGE = 0x40000000 - 0x3c000000 + 1
SPEC20_MAX_UNCERTIFIED = SPEC20_RANGE >> 20


def test_glibc_math_exhaustive():
    pspec = spec20_pspec()
    assert len(pspec) >= 8 and f32_bits(1.0) in pspec
    subprocess.run(["make", "-s", "-C", HERE, "glibc_math_check"], check=True)
    out = subprocess.run([os.path.join(HERE, "glibc_math_check")] + ["0x%08x" % b for b in pspec], check=True,
                         capture_output=True, text=True).stdout
    rows = [l.split() for l in out.strip().splitlines()]
    assert len(rows) == 17 + len(pspec), out
    bad = [r for r in rows if int(r[2]) != 0]
    assert not bad, bad
    assert sum(int(r[1]) for r in rows if not r[0].startswith("spec20_")) > 12e9
    spec = {int(r[0][7:], 16): r for r in rows if r[0].startswith("spec20_")}
    assert sorted(spec) == pspec
    for b, r in spec.items():
        uncertified, in_range = int(r[4]), int(r[5])
        print("spec20 pspec 0x%08x: %s inputs, certified-but-wrong %s, uncertified %d (%d at or above 0x3c000000): %s"
              % (b, r[1], r[2], uncertified, in_range, " ".join(r[6:])))
        assert int(r[1]) == 0x40000000 and len(r) == 6 + uncertified
        assert in_range <= SPEC20_MAX_UNCERTIFIED, (hex(b), in_range)
    assert any(int(r[4]) > 0 for r in spec.values()), "no pspec has an uncertified input: nothing reaches the exact path"
