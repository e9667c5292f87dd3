"""Device check of rtm::sincos_2pi_draw (csrc/rt_glibc_math.h) and of
sqrt_nr(1 - u) (csrc/rt_common.h) over all 2^23 GetRandom draws u = m * 2^-23:
tests/native/gpu_sincos_draw_check.hip, built with hipcc into the test's
temporary directory, evaluates every draw in one launch and compares, on the
host, with the libm's sinf and cosf of 2.f * PI_F * u and with sqrtf(1 - u).
Every count must be 0 of 8,388,608."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "se-195-project-ray-tracer_amd", "csrc")
SRC = os.path.join(HERE, "native", "gpu_sincos_draw_check.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
DRAWS = 1 << 23
PROPERTIES = ["sin", "cos", "bits_sin", "bits_cos", "sqrt"]


def test_every_draw_on_the_device(tmp_path):
    exe = str(tmp_path / "gpu_sincos_draw_check")
    # the product's flags (se-195-project-ray-tracer_amd/Makefile)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-pthread", "-I" + CSRC, "-o", exe, SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    rows = [l.split() for l in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows[:-1]] == PROPERTIES, out.stdout + out.stderr
    for name, checked, bad, first in rows[:-1]:
        assert int(checked) == DRAWS, (name, checked)
        assert int(bad) == 0, "%s: %s of %s draws differ, first m = %s" % (name, bad, checked, first)
    assert out.returncode == 0 and rows[-1] == ["ok", "(0", "failures)"], out.stdout + out.stderr
