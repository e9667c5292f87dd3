"""Device check of GetRandom's stream update as get_random_f runs it
(csrc/spt_rng.h: a shift and v_mad_u32_u16 in place of and, shift and
v_mad_u32_u24): tests/native/gpu_rng_draw_check.hip, built with hipcc into the
test's temporary directory, evaluates mwc_step<true> for all 2^32 values of
either stream in one launch and compares, in the same kernel, with
A * (s & 65535) + (s >> 16) in plain integer code (A = 36969 and 18000); a
second launch follows 2^16 state pairs for 256 draws each (2^24 draws) and
compares the assembled [2, 4) float's bits and both states with the plain
form's.  Every count must be 0."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "se-195-project-ray-tracer_amd", "csrc")
SRC = os.path.join(HERE, "native", "gpu_rng_draw_check.hip")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CHECKED = {"s0": 1 << 32, "s1": 1 << 32, "draw": 1 << 24, "state": 1 << 24}


def test_every_stream_value_and_draw_on_the_device(tmp_path):
    exe = str(tmp_path / "gpu_rng_draw_check")
    # the product's flags (se-195-project-ray-tracer_amd/Makefile)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize",
                    "-I" + CSRC, "-o", exe, SRC], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    rows = [l.split() for l in out.stdout.strip().splitlines()]
    assert [r[0] for r in rows[:-1]] == list(CHECKED), out.stdout + out.stderr
    for name, checked, bad, first in rows[:-1]:
        assert int(checked) == CHECKED[name], (name, checked)
        assert int(bad) == 0, "%s: %s of %s differ, first at %s" % (name, bad, checked, first)
    assert out.returncode == 0 and rows[-1] == ["ok", "(0", "failures)"], out.stdout + out.stderr
