"""CPU check of the pixel-list kernel's claim arithmetic (csrc/spt_pixels.h,
pix_*): which list entry each wanting lane of a wave takes, and the wave's
cursor after the step -- tests/native/pixel_claim_check.cpp, built with g++
into the test's temporary directory, plain and once more under the address
and undefined-behaviour sanitizers (stand-alone host code).  Over random need
masks, list lengths around the wave size and several grid shapes: every entry
is handed out exactly once over all waves, in increasing order within a wave,
and a wave that was told "exhausted" is never handed an entry again.  A GPU
test would show a wrong claim as a pixel rendered twice or never; this one
shows where."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "se-195-project-ray-tracer_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_pixel_claim_arithmetic(tmp_path, flags):
    exe = str(tmp_path / "pixel_claim_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC] + flags +
                   ["-o", exe, os.path.join(HERE, "native", "pixel_claim_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) > 100000     # the number of checks made
