"""CPU check of the sample plan's index arithmetic (csrc/spt_plan.h, plan_*):
which pixel, slot and sort key each lane of each tile's wave stands for, the
integer part of the decision and the scratch layout --
tests/native/plan_index_check.cpp, built with g++ into the test's temporary
directory, plain and once more under the address and undefined-behaviour
sanitizers (stand-alone host code).  Over 1 x 1, 7 x 9, 8 x 8, 9 x 8, 37 x 19
and 1920 x 1080: every pixel is visited exactly once, keys ascend, slot and
pixel index are (h - y - 1) * w + x and y * w + x, and lanes outside the frame
are never listed.  A GPU test would show a wrong index as a list that differs
from numpy's; this one shows where."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "se-195-project-ray-tracer_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "sanitized"])
def test_plan_index_arithmetic(tmp_path, flags):
    exe = str(tmp_path / "plan_index_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC] + flags +
                   ["-o", exe, os.path.join(HERE, "native", "plan_index_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) > 1000000    # the number of checks made
