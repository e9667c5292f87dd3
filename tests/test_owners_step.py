"""CPU check of the owners' step of a flush pass of the uncounted two-query
smallpt kernel (render_kernel's DQ branch; csrc/spt_policy.h, sq_owners*):
the straight-line form that resolves a lane's popped entries, at most two,
against the per-entry loop it replaced, over every state of one lane --
tests/native/owners_step_check.cpp, built with g++ into the test's temporary
directory.  The kernel's results are bit-exact only if the additions into a
sample's radiance, into the parked radiance and into the running average keep
the loop's order; a GPU test would show a slip as a wrong pixel somewhere,
this one shows the state."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "se-195-project-ray-tracer_amd", "csrc")


def test_owners_step_equals_the_loop(tmp_path):
    exe = str(tmp_path / "owners_step_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", "-I" + CSRC, "-o", exe,
                    os.path.join(HERE, "native", "owners_step_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) > 1000000    # the number of states compared
