"""CPU check of smallpt's launch policy (csrc/spt_policy.h): the launch
shapes, priority words, heavy-tile tiers and packed split / nheavy words of
DESIGN.md §3's windows (256 CUs, 1920 wide), the RT_SPT_TUNE parser, the tier
clamps and the packed words' accessors -- tests/native/policy_check.cpp.
Every kernel result is bit-exact whatever the tiers are, so no GPU test
notices a wrong default; this one does."""
import os
import subprocess

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_launch_policy_table():
    subprocess.run(["make", "-s", "-C", NATIVE, "policy_check"], check=True)
    out = subprocess.run([os.path.join(NATIVE, "policy_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) > 1000       # the number of checks made
