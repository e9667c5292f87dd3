"""CPU check of smallpt's kernel variants and LDS layout (csrc/spt_layout.h):
over every variant, block shape and a sweep of scene sizes the regions of
render_kernel's dynamic LDS are disjoint, aligned and inside the bytes
launch() asks for; DESIGN.md §3's per-family totals; and no launch asks for
more LDS than a CU has -- tests/native/layout_check.cpp.  The host and the
kernel take the layout from that one header, so a GPU test sees a wrong
offset only as a fault; this one sees it as a number."""
import os
import subprocess

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")


def test_lds_layout_sweep():
    subprocess.run(["make", "-s", "-C", NATIVE, "layout_check"], check=True)
    out = subprocess.run([os.path.join(NATIVE, "layout_check")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) > 10000      # the number of checks made
