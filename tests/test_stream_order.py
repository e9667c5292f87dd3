"""CPU check of csrc/spt_streams.h, the bookkeeping that orders one prepared
smallpt scene's launches across streams (spt_sched.h's work-counter ring and
learnt order): random launch sequences on 1 to 12 streams, with captures and
releases, against a model that tracks which launches every stream is ordered
after -- tests/native/stream_order_check.cpp, built with g++ into the test's
temporary directory.  tests/test_gpu_smallpt_streams.py runs the two
sequences this guards on the device; this one shows the state at which the
bookkeeping would let a write through under a reader."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "se-195-project-ray-tracer_amd", "csrc")


def test_stream_order_bookkeeping(tmp_path):
    exe = str(tmp_path / "stream_order_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I" + CSRC, "-o", exe,
                    os.path.join(HERE, "native", "stream_order_check.cpp")], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert int(out.stdout.split()[-1]) > 400000     # the number of steps checked
