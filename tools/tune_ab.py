"""A/B of launch tunings (RT_SPT_TUNE strings) on BASELINE configs[4]
(10k-sphere scene, 1920x1080, 64 spp from the initial state) in one process:
per tuning, warm frames (the first records the tile costs, the learnt order
applies from the next), then REPS timed frames (HIP events, median and min),
each frame checked against the reference-core golden hashes.  GROUP=k/N
times an interleaved share instead of the full frame; COUNTED=1 times the
full-counter kernels (all four reference counters).

    TUNES="-;coop=512;walk=8/16/32" REPS=5 python tools/tune_ab.py   ("-": the defaults)
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before rtamd loads the library: one HIP runtime)
import rtamd  # noqa: E402
import oracle_lib  # noqa: E402
import _spt  # noqa: E402

W, H, SPP = int(os.environ.get("W", 1920)), int(os.environ.get("H", 1080)), int(os.environ.get("SPP", 64))
REPS, WARM = int(os.environ.get("REPS", 5)), int(os.environ.get("WARM", 3))
TUNES = os.environ.get("TUNES", "-").split(";")
GROUP = os.environ.get("GROUP")
COUNTED = os.environ.get("COUNTED") == "1"
spheres, n, cam = rtamd.scenes.smallpt("complex", W, H)
gold = None
if (W, H, SPP) == (1920, 1080, 64) and not GROUP:
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "known_answers.json")))["smallpt"][
        "1920x1080_64spp_complex10k"]
ref = None
for tune in TUNES:
    os.environ["RT_SPT_TUNE"] = "" if tune == "-" else tune
    sc = rtamd.SmallptScene(spheres, n)              # (a fresh scene: its own learnt order)
    frame = rtamd.SmallptDeviceFrame(sc, cam, W, H)
    kw = {"share": tuple(int(v) for v in GROUP.split("/"))} if GROUP else {}

    def run():
        frame.render(SPP, counted=COUNTED, **kw)

    _spt.event_ms(run, WARM, 0)
    ts = []
    ok = True
    for _ in range(REPS):
        ts += _spt.event_ms(run, 0, 1)
        h = tuple(oracle_lib.fnv1a64(a) for a in frame.host())      # colours, seeds, pixels
        if gold is not None:
            ok = ok and h == (gold["colors"], gold["seeds"], gold["pixels"])
        else:
            ref = ref or h
            ok = ok and h == ref
    print("tune=%-40s median %.3f ms  min %.3f ms  %s  [%s]" % (
        tune, float(np.median(ts)), min(ts), "EXACT" if ok else "MISMATCH", " ".join("%.2f" % t for t in ts)),
        flush=True)
    sc.close()
