"""Kernel time of each of N row bands (rtamd.dist.row_band) of the bench frame
on one GPU: the multi-GPU load balance of the row sharding."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-195-project-ray-tracer_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (before rtamd loads the library: one HIP runtime)
import rtamd  # noqa: E402
from rtamd import dist as rdist  # noqa: E402
import _spt  # noqa: E402

W, H, SPP = 1920, 1080, 64
S, n, cam = rtamd.scenes.smallpt("cornell", W, H)
frame = rtamd.SmallptDeviceFrame(rtamd.SmallptScene(S, n), cam, W, H)
for N in (2, 4, 8):
    # row bands, then interleaved 8-row groups (bench.py's default split): best of 3 per rank
    for name, window in (("band", lambda r: {"rows": rdist.row_band(r, N, H)}), ("group", lambda r: {"share": (r, N)})):
        ts = [min(_spt.event_ms(lambda: frame.render(SPP, **window(r)), 0, 3)) for r in range(N)]
        print("N=%d %s ms: %s  max/mean %.3f" % (N, name, " ".join("%.2f" % t for t in ts), max(ts) / np.mean(ts)))
