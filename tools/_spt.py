"""What the smallpt timing tools share: the frame their environment variables
describe, and the HIP-event timing loop."""
import os

import torch
import rtamd
from rtamd import dist as rdist


def frame_from_env(kind=None, wh=None, spp=64):
    """The scene, SmallptDeviceFrame and launch keywords that SCENE (c4:
    BASELINE configs[4]'s 10k spheres, else Cornell), WH (default 1920x1080),
    SPP (default `spp`), BAND=k/N (row band k of N: rtamd.dist.row_band) and
    GROUP=k/N (the interleaved share of rank k of N, which wins over BAND)
    describe: frame.render(**kw) is the launch.  A tool with one scene or
    one size passes `kind` / `wh`, and the variable is not read."""
    w, h = (int(v) for v in (wh or os.environ.get("WH", "1920x1080")).split("x"))
    kind = kind or ("complex" if os.environ.get("SCENE") == "c4" else "cornell")
    spheres, n, cam = rtamd.scenes.smallpt(kind, w, h)
    scene = rtamd.SmallptScene(spheres, n)
    kw = {"nsamples": int(os.environ.get("SPP", spp))}
    if os.environ.get("GROUP"):
        kw["share"] = tuple(int(v) for v in os.environ["GROUP"].split("/"))
    elif os.environ.get("BAND"):
        k, N = (int(v) for v in os.environ["BAND"].split("/"))
        kw["rows"] = rdist.row_band(k, N, h)
    return scene, rtamd.SmallptDeviceFrame(scene, cam, w, h), kw


def event_ms(run, warm, reps, stream=None):
    """`warm` untimed run() calls, then `reps` timed ones, each between a HIP
    event pair on `stream` (default: the current one) and synchronised: the
    list of ms."""
    stream = stream or torch.cuda.current_stream()
    for _ in range(warm):
        run()
    if warm:
        torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        run()
        b.record(stream)
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts
