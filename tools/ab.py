"""A/B kernel timing of librt_hip.so builds under build_ab/<name>/ (one child
process per variant, interleaved rounds, HIP-event time on the launch stream).

    KERNEL=smallpt|whitted LIBS=a,b ROUNDS=2 REPS=5 python tools/ab.py

smallpt: Cornell 1920x1080, SPP (default 64) samples per launch (COUNT=full|rays: with counters); BAND=k/N renders
only row band k of N (rtamd.dist.row_band: the per-GPU work of an N-GPU frame).
whitted: raytracer3.0.06 scene, 1920x1080 (WH=640x480: configs[0]'s size), rows [20, H-70).
"""
import ctypes as C
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "se-195-project-ray-tracer_amd"))


def child():
    import numpy as np
    import torch
    import rtamd
    import _spt
    W, H = (int(v) for v in os.environ.get("WH", "1920x1080").split("x"))
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev)
    L = rtamd.lib()
    if os.environ.get("KERNEL", "smallpt") == "whitted":
        prims, n = rtamd.scenes.whitted_scene()
        nbytes = C.sizeof(prims)
        d_prims = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        d_prims.copy_(torch.frombuffer(bytearray(prims), dtype=torch.uint8))
        px = torch.zeros(W * H, dtype=torch.int32, device=dev)

        def run(warm=False):
            rtamd.check(L.rtw_render_async(d_prims.data_ptr(), n, px.data_ptr(), W, H, 20, H - 70, None,
                                           st.cuda_stream))
    else:
        # SCENE=c4: BASELINE configs[4] (8-wide hierarchy kernel); BAND / GROUP=k/N: a row band / the
        # interleaved share of rank k of N
        sc, frame, kw = _spt.frame_from_env()
        # COUNT=full: all four counters (the counted kernel); COUNT=rays: calls and samples only
        cmode = os.environ.get("COUNT", "")
        cm = {"counted": bool(cmode),
              "mode": rtamd.SPT_PATH_TRACING | (rtamd.SPT_COUNT_RAYS if cmode == "rays" else 0)}
        plain = os.environ.get("WARM_PLAIN")       # warm-up launches uncounted (they learn the tile order)

        def run(warm=False):
            frame.render(stream=st, **kw, **({} if (warm and plain) else cm))
    warm = int(os.environ.get("WARM", "3" if os.environ.get("SCENE") == "c4" else "1"))
    _spt.event_ms(lambda: run(warm=True), warm, 0, st)
    ts = _spt.event_ms(run, 0, int(os.environ.get("REPS", "5")), st)
    if os.environ.get("PROF"):      # block counters of a tools-only instrumented build
        names = ["iter", "shadow", "nearest", "diff", "spec", "refr", "light", "bounce", "done",
                 "wcall", "wstep", "wleaf", "wshade", "flush",   # flush: ring entries popped / passes
                 # ... and the same by what started the pass: threshold, no free slot,
                 # previous sample unfolded, emitter term, drain
                 "fl_thr", "fl_slot", "fl_ends", "fl_emit", "fl_drain",
                 # the owners' step of a flush pass: entries resolved (waves: passes that resolve one),
                 # folds of a parked sample, and per pass the lanes that resolve one entry / two
                 "ow_round", "ow_fold", "ow_one", "ow_two"]
        buf = (C.c_ulonglong * (2 * max(len(names), 64)))()   # (room for a build with more counters than names)
        L.spt_prof_read(buf)
        for b, nm in enumerate(names):
            lanes, waves = buf[2 * b], buf[2 * b + 1]
            print("  %-8s lanes %14d waves %12d lanes/wave-exec %.1f" % (nm, lanes, waves, lanes / max(waves, 1)))
    print("%s %s %s min %.3f med %.3f ms" % (os.environ.get("KERNEL", "smallpt"), os.environ.get("BAND", os.environ.get("GROUP", "")),
                                            os.environ.get("VARIANT", "?"), min(ts), float(np.median(ts))),
          flush=True)


def main():
    base = os.path.join(ROOT, "build_ab")
    libs = sorted(os.listdir(base)) if os.path.isdir(base) else []
    if os.environ.get("LIBS"):
        libs = os.environ["LIBS"].split(",")
    tree = os.path.join(ROOT, "se-195-project-ray-tracer_amd", "librt_hip.so")   # "main": the in-tree build
    variants = {name: {"RT_HIP_LIB": tree if name == "main" else os.path.join(base, name, "librt_hip.so")}
                for name in libs}
    if not variants:
        variants = {"tree": {}}
    for _ in range(int(os.environ.get("ROUNDS", "2"))):
        for name, env in variants.items():
            e = dict(os.environ, VARIANT=name, **env)
            subprocess.run([sys.executable, __file__, "child"], env=e, check=True, timeout=300)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
    else:
        main()
