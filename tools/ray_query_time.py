"""Times ray queries (spt_scene_query_async) on one GPU: Mrays/s of the
nearest-hit and the any-hit kind on Cornell, cloud(3000) and BASELINE
configs[4]'s 10k spheres, for two batches of 2^20 rays each:

  camera : the pixel-centre rays of a 1024 x 1024 view (rtamd.scenes.camera_rays)
           -- coherent, every wave's rays side by side;
  random : tests/ray_query_ref.py's random set (origins uniform in the scene's
           box, uniform directions) -- incoherent.

The any-hit kind gets maxt = 1e20 for camera rays and half the scene's extent
for random ones.  For the two hierarchy scenes the same rays also go to the
same spheres prepared with RT_SPT_NO_BVH=1 (the global-memory full scan), the
answers are compared, and the walk / full-scan ratio is printed.

tools/_spt.py's event loop: 3 untimed calls, then REPS (default 20) timed
ones; median with min-max.  Writes the log to --out, default
profiles/r13/ray_query.log."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rtamd  # noqa: E402
import _spt  # noqa: E402
import ray_query_ref as rq  # noqa: E402
import scenes_layouts as sl  # noqa: E402

SIDE = 1024
NRAYS = SIDE * SIDE


def scenes():
    S, n = rtamd.scenes.cornell()
    yield "cornell", S, n, rtamd.scenes.cornell_camera(SIDE, SIDE)
    S, n = sl.cloud(sl.N_LEAF8)
    yield "cloud(3000)", S, n, sl.cloud_camera(SIDE, SIDE)
    S, n, cam = rtamd.scenes.smallpt("complex", SIDE, SIDE)
    yield "configs[4]", S, n, cam


def prepared(S, n, no_bvh):
    old = os.environ.pop("RT_SPT_NO_BVH", None)
    if no_bvh:
        os.environ["RT_SPT_NO_BVH"] = "1"
    try:
        return rtamd.SmallptScene(S, n)
    finally:
        os.environ.pop("RT_SPT_NO_BVH", None)
        if old is not None:
            os.environ["RT_SPT_NO_BVH"] = old


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "ray_query.log"))
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "20")))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    st = torch.cuda.current_stream()
    say("ray query timing: 2^20 rays per call, median of %d calls (min, max) in Mrays/s" % args.reps)
    for name, S, n, cam in scenes():
        p, rad = rq.geometry(S, n)
        lo, hi = rq.scene_box(p, rad)
        half = np.float32(0.5 * float((hi - lo).max()))
        batches = (("camera", rtamd.scenes.camera_rays(cam, SIDE, SIDE), np.float32(1e20)),
                   ("random", rq.random_rays(S, n, NRAYS), half))
        walk = prepared(S, n, False)
        info = walk.info()
        full = prepared(S, n, True) if info["family"] in ("GEO_BVH", "GEO_WIDE") else None
        say("%-12s %6d spheres, %s, leaf %d" % (name, n, info["family"], info["leaf_max"]))
        for bname, rays, maxt in batches:
            d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
            d_tmax = torch.full((NRAYS,), float(maxt), dtype=torch.float32, device="cuda")
            t = torch.empty(NRAYS, dtype=torch.float32, device="cuda")
            ids = torch.empty(NRAYS, dtype=torch.int32, device="cuda")
            for kind in ("nearest", "any"):
                tm = None if kind == "nearest" else d_tmax
                row = "  %-7s %-8s" % (bname, kind)
                med = {}
                answers = {}
                for label, sc in (("", walk), ("full scan", full)):
                    if sc is None:
                        continue
                    ms = _spt.event_ms(lambda: sc.query(d_rays, tm, kind=kind, out=(t, ids), stream=st), 3, args.reps, st)
                    rate = [NRAYS / (1e3 * v) for v in ms]
                    med[label] = float(np.median(rate))
                    answers[label] = (t.clone(), ids.clone())
                    row += "  %s%8.1f (%.1f, %.1f)" % (label + ": " if label else "", med[label], min(rate), max(rate))
                if full is not None:
                    same = torch.equal(answers[""][1], answers["full scan"][1]) and (
                        kind != "nearest" or torch.equal(answers[""][0].view(torch.int32), answers["full scan"][0].view(torch.int32)))
                    row += "  walk / full scan = %.1f  same answers: %s" % (med[""] / med["full scan"], same)
                if kind == "nearest":
                    row += "  hits %.1f %%" % (100.0 * float((ids >= 0).float().mean()))
                else:
                    row += "  occluded %.1f %%" % (100.0 * float((ids > 0).float().mean()))
                say(row)
        walk.close()
        if full is not None:
            full.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
