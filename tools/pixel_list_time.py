"""Times pixel lists (spt_scene_render_pixels_async) on one GPU, Cornell and
BASELINE configs[4]'s 10k spheres at 1920 x 1080.

  (1) Every pixel listed in tile order, 64 samples each, against
      spt_scene_render_async for the same frame and samples, and against
      spt_scene_radiance_async on as many rays (sample 0's jittered camera
      rays in the list's order, 64 samples each): the same state machine
      without the two draws per sample and the pack.  The list's bits are
      compared with the frame's.  Also the list in row order.
  (2) A skewed budget: a random tenth of the pixels at 64 samples, the rest at
      4, listed in tile order -- against a uniform list of the same total
      (10 samples each).
  (3) The same skewed list with RT_SPT_PIXELS_REFILL=0: lanes claim only when
      their whole wave is out of samples, the chunk-synchronous form.  What
      refill buys is (3) / (2).

tools/_spt.py's event loop: 2 untimed calls, then REPS (default 10) timed
ones; median with min-max.  Writes the log to --out, default
profiles/r19/pixel_list_time.log."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rtamd  # noqa: E402
import _spt  # noqa: E402
from radiance_query_time import fmt, jittered  # noqa: E402

SPP, LOW, HIGH = 64, 4, 64


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "pixel_list_time.log"))
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "10")))
    ap.add_argument("--wh", default="1920x1080")
    ap.add_argument("--scenes", default="cornell,complex")
    args = ap.parse_args()
    w, h = (int(v) for v in args.wh.split("x"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    st = torch.cuda.current_stream()
    med = lambda ms: float(np.median(ms))   # noqa: E731
    say("pixel list timing: %d x %d, median of %d calls (min, max)" % (w, h, args.reps))

    def timed(run):
        return _spt.event_ms(run, 2, args.reps, st)

    for kind in args.scenes.split(","):
        S, n, cam = rtamd.scenes.smallpt(kind, w, h)
        sc = rtamd.SmallptScene(S, n)
        info = sc.info()
        say("%-8s %6d spheres, %s, leaf %d" % (kind, n, info["family"], info["leaf_max"]))
        frame, ref = rtamd.SmallptDeviceFrame(sc, cam, w, h), rtamd.SmallptDeviceFrame(sc, cam, w, h)
        # (1) every pixel, uniform
        every, _ = frame.budget_list(np.ones((h, w), np.int32))
        fr = timed(lambda: ref.render(SPP, stream=st))
        pl = timed(lambda: frame.render_pixels(every, nsamples=SPP, use_done=False, stream=st))
        # radiance on the same pixels' rays in the list's order (the order alone moves the time)
        rays, after = jittered(cam, w, h, rtamd.scenes.seeds(w, h))
        p = every.cpu().numpy().astype(np.int64)
        slot = (h - 1 - p // w) * w + p % w
        d_rays = torch.from_numpy(rays[slot]).cuda()
        d_after = torch.from_numpy(np.ascontiguousarray(after[slot]).view(np.int32)).cuda()
        out = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
        so = torch.zeros((w * h, 2), dtype=torch.int32, device="cuda")
        rd = timed(lambda: sc.radiance(d_rays, d_after, SPP, out=out, seeds_out=so, stream=st))
        say("  (1) all pixels x %d   frame %s  radiance %s  list %s" % (SPP, fmt(fr), fmt(rd), fmt(pl)))
        say("      list / radiance = %.3f (radiance's own spread: max / min = %.3f)   list / frame = %.3f   same bits as the frame: %s"
            % (med(pl) / med(rd), max(rd) / min(rd), med(pl) / med(fr), frame.same_bits(ref)))
        rows = torch.arange(w * h, dtype=torch.int32, device="cuda")
        pr = timed(lambda: frame.render_pixels(rows, nsamples=SPP, use_done=False, stream=st))
        say("      the list in row order instead of tile order %s  / tile order = %.3f" % (fmt(pr), med(pr) / med(pl)))
        del d_rays, d_after, out, so
        # (2) skewed, (3) the same without refill
        rng = np.random.default_rng(1)
        budget = np.full(w * h, LOW, np.int32)
        budget[rng.permutation(w * h)[:w * h // 10]] = HIGH
        total = int(budget.sum())
        px, take = frame.budget_list(budget.reshape(h, w))
        uni_spp = total // (w * h)
        un = timed(lambda: frame.render_pixels(every, nsamples=uni_spp, use_done=False, stream=st))
        sk = timed(lambda: frame.render_pixels(px, take, use_done=False, stream=st))
        os.environ["RT_SPT_PIXELS_REFILL"] = "0"
        try:
            nr = timed(lambda: frame.render_pixels(px, take, use_done=False, stream=st))
        finally:
            del os.environ["RT_SPT_PIXELS_REFILL"]
        say("  (2) 10 %% x %d, 90 %% x %d (%d samples; uniform x %d: %d)   uniform %s  skewed %s  skewed / uniform = %.3f"
            % (HIGH, LOW, total, uni_spp, uni_spp * w * h, fmt(un), fmt(sk), med(sk) / med(un)))
        say("  (3) the skewed list, no refill   %s  / uniform = %.3f   / refill = %.3f"
            % (fmt(nr), med(nr) / med(un), med(nr) / med(sk)))
        sc.close()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
