"""Times the adaptive-sampling pieces on one GPU, Cornell and BASELINE
configs[4]'s 10k spheres at 1920 x 1080.

  (a) The cost of the second-moment plane: spt_scene_render_pixels_stats_async
      against spt_scene_render_pixels_async on the same list (every pixel in
      tile order, 64 samples), alternating, median of REPS (default 7) each.
  (b) One plan call (spt_frame_plan_async, three launches) on a frame in the
      middle of a refinement, against the bytes it must move at 6.3 TB/s: two
      passes over 20 B a pixel (colour, m2, done) plus 8 B per listed entry
      and padding position.
  (c) What it buys: frame.refine to an average of 64 samples a pixel (min 8,
      step 8, max 256, the tolerance found by bisection so that the mean of
      `done` lands within 5 % of 64) against the uniform 64-sample frame, both
      RMSEs taken against a 4096-sample frame of the same seeds; and the wall
      time from the first enqueue to completion of that loop eager, as one
      captured graph, and driven from the host through budget_list (torch
      computes the same error map, nonzero + argsort build the list, the host
      waits for the count every pass).

Writes the log to --out, default profiles/r22/adaptive_time.log."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd"), os.path.join(ROOT, "tools")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rtamd  # noqa: E402
import _spt  # noqa: E402

SPP, REF_SPP = 64, 4096
LOOP = dict(min_samples=8, step=8, max_samples=256, floor=1e-3)
PASSES = (LOOP["max_samples"] - LOOP["min_samples"]) // LOOP["step"] + 1
HBM = 6.3e12                                    # achievable bytes / s


def fmt(ms):
    return "%.3f ms (%.3f, %.3f)" % (float(np.median(ms)), min(ms), max(ms))


def start(frame):
    frame.m2
    frame.done
    frame.reset()
    frame.seeds.copy_(frame.seeds0)
    return frame


def host_loop(frame, tol, passes):
    """The loop the plan replaces: the error map in torch, budget_list on the
    host (which waits for the device), render_pixels(stats=True)."""
    w, h = frame.w, frame.h
    mn, mx, step, floor = LOOP["min_samples"], LOOP["max_samples"], LOOP["step"], LOOP["floor"]
    for _ in range(passes):
        c = frame.colors.view(-1, 3)
        n = frame.done
        mean2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        var = torch.clamp_min(torch.nan_to_num(frame.m2 - mean2, nan=0.0), 0.0)
        e = torch.sqrt(var / (n.float() * (mean2 + floor)))
        take = torch.where(n < mn, mn - n, torch.where((e > tol) & (n < mx), torch.clamp_max(mx - n, step), 0))
        budget = take.view(h, w).flip(0)                    # slot order to [y, x]
        pixels, t = frame.budget_list(budget)
        if pixels.numel() == 0:
            break
        frame.render_pixels(pixels, t, stats=True)


def wall(run):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22", "adaptive_time.log"))
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "7")))
    ap.add_argument("--wh", default="1920x1080")
    ap.add_argument("--scenes", default="cornell,complex")
    ap.add_argument("--ref-spp", type=int, default=REF_SPP)
    args = ap.parse_args()
    w, h = (int(v) for v in args.wh.split("x"))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        with open(args.out, "w") as f:                      # (kept up to date: a run cut short leaves what it had)
            f.write("\n".join(lines) + "\n")

    st = torch.cuda.current_stream()
    med = lambda ms: float(np.median(ms))   # noqa: E731
    say("adaptive sampling timing: %d x %d, medians of %d (min, max)" % (w, h, args.reps))
    for kind in args.scenes.split(","):
        S, n, cam = rtamd.scenes.smallpt(kind, w, h)
        sc = rtamd.SmallptScene(S, n)
        info = sc.info()
        say("%-8s %6d spheres, %s, leaf %d" % (kind, n, info["family"], info["leaf_max"]))
        frame = rtamd.SmallptDeviceFrame(sc, cam, w, h)
        every, _ = frame.budget_list(np.ones((h, w), np.int32))
        # (a) alternating: plain, stats, plain, stats ...
        start(frame)
        plain, stats = [], []
        for f in (False, True):                             # untimed
            frame.render_pixels(every, nsamples=SPP, use_done=False, stream=st, stats=f)
        for _ in range(args.reps):
            plain += _spt.event_ms(lambda: frame.render_pixels(every, nsamples=SPP, use_done=False, stream=st), 0, 1, st)
            stats += _spt.event_ms(lambda: frame.render_pixels(every, nsamples=SPP, use_done=False, stream=st, stats=True),
                                   0, 1, st)
        say("  (a) all pixels x %d   plain %s   stats %s   stats / plain = %.4f" % (SPP, fmt(plain), fmt(stats),
                                                                                  med(stats) / med(plain)))
        # (c) the tolerance for a mean of 64: bisection on log(tol)
        lo, hi = 1e-3, 1.0
        tol, mean = None, 0.0
        for _ in range(14):
            tol = float(np.sqrt(lo * hi))
            start(frame).refine(PASSES, tol=tol, **LOOP)
            mean = float(frame.done.float().mean())
            if abs(mean - SPP) <= 0.02 * SPP:
                break
            lo, hi = (tol, hi) if mean > SPP else (lo, tol)
        listed_last = int(frame.plan_totals[0])
        adaptive = frame.colors.clone()
        hist = torch.bincount(frame.done, minlength=LOOP["max_samples"] + 1).cpu().numpy()
        say("  (c) refine(%d passes, tol %.5f, min %d, step %d, max %d): mean of done %.2f, at min %.1f %%, at max %.1f %%, "
            "last plan listed %d" % (PASSES, tol, LOOP["min_samples"], LOOP["step"], LOOP["max_samples"], mean,
                                     100.0 * hist[LOOP["min_samples"]] / (w * h), 100.0 * hist[LOOP["max_samples"]] / (w * h),
                                     listed_last))
        # (b) the plan on a frame in the middle of that refinement
        start(frame).refine(PASSES // 4, tol=tol, **LOOP)
        pl = _spt.event_ms(lambda: frame.plan(tol=tol, stream=st, **LOOP), 3, max(args.reps, 20), st)
        listed = int(frame.plan_totals[0])
        nbytes = 2 * 20 * w * h + 8 * w * h
        floor_ms = nbytes / HBM * 1e3
        say("  (b) one plan call (%d of %d pixels listed) %s   bytes %.1f MB -> %.4f ms at 6.3 TB/s   measured / floor = %.1f"
            % (listed, w * h, fmt(pl), nbytes / 1e6, floor_ms, med(pl) / floor_ms))
        # (c) RMSE against the long frame
        ref = rtamd.SmallptDeviceFrame(sc, cam, w, h)
        ref.reset().render(args.ref_spp)
        uni = rtamd.SmallptDeviceFrame(sc, cam, w, h)
        uni.reset().render(SPP)
        torch.cuda.synchronize()

        def rmse(a, clamp):
            a, b = (a, ref.colors) if not clamp else (a.clamp(0, 1), ref.colors.clamp(0, 1))
            return float(torch.sqrt(torch.mean((a.double() - b.double()) ** 2)))
        say("      RMSE against %d samples: uniform x %d  %.5f (clamped to [0, 1]: %.5f)   adaptive, mean %.2f  %.5f (%.5f)   "
            "adaptive / uniform = %.3f (%.3f)" % (args.ref_spp, SPP, rmse(uni.colors, False), rmse(uni.colors, True), mean,
                                                   rmse(adaptive, False), rmse(adaptive, True),
                                                   rmse(adaptive, False) / rmse(uni.colors, False),
                                                   rmse(adaptive, True) / rmse(uni.colors, True)))
        del ref
        # (c) wall time of the loop: eager, one graph, the host path
        uniform = _spt.event_ms(lambda: uni.render(SPP, stream=st), 1, args.reps, st)
        eager = [wall(lambda: start(frame).refine(PASSES, tol=tol, **LOOP)) for _ in range(args.reps)]
        done_eager = frame.done.clone()
        start(frame)
        frame.plan(tol=tol, **LOOP)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            frame.refine(PASSES, tol=tol, **LOOP)

        def replay():
            start(frame)
            g.replay()
        replay()
        graph = [wall(replay) for _ in range(args.reps)]
        same = bool(torch.equal(frame.done, done_eager))
        host = [wall(lambda: host_loop(start(frame), tol, PASSES)) for _ in range(args.reps)]
        same_host = bool(torch.equal(frame.done, done_eager))
        say("      wall, first enqueue to completion (reset included): eager %s   one graph %s (same done: %s)   "
            "host loop through budget_list %s (same done: %s)   uniform x %d frame, events: %s"
            % (fmt(eager), fmt(graph), same, fmt(host), same_host, SPP, fmt(uniform)))
        del g
        sc.close()


if __name__ == "__main__":
    main()
