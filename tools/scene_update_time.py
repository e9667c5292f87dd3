"""Times an edit of a prepared smallpt scene on one GPU, two ways, on four
scenes (n256, cloud(3000), BASELINE configs[4]'s 10k spheres, cloud(56000)):
10 % of the spheres move at every step.

  (a) rebuild: spt_scene_destroy + spt_scene_create of the edited array, until
      the device is idle (what spt_multi_set_scene does per band);
  (b) update:  spt_scene_update_async + stream idle, and separately the host
      time until the call returns.  The scene's first update (which builds the
      refit's metadata) is reported on its own, not among the repetitions;
  (c) one 640x480 4-spp frame on the scene refitted through all those steps
      against the same frame on a fresh scene of the same final array
      (tools/_spt.py's event loop; both after three warming launches, which
      teach a hierarchy scene its dispatch order).

(a) and (b) are host clocks around work that ends in a synchronise; median of
REPS (default 20) with min-max.  Writes the log to --out, default the next
profiles/rNN/scene_update.log."""
import argparse
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rtamd  # noqa: E402
import _spt  # noqa: E402
import refit_check as rc  # noqa: E402
import scenes_layouts as sl  # noqa: E402

W, H, SPP = 640, 480, 4


def scenes():
    S, n = sl.n256()
    yield "n256", S, n, sl.small_camera(W, H)
    S, n = sl.cloud(sl.N_LEAF8)
    yield "cloud(3000)", S, n, sl.cloud_camera(W, H)
    S, n, cam = rtamd.scenes.smallpt("complex", W, H)
    yield "configs[4]", S, n, cam
    S, n = sl.cloud(sl.N_NOWIDE)
    yield "cloud(56000)", S, n, sl.cloud_camera(W, H)


def steps(rows, count):
    """`count` arrays: at each step a fresh tenth of the spheres (never the
    first four: ground and lights) moves by up to 2 % of the scene's extent."""
    rng = np.random.default_rng(7)
    n = len(rows)
    cen = rows[4:, 1:4].astype(np.float64)
    amp = 0.02 * float((np.percentile(cen, 95, axis=0) - np.percentile(cen, 5, axis=0)).max())
    out, cur = [], rows.copy()
    for _ in range(count):
        pick = 4 + rng.choice(n - 4, n // 10, replace=False)
        cur = cur.copy()
        cur[pick, 1:4] += rng.uniform(-amp, amp, (len(pick), 3)).astype(np.float32)
        out.append(rc.from_raw(cur))
    return out


def stat(ts):
    return "%.3f ms (min %.3f, max %.3f)" % (float(np.median(ts)), min(ts), max(ts))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "20")))
    args = ap.parse_args()
    out = args.out
    if out is None:
        rounds = [int(m.group(1)) for m in (re.search(r"r(\d+)$", p) for p in glob.glob(os.path.join(ROOT, "profiles", "r*"))) if m]
        out = os.path.join(ROOT, "profiles", "r%02d" % (max(rounds, default=0) + 1), "scene_update.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    st = torch.cuda.current_stream()
    reps, warm = args.reps, 3
    say("scene update timing: %d%% of the spheres move per step; median of %d (min, max); frame %dx%d %d spp" % (
        10, reps, W, H, SPP))
    for name, S, n, cam in scenes():
        arrays = steps(rc.raw_rows(S, n), warm + reps)
        # (a) destroy + create + idle
        sc = rtamd.SmallptScene(S, n)
        info = sc.info()
        ta = []
        for i, arr in enumerate(arrays):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.close()
            sc = rtamd.SmallptScene(arr, n)
            torch.cuda.synchronize()
            if i >= warm:
                ta.append(1e3 * (time.perf_counter() - t0))
        sc.close()
        # (b) update + idle, and the host time of the call
        sc = rtamd.SmallptScene(S, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.update(S, stream=st)
        st.synchronize()
        first = 1e3 * (time.perf_counter() - t0)
        tb, th = [], []
        for i, arr in enumerate(arrays):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sc.update(arr, stream=st)
            t1 = time.perf_counter()
            st.synchronize()
            t2 = time.perf_counter()
            if i >= warm:
                tb.append(1e3 * (t2 - t0))
                th.append(1e3 * (t1 - t0))
        ui = sc.update_info()
        # (c) a frame on the refitted tree against a fresh tree of the same spheres
        fresh = rtamd.SmallptScene(arrays[-1], n)
        fa, fb = rtamd.SmallptDeviceFrame(sc, cam, W, H), rtamd.SmallptDeviceFrame(fresh, cam, W, H)
        tr = _spt.event_ms(lambda: fa.render(SPP, stream=st), warm, reps, st)
        tf = _spt.event_ms(lambda: fb.render(SPP, stream=st), warm, reps, st)
        same = fa.same_bits(fb)
        say("%-13s %6d spheres, %s, leaf %d, %d binary / %d wide nodes, %d metadata bytes" % (
            name, n, info["family"], info["leaf_max"], info["nodes"], info["wnodes"], ui["metadata_bytes"]))
        say("  (a) destroy + create + idle : %s" % stat(ta))
        say("  (b) update + idle           : %s   host time of the call: %s   first update: %.3f ms" % (
            stat(tb), stat(th), first))
        say("      (a) / (b) = %.1f; refits %d, reallocations %d" % (
            float(np.median(ta)) / float(np.median(tb)), ui["refits"], ui["reallocations"]))
        say("  (c) frame, refitted tree    : %s   fresh tree: %s   ratio %.3f   same bits: %s" % (
            stat(tr), stat(tf), float(np.median(tr)) / float(np.median(tf)), same))
        sc.close()
        fresh.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
