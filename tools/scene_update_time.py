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
      teach a hierarchy scene its dispatch order);
  (d) regroup: spt_scene_regroup_async + stream idle on that refitted scene,
      the host time of the call, the first regroup on its own, and the same
      frame on the regrouped tree, placed between (c)'s two;
  (e) the regroup with the LDS tier given subtrees of at most 0 (every tree
      level sorted by passes of its own), 64, 256, 1024 and 4096 entries
      (RT_SPT_REGROUP_LDS, a fresh scene of the final array) against (d).

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
LDS_SIZES = (0, 64, 256, 1024, 4096)    # RT_SPT_REGROUP_LDS values of (e); 0: the per-level form


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


def time_regroups(sc, st, warm, reps):
    """(first call + idle, later calls + idle, their host times): the work of
    a regroup does not depend on how the entries lie, so repeating it on the
    regrouped tree times the same launches."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sc.regroup(stream=st)
    st.synchronize()
    first = 1e3 * (time.perf_counter() - t0)
    tg, th = [], []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.regroup(stream=st)
        t1 = time.perf_counter()
        st.synchronize()
        t2 = time.perf_counter()
        if i >= warm:
            tg.append(1e3 * (t2 - t0))
            th.append(1e3 * (t1 - t0))
    return first, tg, th


def regroup_lines(say, sc, fa, fb, last, n, st, warm, reps, rebuild, refit_frame, fresh_frame):
    """(d) a regroup of the tree refitted through all the steps, and the frame
    on it, between the refit-only frame and the fresh tree's; (e) the same
    regroup with every level sorted by passes of its own (no LDS tier)."""
    first, tg, th = time_regroups(sc, st, warm, reps)
    ri = sc.regroup_info()
    tq = _spt.event_ms(lambda: fa.render(SPP, stream=st), warm, reps, st)
    same = fa.same_bits(fb)
    say("  (d) regroup + idle          : %s   host time of the call: %s   first regroup: %.3f ms" % (
        stat(tg), stat(th), first))
    say("      %d tree levels, %d by global passes, %d regroup bytes; (a) / (d) = %.1f" % (
        ri["levels"], ri["global_levels"], ri["bytes"], rebuild / float(np.median(tg))))
    q = float(np.median(tq))
    gap = refit_frame - fresh_frame
    say("      frame, regrouped tree   : %s   refit-only %.3f, fresh %.3f: %s of the gap closed   same bits: %s" % (
        stat(tq), refit_frame, fresh_frame, "%.0f %%" % (100 * (refit_frame - q) / gap) if gap > 0 else "n/a", same))
    for sub_max in LDS_SIZES:
        os.environ["RT_SPT_REGROUP_LDS"] = str(sub_max)
        try:
            flat = rtamd.SmallptScene(last, n)
            first0, tg0, th0 = time_regroups(flat, st, warm, reps)
        finally:
            del os.environ["RT_SPT_REGROUP_LDS"]
        ri0 = flat.regroup_info()
        say("  (e) LDS tier up to %4d + idle: %s   host time of the call: %s   %d global levels   (e) / (d) = %.2f" % (
            sub_max, stat(tg0), stat(th0), ri0["global_levels"], float(np.median(tg0)) / float(np.median(tg))))
        flat.close()


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
        if info["nodes"]:
            regroup_lines(say, sc, fa, fb, arrays[-1], n, st, warm, reps, float(np.median(ta)), float(np.median(tr)),
                          float(np.median(tf)))
        sc.close()
        fresh.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
