"""Times a geometry edit of a prepared smallpt scene from device memory
(SmallptScene.move, spt_scene_move_async) against the same edit from a host
array (SmallptScene.update, spt_scene_update_async), on one GPU, on
tools/scene_update_time.py's four scenes and motion: a range of 10 % of the
spheres, and all of them, displaced by up to 2 % of the scene's extent per
step.  Both scenes are prepared before anything is timed.

  (a) one call: the device time between two events around it, the host time
      until it returns, and the host clock until the stream is idle -- move
      from a device tensor of the range, update from the host array of the
      same range, alternating on two scenes of the same spheres;
  (b) one animation step on the GPU, a torch step (positions += velocities on
      the geometry tensor), the edit and one 640x480 4-spp frame:
        move:    step -> move -> frame                     (nothing waits)
        update:  step -> .cpu() -> rows -> update -> frame (the copy waits)
      a host clock around one step that ends in a synchronise, and the same
      loop with STEPS (default 20) steps enqueued back to back and one
      synchronise at the end, per step;
  (c) the frames of both scenes after the last step have the same bits.

Median of REPS (default 20) with min-max.  Writes the log to --out, default
the next profiles/rNN/scene_move.log."""
import argparse
import glob
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd"), os.path.join(ROOT, "tests"),
                os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rtamd  # noqa: E402
import _spt  # noqa: E402
import refit_check as rc  # noqa: E402
from scene_update_time import H, SPP, W, scenes, stat  # noqa: E402


def amplitude(rows):
    """2 % of the scene's extent (scene_update_time.steps' measure)."""
    cen = rows[4:, 1:4].astype(np.float64)
    return 0.02 * float((np.percentile(cen, 95, axis=0) - np.percentile(cen, 5, axis=0)).max())


class Edit:
    """Spheres [first, first + count) of one scene, animated on the device:
    the geometry tensor G (p.xyz, rad), velocities V, and the two ways of
    handing a step's G to a scene."""

    def __init__(self, rows, first, count, seed):
        self.rows, self.first, self.count = rows.copy(), first, count
        part = rows[first:first + count]
        self.G = torch.from_numpy(np.ascontiguousarray(np.concatenate([part[:, 1:4], part[:, 0:1]], 1))).cuda()
        v = np.zeros((count, 4), np.float32)
        v[:, :3] = np.random.default_rng(seed).uniform(-1, 1, (count, 3)) * amplitude(rows)
        self.V = torch.from_numpy(v).cuda()

    def step(self):
        self.V.neg_()                                        # there and back: the scene stays where it was built
        self.G.add_(self.V)

    def move(self, sc, stream=None):
        sc.move(self.G, first=self.first, stream=stream)

    def host_array(self):
        """The range as a host Sphere array with G's geometry (waits for the device)."""
        g = self.G.cpu().numpy()
        part = self.rows[self.first:self.first + self.count]
        part[:, 1:4] = g[:, :3]
        part[:, 0] = g[:, 3]
        return rc.from_raw(part)

    def update(self, sc, arr=None, stream=None):
        sc.update(self.host_array() if arr is None else arr, first=self.first, count=self.count, stream=stream)


def time_calls(call_a, call_b, st, warm, reps):
    """Per call of each, alternating: (event ms, host ms of the call, ms until the stream is idle)."""
    out = ([], [], []), ([], [], [])
    for i in range(warm + reps):
        for call, (te, th, ti) in zip((call_a, call_b), out):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            b.record(st)
            st.synchronize()
            t2 = time.perf_counter()
            if i >= warm:
                te.append(a.elapsed_time(b))
                th.append(1e3 * (t1 - t0))
                ti.append(1e3 * (t2 - t0))
    return out


def time_loop(step, st, warm, reps, steps):
    """(ms of one synchronised step, ms per step of `steps` enqueued back to back)."""
    one, many = [], []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        st.synchronize()
        if i >= warm:
            one.append(1e3 * (time.perf_counter() - t0))
    for i in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        st.synchronize()
        many.append(1e3 * (time.perf_counter() - t0) / steps)
    return one, many


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "20")))
    ap.add_argument("--steps", type=int, default=int(os.environ.get("STEPS", "20")))
    ap.add_argument("--scenes", default=None, help="comma-separated scene names (default: all four)")
    args = ap.parse_args()
    out = args.out
    if out is None:
        rounds = [int(m.group(1)) for m in (re.search(r"r(\d+)$", p) for p in glob.glob(os.path.join(ROOT, "profiles", "r*"))) if m]
        out = os.path.join(ROOT, "profiles", "r%02d" % (max(rounds, default=0) + 1), "scene_move.log")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    st = torch.cuda.current_stream()
    reps, warm = args.reps, 3
    say("scene move timing: move from a device tensor against update from the host array of the same range; "
        "median of %d (min, max); frame %dx%d %d spp; loops of %d steps" % (reps, W, H, SPP, args.steps))
    for name, S, n, cam in scenes():
        if args.scenes and name not in args.scenes.split(","):
            continue
        rows = rc.raw_rows(S, n)
        sm, su = rtamd.SmallptScene(S, n), rtamd.SmallptScene(S, n)
        t0 = time.perf_counter()
        sm.move_prepare(stream=st)
        st.synchronize()
        prep = 1e3 * (time.perf_counter() - t0)
        su.update(S, stream=st)                               # (the first update: metadata, staging)
        st.synchronize()
        fm, fu = rtamd.SmallptDeviceFrame(sm, cam, W, H), rtamd.SmallptDeviceFrame(su, cam, W, H)
        info = sm.info()
        say("%-13s %6d spheres, %s, %d binary / %d wide nodes, %d lights; move_prepare %.3f ms" % (
            name, n, info["family"], info["nodes"], info["wnodes"], info["nlights"], prep))
        tenth = max(1, n // 10)
        for label, first, count in (("10 %", 4 + (n - 4 - tenth) // 2, tenth), ("all", 0, n)):
            em, eu = Edit(rows, first, count, 11), Edit(rows, first, count, 11)
            # (a) one call
            em.step()
            eu.step()
            arr = eu.host_array()
            (me, mh, mi), (ue, uh, ui) = time_calls(lambda: em.move(sm, st), lambda: eu.update(su, arr, st), st, warm, reps)
            say("  %-4s (%6d spheres, %8d B of geometry, %8d B of records)" % (label, count, 16 * count, 44 * count))
            say("    (a) move  : device %s   host time of the call: %s   call + idle: %s" % (stat(me), stat(mh), stat(mi)))
            say("        update: device %s   host time of the call: %s   call + idle: %s" % (stat(ue), stat(uh), stat(ui)))
            say("        device time, move / update = %.2f" % (float(np.median(me)) / float(np.median(ue))))

            # (b) the animation step
            def step_move():
                em.step()
                em.move(sm, st)
                fm.render(SPP, stream=st)

            def step_update():
                eu.step()
                eu.update(su, None, st)
                fu.render(SPP, stream=st)

            tf = _spt.event_ms(lambda: fm.render(SPP, stream=st), warm, reps, st)
            m1, mk = time_loop(step_move, st, warm, reps, args.steps)
            u1, uk = time_loop(step_update, st, warm, reps, args.steps)
            say("    (b) frame alone: %s" % stat(tf))
            say("        step -> move -> frame          : one step + idle %s   back to back, per step %s" % (stat(m1), stat(mk)))
            say("        step -> .cpu() -> update -> frame: one step + idle %s   back to back, per step %s" % (stat(u1), stat(uk)))
            say("        per step back to back, move / update = %.2f" % (float(np.median(mk)) / float(np.median(uk))))
            # (c) the same scene either way
            fm.reset().render(SPP, stream=st)
            fu.reset().render(SPP, stream=st)
            same = fm.same_bits(fu) and (sm.spheres().view(np.uint32) == su.spheres().view(np.uint32)).all()
            say("    (c) same spheres and frame bits: %s" % bool(same))
        mi_, ui_ = sm.move_info(), su.update_info()
        say("  moves %d (refits %d); updates %d (refits %d, reallocations %d)" % (
            mi_["moves"], mi_["refits"], ui_["updates"], ui_["refits"], ui_["reallocations"]))
        sm.close()
        su.close()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
