"""Times rtq_trace_async on the camera rays of a frame against rtq_render_async
on that frame, on one GPU: 800 x 600 (4.32 M rays) and 1920 x 1080 (18.7 M
rays), reference scene, no counters; the rays once as the frame's chains
(group = 9: the pixel sums, which scenes.queue_pack turns into the frame) and
once each on its own (group = 1: a colour per ray).

The trace and the frame run the same level pass; the trace reads its root rays
from memory (24 B each) where the frame rebuilds them from the pixel's
coordinates, writes t and id per ray and three floats per chain where the frame
writes 4 B per pixel, and runs its slabs on one stream where a large frame
alternates two.  What that costs is what this tool measures.

Each measurement runs in a child process of its own (--child), so that the
frame can also be timed with another build of the library (--frame-lib, e.g.
the parent commit's librt_hip.so: RT_HIP_LIB in that child): per round one
child each for the other build's frame, this build's two traces and this
build's frame, ROUNDS (default 2) rounds, so that drift hits all of them.  A
child warms every shape up (3 untimed calls), sizes its timed window from one
untimed batch so that it lasts at least WINDOW seconds (default 0.1), then
takes REPS (default 9) timings, each one HIP-event pair around that many
back-to-back calls on one stream; medians with min-max over all of a variant's
timings.  The group = 9 child also checks that rtamd.scenes.queue_pack of its
colours is the frame the same build renders.  --size WxH restricts a run (or
one --child under a profiler) to one of the two sizes.  Prints the log, and
writes it to --out if given."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ((800, 600), (1920, 1080))
GROUPS = {"trace, group 9": 9, "trace, group 1": 1}


def child(what, reps, window, sizes):
    sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd")]
    import numpy as np
    import torch
    import rtamd
    P, n = rtamd.scenes.queue_scene()
    d_prims = torch.from_numpy(np.frombuffer(P, dtype=np.uint8).copy()).cuda()
    s = torch.cuda.current_stream().cuda_stream
    out = {}
    for w, h in sizes:
        d_frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")

        def frame():
            rtamd.check(rtamd.lib().rtq_render_async(d_prims.data_ptr(), n, d_frame.data_ptr(), w, h, 0, h, None, s))
        group = GROUPS.get(what)
        if group:
            d_rays = torch.from_numpy(rtamd.scenes.queue_camera_rays(w, h).reshape(-1, 6)).cuda()
            nr = d_rays.shape[0]
            outs = (torch.empty((nr // group, 3), dtype=torch.float32, device="cuda"),
                    torch.empty(nr, dtype=torch.float32, device="cuda"),
                    torch.empty(nr, dtype=torch.int32, device="cuda"))

            def run():
                rtamd.queue_trace_async(d_rays, d_prims, n, group=group, out=outs)
        else:
            run = frame
        for _ in range(3):
            run()
        torch.cuda.synchronize()

        def timed(calls):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                run()
            b.record()
            torch.cuda.synchronize()
            return a.elapsed_time(b) / calls
        calls = max(5, int(np.ceil(1e3 * window / timed(5))))
        ms = [timed(calls) for _ in range(reps)]
        res = {"ms": ms, "calls": calls, "rays": 9 * w * h}
        if group == 9:
            frame()
            torch.cuda.synchronize()
            px = rtamd.scenes.queue_pack(outs[0].cpu().numpy().reshape(h, w, 3))
            res["same_as_frame"] = bool((px == d_frame.cpu().numpy().view(np.uint32)).all())
        if group:
            del d_rays, outs
        out["%dx%d" % (w, h)] = res
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="also write the log to this file")
    ap.add_argument("--frame-lib", default=None, help="another build's librt_hip.so to time the frame with as well")
    ap.add_argument("--rounds", type=int, default=int(os.environ.get("ROUNDS", "2")))
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "9")))
    ap.add_argument("--window", type=float, default=float(os.environ.get("WINDOW", "0.1")),
                    help="least length of a timed window in seconds")
    ap.add_argument("--size", default=None, help="only this size, e.g. 1920x1080 (a profiler run of one child)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    sizes = tuple(s for s in SIZES if args.size in (None, "%dx%d" % s))
    if args.child:
        return child(args.child, args.reps, args.window, sizes)
    import numpy as np
    variants = [(name, None) for name in GROUPS] + [("frame", None)]
    if args.frame_lib:
        variants.insert(0, ("frame, other build", os.path.abspath(args.frame_lib)))
    got = {name: {} for name, _ in variants}
    same, calls = {}, {}
    for _ in range(args.rounds):
        for name, libpath in variants:
            env = dict(os.environ)
            env.pop("RT_HIP_LIB", None)
            if libpath:
                env["RT_HIP_LIB"] = libpath
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child",
                                name if name in GROUPS else "frame", "--reps", str(args.reps),
                                "--window", str(args.window)] + (["--size", args.size] if args.size else []), env=env,
                               stdout=subprocess.PIPE, text=True, timeout=600)
            if p.returncode != 0:                        # (a failed child: stop, start nothing more on the device)
                sys.exit("child %r failed with %d" % (name, p.returncode))
            res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
            for size, r in res.items():
                got[name].setdefault(size, []).extend(r["ms"])
                calls.setdefault(size, {})[name] = r["calls"]
                if "same_as_frame" in r:
                    same[size] = r["same_as_frame"]
    lines = ["queue trace timing: rtq_trace_async on a frame's camera rays (group 9 and group 1) against "
             "rtq_render_async on that frame; %d rounds x %d timings, each a window of at least %g s; median ms per "
             "call (min, max)" % (args.rounds, args.reps, args.window)]
    if args.frame_lib:
        lines.append("other build: %s" % args.frame_lib)
    for w, h in sizes:
        size = "%dx%d" % (w, h)
        nr = 9 * w * h
        lines.append("%s: %d rays; queue_pack(trace, group 9) == frame: %s" % (size, nr, same[size]))
        med = {}
        for name, _ in variants:
            ms = got[name][size]
            med[name] = float(np.median(ms))
            lines.append("  %-20s %8.3f (%.3f, %.3f) ms   %7.1f Mrays/s   %d calls a window"
                         % (name, med[name], min(ms), max(ms), nr / (1e3 * med[name]), calls[size][name]))
        for name in GROUPS:
            lines.append("  %s / frame = %.3f" % (name, med[name] / med["frame"]))
        if args.frame_lib:
            lines.append("  frame / frame, other build = %.3f" % (med["frame"] / med["frame, other build"]))
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
