"""Times the level-pass tracers' ray queries (rtp_query_async) on one GPU:
Mrays/s of NEAREST (one and two rays per lane, RT_PRIMS_QUERY_RAYS), SHADOW
and OCCLUDER for both tracers, on their reference scenes (17 primitives) and
on tests/prims_query_ref.py's 64-primitive scene, for two batches of 2^20 rays:

  fan    : the centre rays of a 1024 x 1024 view from the tracers' camera
           point (0, 0.25, -7) through their view plane -- coherent, every
           wave's rays side by side;
  random : origins uniform in the scenes' box, uniform directions --
           incoherent.

Shadow lengths are uniform in [0.5, 40).  A call on the small scenes takes
less time than the host needs to enqueue it, so each variant's CALLS (default
100) back-to-back calls are captured into one graph, and a timing is one
HIP-event pair around one replay, after 2 untimed replays; REPS (default 9)
timings per variant, the two NEAREST variants alternating (1, 2, 1, 2, ...)
so that drift hits both; median with min-max.  The two variants' answers are
compared.  Writes the log to --out, default profiles/r16/prims_query.log."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "se-195-project-ray-tracer_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import rtamd  # noqa: E402
import prims_query_ref as Q  # noqa: E402

SIDE = 1024
NRAYS = SIDE * SIDE
F = np.float32


def fan_rays():
    """Pixel-centre directions of the references' view (x in [-3, 3], y in
    [2.25, -2.25] at z = 0) from (0, 0.25, -7), normalised in float32."""
    x = (F(-3) + (np.arange(SIDE, dtype=F) + F(0.5)) * F(6.0 / SIDE))[None, :].repeat(SIDE, 0)
    y = (F(2.25) - (np.arange(SIDE, dtype=F) + F(0.5)) * F(4.5 / SIDE))[:, None].repeat(SIDE, 1)
    d = np.stack([x, y - F(0.25), np.full_like(x, 7)], -1).reshape(-1, 3)
    d *= (F(1) / np.sqrt((d * d).sum(1, dtype=F)))[:, None]
    o = np.tile(np.array([0, 0.25, -7], F), (NRAYS, 1))
    return np.concatenate([o, d], 1).astype(F)


def scenes(tracer):
    P, n = rtamd.scenes.whitted_scene() if tracer == "whitted" else rtamd.scenes.queue_scene()
    yield "reference", P, n
    big = Q.big_scene(tracer)
    yield "64 primitives", big.prims(tracer), big.n


def graph_of(run, calls):
    """`calls` back-to-back run()s (on the current stream) as one graph."""
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            run()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    return g


def replay_ms(g, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "prims_query.log"))
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "9")))
    ap.add_argument("--calls", type=int, default=int(os.environ.get("CALLS", "100")))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(16)
    batches = (("fan", fan_rays()), ("random", Q.random_rays(rng, NRAYS, (-9, -6, -8), (9, 8, 30))))
    d_lens = torch.from_numpy(rng.uniform(0.5, 40.0, NRAYS).astype(F)).cuda()
    t = torch.empty(NRAYS, dtype=torch.float32, device="cuda")
    ids = torch.empty(NRAYS, dtype=torch.int32, device="cuda")
    res = torch.empty(NRAYS, dtype=torch.int32, device="cuda")
    say("level-pass ray query timing: 2^20 rays per call, %d calls per graph replay, median of %d replays (min, max) "
        "in Mrays/s" % (args.calls, args.reps))
    ratios, disjoint = [], {1: 0, 2: 0}

    def rate(ms):
        r = [NRAYS / (1e3 * v) for v in ms]
        return float(np.median(r)), min(r), max(r)

    for tracer in ("whitted", "queue"):
        for sname, P, n in scenes(tracer):
            ps = rtamd.PrimScene(P, n, tracer=tracer)
            say("%-8s %-14s %2d primitives" % (tracer, sname, n))
            for bname, rays in batches:
                d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()

                def nearest(k):
                    os.environ["RT_PRIMS_QUERY_RAYS"] = str(k)           # (read at the call: fixed at capture)
                    ps.query(d_rays, kind="nearest", out=(t, ids, res))
                answers, graphs = {}, {}
                for k in (1, 2):
                    graphs[k] = graph_of(lambda: nearest(k), args.calls)
                    answers[k] = (t.clone(), ids.clone(), res.clone())
                os.environ.pop("RT_PRIMS_QUERY_RAYS", None)
                same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(answers[1], answers[2]))
                ms = {1: [], 2: []}
                for _ in range(args.reps):
                    for k in (1, 2):
                        ms[k].append(replay_ms(graphs[k], args.calls))
                hits = 100.0 * float((ids >= 0).float().mean())
                del graphs
                r1, r2 = rate(ms[1]), rate(ms[2])
                if r2[1] > r1[2]:
                    disjoint[2] += 1
                elif r1[1] > r2[2]:
                    disjoint[1] += 1
                ratios.append(r2[0] / r1[0])
                say("  %-7s nearest   R=1 %8.1f (%.1f, %.1f)  R=2 %8.1f (%.1f, %.1f)  R=2 / R=1 = %.3f  same answers: %s"
                    "  hits %.1f %%" % ((bname,) + r1 + r2 + (r2[0] / r1[0], same, hits)))
                for kind in ("shadow", "occluder"):
                    g = graph_of(lambda: ps.query(d_rays, d_lens, kind=kind, out=(None, ids, None)), args.calls)
                    r = rate([replay_ms(g, args.calls) for _ in range(args.reps)])
                    del g
                    say("  %-7s %-9s     %8.1f (%.1f, %.1f)  occluded %.1f %%" % (
                        (bname, kind) + r + (100.0 * float(((ids > 0) if kind == "shadow" else (ids >= 0)).float().mean()),)))
            ps.close()
    geo = float(np.exp(np.mean(np.log(ratios))))
    say("NEAREST, two rays per lane over one: geometric mean %.3f over %d rows (min %.3f, max %.3f); rows whose "
        "min-max ranges do not overlap: %d in favour of R=2, %d in favour of R=1"
        % (geo, len(ratios), min(ratios), max(ratios), disjoint[2], disjoint[1]))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
