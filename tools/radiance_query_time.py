"""Times radiance queries (spt_scene_radiance_async) on one GPU against the
renderer, the yardstick: the same estimator on the same rays, reached through
the tiled frame kernels instead of one ray per lane.

  (a) Cornell, the 1024 x 768 jittered camera rays of sample 0 (the jitter
      drawn on the host from the frame's initial seeds), one sample per ray,
      against spt_scene_render_async for that frame at nsamples = 1; the bits
      (colours in the flipped slots, and the states) are compared.
  (b) The same rays at nsamples = 64 against the 64-sample frame.  (The frame
      re-draws its jitter per sample, the query keeps its rays: equal work per
      sample on average, not equal bits.)
  (c) cloud(3000) and BASELINE configs[4]'s 10k spheres: the camera rays, and
      tests/ray_query_ref.py's random rays (as many), one sample, in
      Mrays/s, with the frame's time for the camera rays.

tools/_spt.py's event loop: 3 untimed calls, then REPS (default 20) timed
ones; median with min-max.  Writes the log to --out, default
profiles/r14/radiance_query.log."""
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

W, H = 1024, 768
NRAYS = W * H


def jittered(cam, w, h, seeds):
    """(rays in slot order, states after the two jitter draws) of sample 0."""
    i = np.arange(w * h)
    x, y = i % w, h - 1 - i // w                                # slot i = (h - y - 1) * w + x
    s = seeds.reshape(-1, 2)
    v1, s0, s1 = rtamd.scenes.mwc_draw(s[:, 0], s[:, 1])
    v2, s0, s1 = rtamd.scenes.mwc_draw(s0, s1)
    rays = rtamd.scenes.camera_rays(cam, w, h, x, y, v1 - np.float32(0.5), v2 - np.float32(0.5))
    return rays, np.stack([s0, s1], axis=1)


def fmt(ms):
    return "%8.3f ms (%.3f, %.3f)" % (float(np.median(ms)), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "radiance_query.log"))
    ap.add_argument("--reps", type=int, default=int(os.environ.get("REPS", "20")))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    st = torch.cuda.current_stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
    say("radiance query timing: %d x %d = %d rays per call, median of %d calls (min, max)" % (W, H, NRAYS, args.reps))

    def case(name, S, n, cam, spps, random_too):
        sc = rtamd.SmallptScene(S, n)
        info = sc.info()
        say("%-12s %6d spheres, %s, leaf %d" % (name, n, info["family"], info["leaf_max"]))
        frame = rtamd.SmallptDeviceFrame(sc, cam, W, H)
        rays, after = jittered(cam, W, H, rtamd.scenes.seeds(W, H))
        d_rays, d_after = dev(rays), dev(after.view(np.int32))
        out = torch.zeros((NRAYS, 3), dtype=torch.float32, device="cuda")
        so = torch.zeros((NRAYS, 2), dtype=torch.int32, device="cuda")
        for spp in spps:
            fr = _spt.event_ms(lambda: frame.render(spp, stream=st), 3, args.reps, st)
            qr = _spt.event_ms(lambda: sc.radiance(d_rays, d_after, spp, out=out, seeds_out=so, stream=st), 3, args.reps, st)
            row = "  camera  %2d spp  frame %s  query %s  query / frame = %.2f  %.1f Mrays/s" % (
                spp, fmt(fr), fmt(qr), float(np.median(qr)) / float(np.median(fr)), spp * NRAYS / (1e3 * float(np.median(qr))))
            if spp == 1:
                same = (torch.equal(out.view(-1).view(torch.int32), frame.colors.view(torch.int32))
                        and torch.equal(so.view(-1), frame.seeds))
                row += "  same bits as the frame: %s" % same
            say(row)
        if random_too:
            rr_ = dev(rq.random_rays(S, n, NRAYS))
            qr = _spt.event_ms(lambda: sc.radiance(rr_, d_after, 1, out=out, seeds_out=so, stream=st), 3, args.reps, st)
            say("  random   1 spp  query %s  %.1f Mrays/s  nonzero %.1f %%" % (
                fmt(qr), NRAYS / (1e3 * float(np.median(qr))), 100.0 * float((out != 0).any(dim=1).float().mean())))
        sc.close()

    S, n = rtamd.scenes.cornell()
    case("cornell", S, n, rtamd.scenes.cornell_camera(W, H), (1, 64), False)
    S, n = sl.cloud(sl.N_LEAF8)
    case("cloud(3000)", S, n, sl.cloud_camera(W, H), (1,), True)
    S, n, cam = rtamd.scenes.smallpt("complex", W, H)
    case("configs[4]", S, n, cam, (1,), True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
