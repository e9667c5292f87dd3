"""One prepared scene's frames in flight on two streams stay exact.

A hierarchy scene keeps mutable device state between launches -- the ring of
work counters its persistent waves fetch from, and the learnt dispatch order
of its tile groups (csrc/spt_sched.h) -- and include/rt_hip.h lets one host
thread issue its launches on any streams.  Every test here runs on one GPU
with one host thread and two streams, with no host synchronisation between
the launches that are meant to overlap, and compares every plane with the CPU
oracle, bit for bit.

The long launch "A" is cloud(3000)'s 96 x 64 frame (96 tiles, the 8-wide
family) with RT_SPT_TUNE=blocks=1 around that launch only: one block of 16
resident waves on one CU, the rest of the device free for stream B.  A is
always the second progressive pass in place (FIRST samples, a synchronise,
then NA more with seeds_in = frame.seeds): a tile handed out twice changes
its colours and seeds, a tile never handed out keeps the first pass's.

  1. ring wrap      64 (and 130) one-block launches on B while A holds its
                    work-counter entry: the ring comes back to A's entry.
  2. order rewrite  key K1 learnt and in use by A; B learns K2 (same frame and
                    window, one sample -- or another camera) and uploads its
                    order into the buffer A dispatches from.
  3. the same with the full counters (the scene's second order object).
  4. control        query, radiance and render_pixels on B while A runs (they
                    take no scene state), and a Cornell frame (full scan: no
                    order, no ring) on two streams at once.
  5. the level-pass tracers (Whitted and queue) alternating on two streams:
                    they share one arena.

Tests 1-3 and the first of 4 assert that they overlapped: an event recorded after A is still
pending when B's whole sequence has completed.  A test whose launches did not
overlap fails; it does not skip.

Sizing of A (MI355X, HIP events, median of 5, each sequence alone; ms):
  A, one block, order learnt (tests 2, 3: every tile then runs cooperatively,
  eight lanes per pixel)         128 spp 273   256 spp 541   512 spp 1080
                                 (full counters: 287 / 568 / 1131)
  A, one block, the first launch of its key (tests 1, 4: no order yet)
                                 256 spp 207, from one timeline of test 1
                                 (so about 414 at 512 spp; not timed alone)
  B, 64 / 130 one-block launches                 15.2 / 30.9
  B, K2 with one sample, two launches            0.75  (full counters 5.5)
  B, K2 with the sky camera, two launches        256 spp 6.5   512 spp 12.9
                                                 (full counters 6.9 / 13.7)
NA is the smallest power of two at which A takes at least 10 times the
longest B sequence: 130 launches against the unlearnt A give 6.7 at 256 spp
and 13.4 at 512; every other pair is above 80.

Against the library as it was before the streams were ordered
(spt_streams.h), this file, one run: all four cases of tests 2 and 3 failed,
each with 256 of A's 6144 pixels wrong (one tile group: rendered twice or
not at all); tests 1, 4 and 5 passed -- A came out exact under both ring
wraps although the overlap held (the 64th launch was queued 14 ms into A).
The entry is zeroed by another kernel, and a running kernel need not see
another's stores to memory it holds in its own cache; so the wrap is a hazard
that one run did not show, not a reading shown wrong.  Earlier drafts of
this file failed the same way (three of the four order cases each time).
"""
import ctypes as C
import os

import numpy as np
import pytest

import lit_scenes as L
import pixel_list_ref as plr
import radiance_ref as rr
import ray_query_ref as rq
import scenes_layouts as sl
from spt_check import assert_same

pytestmark = pytest.mark.gpu

HOOKS = ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE", "RT_SPT_SCHED", "RT_SPT_DUAL",
         "RT_SPT_QUERY_BLOCKS")
N_SPHERES = sl.N_LEAF8                          # cloud3000: the smallest scene of the 8-wide family
W, H = 96, 64                                   # 96 tiles: six times the 16 resident waves of one block
FIRST = 4                                       # the first progressive pass
NA = 512                                        # A's samples (the sizing above)
BW, BH = 32, 16                                 # stream B's small frames: 8 tiles, one block


def sky_camera(w, h):
    """From above the cloud, looking up and away from it: every ray misses."""
    return sl.camera((0.0, 50.0, 200.0), (0.0, 150.0, 230.0), w, h)


CAMERAS = {"cloud": sl.cloud_camera, "sky": sky_camera}


@pytest.fixture(scope="module")
def world(rt, oracle):
    """(spheres, n), the prepared scene (created with no hook set) and
    ref(w, h, steps, cam="cloud") -> the oracle's frame, computed once and
    read-only."""
    saved = {k: os.environ.pop(k) for k in HOOKS if k in os.environ}
    S, n = sl.cloud(N_SPHERES)
    sc = rt.SmallptScene(S, n)
    os.environ.update(saved)
    cache = {}

    def ref(w, h, steps, cam="cloud"):
        key = (w, h, tuple(steps), cam)
        if key not in cache:
            cache[key] = L.oracle_frame(oracle, w, h, steps, scene=(S, n), cam=CAMERAS[cam](w, h), nthreads=L.NT)
        return cache[key]

    yield (S, n), sc, ref
    sc.close()


def _frame(rt, sc, w, h, cam="cloud"):
    return rt.SmallptDeviceFrame(sc, CAMERAS[cam](w, h), w, h)


@pytest.fixture
def streams(rt, world, monkeypatch):
    """Two streams that the device runs side by side.  The HIP runtime maps
    its streams onto a few hardware queues, and two streams that share a
    queue run one after the other (measured: with the first two streams a
    process takes from torch, stream B's work started when A had ended).  So
    pairs are drawn until a short one-block launch on the first is still
    running when a fill on the second has completed."""
    import torch
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    probe, flag = _frame(rt, world[1], W, H), torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(8):
        sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
        monkeypatch.setenv("RT_SPT_TUNE", "blocks=1")
        probe.render(8, stream=sa)
        monkeypatch.delenv("RT_SPT_TUNE")
        ev_a, ev_b = torch.cuda.Event(), torch.cuda.Event()
        ev_a.record(sa)
        with torch.cuda.stream(sb):
            flag.fill_(1.0)
        ev_b.record(sb)
        ev_b.synchronize()
        apart = not ev_a.query()
        torch.cuda.synchronize()
        if apart:
            return sa, sb
    pytest.fail("none of eight pairs of streams ran side by side")


def _rehearse(frame, stream, monkeypatch, sequence, counted=False):
    """The test's two streams used side by side once beforehand, complete on
    return: a short one-block launch into `frame` on `stream`, and stream B's
    whole sequence.  The first time a process has work on two streams, and
    the first launch of a kernel variant (the one-block launches change
    variant once they have an order), the second stream's work can wait until
    the device is idle -- measured: an unrehearsed sequence started only when
    A had ended -- which is not the overlap under test."""
    import torch
    monkeypatch.setenv("RT_SPT_TUNE", "blocks=1")
    frame.render(8, counted=counted, stream=stream)
    monkeypatch.delenv("RT_SPT_TUNE")
    sequence()
    torch.cuda.synchronize()


def _first_pass(frame, counted=False):
    """FIRST samples into a fresh frame, complete on return."""
    import torch
    frame.reset()
    if counted:
        frame.counters.zero_()
    frame.render(FIRST, counted=counted)
    torch.cuda.synchronize()


def _launch_a(frame, stream, monkeypatch, counted=False):
    """The long launch: NA further samples in place, on one CU; returns the
    event recorded after it."""
    import torch
    monkeypatch.setenv("RT_SPT_TUNE", "blocks=1")
    frame.render(NA, first_sample=FIRST, seeds_in=frame.seeds, counted=counted, stream=stream)
    monkeypatch.delenv("RT_SPT_TUNE")
    assert frame.scene.info()["nblocks"] == 1
    ev = torch.cuda.Event()
    ev.record(stream)
    return ev


def _assert_overlapped(ev_a, stream_b):
    """A was still running when everything queued on B had completed."""
    import torch
    ev_b = torch.cuda.Event()
    ev_b.record(stream_b)
    ev_b.synchronize()
    assert not ev_a.query(), "the long launch finished before stream B's sequence: nothing overlapped"


def _report(what, frame, ref):
    """The differing pixels of a frame, printed before the assertion."""
    col, seeds, px = frame.host()
    bad = (col.view(np.uint32) != ref[0].view(np.uint32)).reshape(-1, 3).any(axis=1) | \
        (seeds.view(np.uint32) != ref[1].view(np.uint32)).reshape(-1, 2).any(axis=1)
    print("%s: %d of %d pixels differ from the oracle" % (what, int(bad.sum()), bad.size))


# ---- 1. the work-counter ring wraps under a running launch --------------------------
@pytest.mark.parametrize("nb", [64, 130])
def test_ring_wrap_under_a_running_launch(rt, world, streams, monkeypatch, nb):
    """A holds a ring entry; nb one-sample, one-block launches follow on B
    (64: the last takes A's entry again; 130: the ring wraps twice).  A's
    counters must not restart under it."""
    import torch
    _, sc, ref = world
    sa, sb = streams
    assert sc.info()["family"] == "GEO_WIDE"
    a = _frame(rt, sc, W, H)
    small = [_frame(rt, sc, BW, BH) for _ in range(2)]

    def sequence():
        for k in range(nb):
            small[k & 1].render(1, stream=sb)

    _rehearse(a, sa, monkeypatch, sequence)
    for f in small:
        f.reset()
    _first_pass(a)
    ev_a = _launch_a(a, sa, monkeypatch)
    sequence()
    _assert_overlapped(ev_a, sb)
    torch.cuda.synchronize()
    _report("ring wrap x %d, A" % nb, a, ref(W, H, [FIRST, NA]))
    assert_same(a, ref(W, H, [FIRST, NA]), counted=False)
    for f in small:                                              # (the last two B frames)
        assert_same(f, ref(BW, BH, [1]), counted=False)


# ---- 2, 3. the learnt order is rewritten under a launch that reads it -----------------
def _order_rewrite(rt, world, streams, monkeypatch, k2_cam, k2_samples, counted):
    import torch
    _, sc, ref = world
    sa, sb = streams
    assert sc.info()["family"] == "GEO_WIDE"
    a, tmp = _frame(rt, sc, W, H), _frame(rt, sc, W, H)
    k2 = [_frame(rt, sc, W, H, k2_cam) for _ in range(2)]

    def sequence():
        k2[0].render(k2_samples, counted=counted, stream=sb)     # another key: its costs are recorded
        sb.synchronize()                                         # (stream B only)
        k2[1].render(k2_samples, counted=counted, stream=sb)     # builds K2's order and uploads it

    _rehearse(a, sa, monkeypatch, sequence, counted)
    for f in k2:
        f.reset()
    _first_pass(a, counted)
    # K1 (this frame and window, NA samples, the cloud camera) learnt on stream A: the first launch
    # records the tile costs, the second builds the order from them and dispatches by it
    for _ in range(2):
        tmp.render(NA, counted=counted, stream=sa)
        sa.synchronize()
    ev_a = _launch_a(a, sa, monkeypatch, counted)
    sequence()
    _assert_overlapped(ev_a, sb)
    torch.cuda.synchronize()
    want_a, want_k2 = ref(W, H, [FIRST, NA]), ref(W, H, [k2_samples], k2_cam)
    _report("order rewrite (%s camera, %d samples%s), A" % (k2_cam, k2_samples, ", counted" if counted else ""), a,
            want_a)
    assert_same(a, want_a, counted=counted)
    for f in k2:
        assert_same(f, want_k2, counted=counted)


K2 = [pytest.param("cloud", 1, id="one-sample"), pytest.param("sky", NA, id="other-camera")]


@pytest.mark.parametrize("k2_cam,k2_samples", K2)
def test_order_rewrite_under_a_running_launch(rt, world, streams, monkeypatch, k2_cam, k2_samples):
    """K2 has K1's frame size and window, so as many dispatch slots and the
    same order buffer: with one sample, or with K1's samples and another
    camera."""
    _order_rewrite(rt, world, streams, monkeypatch, k2_cam, k2_samples, False)


@pytest.mark.parametrize("k2_cam,k2_samples", K2)
def test_order_rewrite_full_counter_kernels(rt, world, streams, monkeypatch, k2_cam, k2_samples):
    """The same with counted=True on every launch: the full-counter kernels
    learn an order of their own.  The four counters are compared too."""
    _order_rewrite(rt, world, streams, monkeypatch, k2_cam, k2_samples, True)


# ---- 4. control: calls that take no scene state, and a full-scan scene -------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _bits(x):
    import torch
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def test_stateless_calls_beside_a_running_launch(rt, world, streams, monkeypatch):
    """One query, one radiance and one render_pixels call on B while A runs:
    each equals its restatement (ray_query_ref, radiance_ref, pixel_list_ref),
    and A the oracle."""
    import torch
    (S, n), sc, ref = world
    sa, sb = streams
    rays, _ = rq.ray_set(S, n, sl.cloud_camera, 1024)
    want_q = rq.scan(S, n, rays)["nearest"]
    step = rr.reference(S, n, sl.cloud_camera, (16, 8), 256, 0, samples=1)[0]
    snaps = plr.snapshots(S, n, sl.cloud_camera(BW, BH), BW, BH, 2)
    totals = np.zeros((BH, BW), np.int64)
    totals[3:11, 5:23] = 2                                       # the listed pixels take two samples
    ys, xs = np.nonzero(totals)
    d_rays, d_rad_rays, d_seeds = _dev(rays), _dev(step["rays"]), _dev(step["seeds_in"])
    d_list = _dev((ys * BW + xs).astype(np.int32))
    a, pf = _frame(rt, sc, W, H), _frame(rt, sc, BW, BH)
    res = {}

    def sequence():
        with torch.cuda.stream(sb):
            res["q"] = sc.query(d_rays, stream=sb)
            res["r"] = sc.radiance(d_rad_rays, d_seeds, 1, 0, 0, stream=sb)
            pf.render_pixels(d_list, nsamples=2, stream=sb)

    _rehearse(a, sa, monkeypatch, sequence)
    pf.reset()
    pf.seeds.copy_(pf.seeds0)
    pf.done.zero_()
    _first_pass(a)
    ev_a = _launch_a(a, sa, monkeypatch)
    sequence()
    (t, ids), (out, so) = res["q"], res["r"]
    _assert_overlapped(ev_a, sb)
    torch.cuda.synchronize()
    assert_same(a, ref(W, H, [FIRST, NA]), counted=False)
    assert (ids.cpu().numpy() == want_q[1]).all() and (_bits(t) == want_q[0].view(np.uint32)).all()
    assert (_bits(out) == step["col"].view(np.uint32)).all() and (_bits(so) == step["seeds_out"]).all()
    col, seeds, px, done = plr.expected(snaps, totals)
    assert_same(pf, (col, seeds, px), counted=False)
    assert (pf.done.cpu().numpy() == done).all()


def test_full_scan_scene_on_two_streams(rt, oracle, streams):
    """Cornell (the full scan: no order, no ring): two progressive passes of
    two frames, interleaved on two streams."""
    import torch
    sa, sb = streams
    S, n = rt.scenes.cornell()
    sc = rt.SmallptScene(S, n)
    try:
        assert sc.info()["family"] == "GEO_LDS"
        sizes = ((96, 64), (80, 48))
        frames = [rt.SmallptDeviceFrame(sc, rt.scenes.cornell_camera(w, h), w, h) for w, h in sizes]
        for f in frames:
            f.reset()
        torch.cuda.synchronize()
        for first, ns in ((0, 3), (3, 5)):
            for f, s in zip(frames, (sa, sb)):
                f.render(ns, first_sample=first, seeds_in=f.seeds if first else None, stream=s)
        torch.cuda.synchronize()
        for f, (w, h) in zip(frames, sizes):
            assert_same(f, L.oracle_frame(oracle, w, h, [3, 5]), counted=False)
    finally:
        sc.close()


# ---- 5. the level-pass tracers share one arena -------------------------------------------
def test_whitted_and_queue_frames_alternate_on_two_streams(rt, oracle, streams):
    """rtw_render_async and rtq_render_async frames of different small sizes,
    alternating on two streams with no host synchronisation: each waits for
    the arena's previous user (rt_levelpass.h, wf_done)."""
    import torch
    s1, s2 = streams
    wp, wn = rt.scenes.whitted_scene()
    qp, qn = rt.scenes.queue_scene()
    d_w = torch.frombuffer(bytearray(bytes(wp)[:96 * wn]), dtype=torch.uint8).cuda()
    d_q = torch.frombuffer(bytearray(bytes(qp)[:96 * qn]), dtype=torch.uint8).cuda()
    plan = [("whitted", 200, 150, s1), ("queue", 96, 72, s2), ("queue", 160, 120, s1), ("whitted", 97, 131, s2)]
    frames = [torch.zeros(h * w, dtype=torch.int32, device="cuda") for _, w, h, _ in plan]
    torch.cuda.synchronize()
    lib = rt.lib()
    for (kind, w, h, s), f in zip(plan, frames):
        if kind == "whitted":
            rt.check(lib.rtw_render_async(d_w.data_ptr(), wn, f.data_ptr(), w, h, 20, h - 70, None,
                                          C.c_void_p(s.cuda_stream)))
        else:
            rt.check(lib.rtq_render_async(d_q.data_ptr(), qn, f.data_ptr(), w, h, 0, h, None,
                                          C.c_void_p(s.cuda_stream)))
    torch.cuda.synchronize()
    for (kind, w, h, _), f in zip(plan, frames):
        got = f.cpu().numpy()
        if kind == "whitted":
            want, _ = oracle.whitted_render(w, h, nthreads=L.NT)
            assert (got.view(np.uint32).reshape(h, w) == want).all(), (kind, w, h)
        else:
            want, _ = oracle.queue_render(w, h, nthreads=L.NT)
            assert (got.view(np.uint8).reshape(h, w, 4) == want).all(), (kind, w, h)
