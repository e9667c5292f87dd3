"""GPU parity of the adaptive-sampling pieces with their numpy restatement
(tests/adaptive_ref.py, pinned on the CPU by tests/test_adaptive_ref.py), with
no tolerance: floats are compared as bit patterns (a NaN of d_error equal to
any NaN: the expressions fix neither its sign nor its payload), everything
else as integers.

  1. spt_scene_render_pixels_stats_async (render_pixels(stats=True)): every
     kernel family in both modes, mixed takes over two calls with entries
     outside the frame -- colours, seeds, pixels and done are the plain call's
     (pixel_list_ref.expected), m2 is each pixel's snapshot at its own total;
     once more on a one-block grid.
  2. m2 of unlisted pixels, zero takes and out-of-range entries is left alone.
  3. spt_frame_plan_async equals the numpy plan in d_list, d_take, d_error and
     d_totals: on the frames test 1 leaves and on synthetic planes.
  4. frame.refine: the closed loop equals the loop simulated on the reference.
  5. Three (plan, render) pairs captured into one graph replay the eager bits.
  6. Argument errors of both entry points, with nothing launched."""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as ar
import pixel_list_ref as plr
from test_gpu_radiance import FAMILIES, HOOKS, MODES, SCENES

pytestmark = pytest.mark.gpu

PT, DL = 0, 1
W, H = 37, 19
TAKES = np.array([0, 0, 1, 1, 2, 3, 5], np.int32)
NMAX = 2 * int(TAKES.max())
INVALID = -1
LOOP = dict(tol=0.4, min_samples=2, step=2, max_samples=8)      # the closed loop (floor: the default, 1e-3)
# The scan block takes 4,096 tiles a trip (csrc/spt_plan.h, PLAN_SCAN_TRIP: 1,024
# threads, four consecutive tiles each): 520 x 520 is 65 x 65 = 4,225 tiles, one
# full trip and 129 tiles of a second -- 32 threads with four tiles, one with one.
BIG = (520, 520)


def _clean(monkeypatch, **env):
    for k in HOOKS + ("RT_SPT_PIXELS_REFILL",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def world(rt):
    """spheres(name) -> (S, n); snaps(name, nmax, mode) -> adaptive_ref's
    snapshots of the 37 x 19 frame, computed once and read-only; scene(name,
    env, monkeypatch) -> a prepared SmallptScene, kept for the module;
    frames: what test 1 leaves for test 3."""
    sph, refs, scenes, frames = {}, {}, {}, {}

    def spheres(name):
        if name not in sph:
            sph[name] = SCENES[name][0]()
        return sph[name]

    def snaps(name, nmax, mode):
        key = (name, nmax, mode)
        if key not in refs:
            S, n = spheres(name)
            refs[key] = ar.snapshots(S, n, SCENES[name][1](W, H), W, H, nmax, mode)
        return refs[key]

    def scene(name, env, monkeypatch):
        key = (name, tuple(sorted(env.items())))
        _clean(monkeypatch, **env)
        if key not in scenes:
            scenes[key] = rt.SmallptScene(*spheres(name))
        return scenes[key]

    yield spheres, snaps, scene, frames
    frames.clear()
    for sc in scenes.values():
        sc.close()


def _dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _start(frame):
    """A progressive frame's start: zero colours, pixels, counts and m2, the seed fill."""
    frame.m2
    frame.done
    frame.reset()
    frame.seeds.copy_(frame.seeds0)
    return frame


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _assert_expected(frame, snaps, totals, what=""):
    """Every word of the five planes is the snapshot's of the pixel's total."""
    ecol, eseeds, epx, edone = plr.expected(snaps, totals)
    em2 = ar.expected_m2(snaps, totals)
    col, seeds, px = frame.host()
    done, m2 = frame.done.cpu().numpy(), _bits(frame.m2)
    bad = np.flatnonzero((col.view(np.uint32).reshape(-1, 3) != ecol.view(np.uint32).reshape(-1, 3)).any(axis=1)
                         | (seeds.reshape(-1, 2) != eseeds.reshape(-1, 2)).any(axis=1) | (done != edone))
    assert len(bad) == 0, "%s: %d slots differ from the plain call's, first slot %d: done %d want %d" % (
        what, len(bad), bad[0], done[bad[0]], edone[bad[0]])
    assert (px == epx).all(), "%s: %d packed pixels differ" % (what, (px != epx).sum())
    bad = np.flatnonzero(m2 != em2.view(np.uint32))
    assert len(bad) == 0, "%s: m2 differs in %d slots, first slot %d (done %d): %r want %r" % (
        what, len(bad), bad[0], done[bad[0]], m2[bad[0]:bad[0] + 1].view(np.float32)[0], em2[bad[0]])


def _totals(pixels, take):
    t = np.zeros(W * H, np.int64)
    ok = (pixels >= 0) & (pixels < W * H)
    np.add.at(t, pixels[ok], np.maximum(take[ok], 0))
    return t.reshape(H, W)


def _mixed_lists():
    """Two seeded permutations of all pixels with takes from TAKES, entries -1
    and w * h (with a take) sprinkled in between."""
    rng = np.random.default_rng(17)
    lists = []
    for _ in range(2):
        p, t = rng.permutation(W * H).astype(np.int32), TAKES[rng.integers(0, len(TAKES), W * H)]
        at = np.arange(5, W * H, 41)
        p = np.insert(p, at, np.where(np.arange(len(at)) % 2, -1, W * H).astype(np.int32))
        t = np.insert(t, at, 3).astype(np.int32)
        lists.append((p, t))
    return lists


# ---- 1. stats equals plain, m2 equals the reference -----------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,env,family,leaf", FAMILIES)
def test_stats_call_equals_plain_and_m2_the_reference(rt, world, monkeypatch, name, env, family, leaf, mode):
    sc = world[2](name, env, monkeypatch)
    info = sc.info()
    assert info["family"] == family and info["leaf_max"] == leaf, info
    cam = SCENES[name][1](W, H)
    lists = _mixed_lists()
    assert all((p < 0).any() and (p >= W * H).any() for p, _ in lists)
    totals = sum(_totals(p, t) for p, t in lists)
    assert totals.min() == 0 and totals.max() >= 6 and len(np.unique(totals)) >= 7
    snaps = world[1](name, NMAX, mode)
    frame = _start(rt.SmallptDeviceFrame(sc, cam, W, H))
    frame.render_pixels(_dev(lists[0][0]), _dev(lists[0][1]), mode=mode, stats=True)
    _assert_expected(frame, snaps, _totals(*lists[0]), "%s first call" % name)
    frame.render_pixels(_dev(lists[1][0]), _dev(lists[1][1]), mode=mode, stats=True)
    _assert_expected(frame, snaps, totals, "%s second call" % name)
    world[3][(name, family, leaf, mode)] = frame
    monkeypatch.setenv("RT_SPT_QUERY_BLOCKS", "1")
    one = _start(rt.SmallptDeviceFrame(sc, cam, W, H))
    for p, t in lists:
        one.render_pixels(_dev(p), _dev(t), mode=mode, stats=True)
    _assert_expected(one, snaps, totals, "%s one block" % name)


# ---- 2. m2 left alone ------------------------------------------------------------------------
def test_m2_of_unlisted_pixels_is_left_alone(rt, world, monkeypatch):
    """A pattern in m2, every third pixel listed (every fifth of those with a
    take of 0), entries outside the frame in between: only the listed pixels
    with a take get a new m2 -- their snapshot's."""
    sc = world[2]("cornell", {}, monkeypatch)
    frame = _start(rt.SmallptDeviceFrame(sc, SCENES["cornell"][1](W, H), W, H))
    MP = -3.5
    frame.m2.fill_(MP)
    pixels = np.arange(0, W * H, 3, dtype=np.int32)
    take = np.where(np.arange(len(pixels)) % 5 == 0, 0, 2).astype(np.int32)
    at = np.arange(2, len(pixels), 17)
    lp = np.insert(pixels, at, np.where(np.arange(len(at)) % 2, -1, W * H).astype(np.int32))
    lt = np.insert(take, at, 2).astype(np.int32)
    frame.render_pixels(_dev(lp), _dev(lt), stats=True)
    m2 = frame.m2.cpu().numpy()
    slot = (H - pixels // W - 1) * W + pixels % W
    listed = np.zeros(W * H, bool)
    listed[slot[take > 0]] = True
    assert (m2[~listed] == MP).all() and (~listed).sum() > W * H // 2
    em2 = ar.expected_m2(world[1]("cornell", NMAX, PT), _totals(pixels, take))
    assert (m2[listed].view(np.uint32) == em2[listed].view(np.uint32)).all() and (m2[listed] >= 0).all()
    assert (frame.done.cpu().numpy()[listed] == 2).all()


# ---- 3. the plan equals the numpy plan ----------------------------------------------------------
def _plan_call(rt, col, m2, done, w, h, params, cap, error=True, totals=True, guard=16):
    """spt_frame_plan_async on device copies of the planes; (list, take,
    error bits or None, totals or None) on the host.  The list and take
    tensors carry `guard` words more than cap, which must keep their pattern."""
    import torch
    d_col, d_m2, d_done = _dev(col, np.float32), _dev(m2, np.float32), _dev(done)
    d_list = torch.full((cap + guard,), 77, dtype=torch.int32, device="cuda")
    d_take = torch.full((cap + guard,), 88, dtype=torch.int32, device="cuda")
    d_err = torch.full((w * h,), -1.0, dtype=torch.float32, device="cuda") if error else None
    d_tot = torch.full((2,), -1, dtype=torch.int64, device="cuda") if totals else None
    scratch = torch.zeros(rt.lib().spt_frame_plan_scratch_bytes(w, h) // 8, dtype=torch.int64, device="cuda")
    p = rt._lib.PlanParams(*params)
    rc = rt.lib().spt_frame_plan_async(
        d_col.data_ptr(), d_m2.data_ptr(), d_done.data_ptr(), w, h, C.byref(p), d_list.data_ptr(), d_take.data_ptr(), cap,
        d_err.data_ptr() if error else None, d_tot.data_ptr() if totals else None, scratch.data_ptr(), None)
    assert rc == 0, rt.lib().rt_last_error()
    torch.cuda.synchronize()
    lst, tk = d_list.cpu().numpy(), d_take.cpu().numpy()
    assert (lst[cap:] == 77).all() and (tk[cap:] == 88).all(), "written past cap"
    return (lst[:cap], tk[:cap], d_err.cpu().numpy() if error else None,
            tuple(int(v) for v in d_tot.cpu().numpy()) if totals else None)


def _assert_plan(rt, col, m2, done, w, h, params, cap, what, **kw):
    elist, etake, eerr, etot = ar.plan(col, m2, done, w, h, params, cap)
    lst, tk, err, tot = _plan_call(rt, col, m2, done, w, h, params, cap, **kw)
    assert tot is None or tot == etot, "%s: totals %r want %r" % (what, tot, etot)
    bad = np.flatnonzero((lst != elist) | (tk != etake))
    assert len(bad) == 0, "%s: %d of %d entries differ, first %d: (%d, %d) want (%d, %d)" % (
        what, len(bad), cap, bad[0], lst[bad[0]], tk[bad[0]], elist[bad[0]], etake[bad[0]])
    if err is not None:
        bad = np.flatnonzero(~ar.same_floats(err, eerr))
        assert len(bad) == 0, "%s: d_error differs in %d slots, first %d: %r want %r" % (
            what, len(bad), bad[0], err[bad[0]], eerr[bad[0]])
    return etot


def _param_sets(mx):
    """(name, (min, max, step, tol, floor)): the tolerance's two ends, max ==
    min, a step past max - n, and a middle case."""
    inf = float("inf")
    return [("mid", (2, mx, 2, 0.3, 1e-3)), ("tol0", (1, mx, 3, 0.0, 0.0)), ("tolinf", (3, mx, 2, inf, 1e-3)),
            ("max=min", (mx, mx, 1, 0.1, 1e-3)), ("bigstep", (1, mx, 1000, 0.05, 0.5))]


@pytest.mark.parametrize("mode", MODES)
def test_plan_on_the_frames_test_one_leaves(rt, world, monkeypatch, mode):
    """Uneven done (0 .. 10) from the mixed takes, real colours and m2."""
    key = ("cornell", "GEO_LDS", 0, mode)
    if key not in world[3]:                                     # (run alone: make the frame here)
        sc = world[2]("cornell", {}, monkeypatch)
        frame = _start(rt.SmallptDeviceFrame(sc, SCENES["cornell"][1](W, H), W, H))
        for p, t in _mixed_lists():
            frame.render_pixels(_dev(p), _dev(t), mode=mode, stats=True)
        world[3][key] = frame
    frame = world[3][key]
    col, _, _ = frame.host()
    m2, done = frame.m2.cpu().numpy(), frame.done.cpu().numpy()
    assert done.min() == 0 and done.max() >= 6
    counts = []
    for what, params in _param_sets(8):
        tot = _assert_plan(rt, col, m2, done, W, H, params, W * H, what)
        counts.append(tot[0])
        _assert_plan(rt, col, m2, done, W, H, params, max(tot[0] // 2, 1), what + " truncated")
        _assert_plan(rt, col, m2, done, W, H, params, 0, what + " cap 0")
    assert all(0 < c < W * H for c in counts) and len(set(counts)) >= 3
    # the frame's own method on its own planes: the same list, frame-owned and reused
    pixels, take = frame.plan(0.3, 2, 8, 2, error=True)
    again, _ = frame.plan(0.3, 2, 8, 2)
    assert again.data_ptr() == pixels.data_ptr() and pixels.numel() == W * H
    elist, etake, eerr, etot = ar.plan(col, m2, done, W, H, (2, 8, 2, 0.3, 1e-3), W * H)
    assert (pixels.cpu().numpy() == elist).all() and (take.cpu().numpy() == etake).all()
    assert tuple(frame.plan_totals.cpu().numpy()) == etot and ar.same_floats(frame.error.cpu().numpy(), eerr).all()


def _synthetic(w, h, mx, seed):
    """Random done in [0, max]; colours in [0, 4); m2 below, equal to and above
    |c|^2; zero colours (with zero and non-zero m2); NaN and +-inf in colours
    and m2."""
    rng = np.random.default_rng(seed)
    n = w * h
    done = rng.integers(0, mx + 1, n).astype(np.int32)
    c = (rng.random((n, 3)) * 4).astype(np.float32)
    kind = rng.integers(0, 12, n)
    if n >= 64:
        kind[:12] = np.arange(12)                               # every kind at least once
    c[(kind == 3) | (kind == 4)] = 0
    mean2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
    m2 = (mean2 * (1 + rng.random(n) * np.where(rng.random(n) < .5, 2, .05))).astype(np.float32)     # above, far and near
    m2[kind == 0] = mean2[kind == 0]                            # equal: var 0
    m2[kind == 1] = mean2[kind == 1] * np.float32(.75)          # below: var negative
    m2[kind == 2] = np.nextafter(mean2[kind == 2], np.float32(np.inf))     # one ulp above
    m2[kind == 4] = 1.5                                         # spread over a zero colour
    c[kind == 5, 0] = np.nan
    c[kind == 6, 1] = np.inf
    c[kind == 7, 2] = -np.inf
    m2[kind == 8] = np.nan
    m2[kind == 9] = np.inf
    m2[kind == 10] = -np.inf
    return c.reshape(-1), m2, done


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (9, 1), (W, H), BIG], ids=lambda v: str(v))
def test_plan_on_synthetic_planes(rt, w, h):
    mx = 12
    col, m2, done = _synthetic(w, h, mx, 100 + w)
    assert (w, h) != BIG or (ar.tile_key(np.array([w - 1]), np.array([h - 1]), w)[0] // 64 + 1) % 4096 == 129
    for what, params in _param_sets(mx):
        tot = _assert_plan(rt, col, m2, done, w, h, params, w * h, "%dx%d %s" % (w, h, what))
        if tot[0] > 1:
            _assert_plan(rt, col, m2, done, w, h, params, tot[0] - 1, "%dx%d %s cap below the count" % (w, h, what))
            _assert_plan(rt, col, m2, done, w, h, params, tot[0] // 3, "%dx%d %s cap a third" % (w, h, what))
        _assert_plan(rt, col, m2, done, w, h, params, 0, "%dx%d %s cap 0" % (w, h, what))
        _assert_plan(rt, col, m2, done, w, h, params, w * h + 5, "%dx%d %s cap above w*h, no error, no totals" % (w, h, what),
                     error=False, totals=False)
    if w * h >= 64:
        tol0, tolinf = (ar.plan(col, m2, done, w, h, p, w * h)[3][0] for _, p in _param_sets(mx)[1:3])
        assert tol0 > tolinf > 0 and tol0 < w * h               # tol = inf: the bootstrap only; tol = 0: not everything


# ---- 4. the closed loop ------------------------------------------------------------------------
def _loop_condition(totals, log):
    """Asserted on the reference alone: after the bootstrap the passes list
    between 10 % and 90 % of the pixels until the last lists none, and each of
    the totals 2, 4, 6, 8 occurs."""
    shares = [l[0] / (W * H) for l in log]
    assert shares[0] == 1.0 and shares[-1] == 0.0 and all(0.1 < s < 0.9 for s in shares[1:-1]), shares
    assert sorted(np.unique(totals)) == [2, 4, 6, 8], np.unique(totals)


def _cloud_tol(snaps):
    """The tolerance of the cloud's loop, from the reference's error map after
    the two bootstrap samples: the median of its positive entries (half the
    frame sees the background, whose error is 0)."""
    col, _, _, done = plr.expected(snaps, np.full((H, W), 2))
    err = ar.plan(col, snaps["m2"][2], done, W, H, (2, 8, 2, 0.0, 1e-3), W * H)[2]
    return float(np.float32(np.median(err[np.isfinite(err) & (err > 0)])))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["cornell", "cloud3000"])
def test_refine_equals_the_loop_on_the_reference(rt, world, monkeypatch, name, mode):
    import torch
    sc = world[2](name, {}, monkeypatch)
    snaps = world[1](name, NMAX, mode)
    loop = dict(LOOP)
    if name != "cornell":
        loop["tol"] = _cloud_tol(snaps)
    params = (loop["min_samples"], loop["max_samples"], loop["step"], np.float32(loop["tol"]), 1e-3)
    totals, log = ar.refine(snaps, 5, params)
    _loop_condition(totals, log)
    frame = _start(rt.SmallptDeviceFrame(sc, SCENES[name][1](W, H), W, H))
    frame.refine(4, mode=mode, **loop)
    torch.cuda.synchronize()
    assert tuple(frame.plan_totals.cpu().numpy()) == log[3]
    frame.refine(1, mode=mode, **loop)
    _assert_expected(frame, snaps, totals, "%s after five passes" % name)
    assert tuple(frame.plan_totals.cpu().numpy()) == (0, 0)
    pixels, take = frame.plan(**loop)
    assert (pixels == -1).all() and (take == 0).all()


# ---- 5. capture ------------------------------------------------------------------------------------
def test_three_captured_pairs_replay_the_eager_bits(rt, world, monkeypatch):
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    cam = SCENES["cornell"][1](W, H)
    eager, frame = rt.SmallptDeviceFrame(sc, cam, W, H), rt.SmallptDeviceFrame(sc, cam, W, H)
    _start(eager).refine(3, **LOOP)
    _start(frame)
    frame.plan(**LOOP)                                      # (the frame's buffers are made before the capture)
    frame.plan_totals.fill_(-1)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frame.refine(3, **LOOP)
    _start(frame)
    g.replay()
    torch.cuda.synchronize()
    assert frame.same_bits(eager) and torch.equal(frame.done, eager.done)
    assert torch.equal(frame.m2.view(torch.int32), eager.m2.view(torch.int32))
    assert torch.equal(frame.plan_totals, eager.plan_totals) and int(frame.plan_totals[0]) > 0
    assert 4 <= int(frame.done.max()) <= 6 and int(frame.done.min()) == 2
    snaps = world[1]("cornell", NMAX, PT)
    totals, _ = ar.refine(snaps, 3, (2, 8, 2, np.float32(0.4), 1e-3))
    _assert_expected(frame, snaps, totals, "replay")
    del g


# ---- 6. argument errors --------------------------------------------------------------------------
def test_stats_call_argument_errors(rt, world, monkeypatch):
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    w, h = 8, 8
    cam = SCENES["cornell"][1](w, h)
    frame = rt.SmallptDeviceFrame(sc, cam, w, h)
    frame.reset(colors=-7.0, pixels=0xA5A5A5A5, seeds=0x12345678)
    frame.done.fill_(9)
    frame.m2.fill_(-2.0)
    pixels, take = _dev(np.arange(16)), _dev(np.ones(16))
    f = rt.lib().spt_scene_render_pixels_stats_async
    ok = dict(scene=sc.handle, camera=C.byref(cam), d_colors=frame.colors.data_ptr(), d_seeds_in=frame.seeds0.data_ptr(),
              d_seeds_out=frame.seeds.data_ptr(), d_pixels=frame.pixels.data_ptr(), d_m2=frame.m2.data_ptr(), w=w, h=h,
              d_list=pixels.data_ptr(), d_take=None, nlist=16, nsamples=1, d_done=None, first_sample=0, mode=PT, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    for null in ("scene", "camera", "d_colors", "d_seeds_in", "d_seeds_out", "d_pixels", "d_m2", "d_list"):
        assert call(**{null: None}) == INVALID, null
    assert "spt_scene_render_pixels_stats_async" in rt.lib().rt_last_error().decode()
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=-3) == INVALID
    assert call(w=1 << 16, h=1 << 15) == INVALID
    assert call(nsamples=-1) == INVALID and call(first_sample=-1) == INVALID
    assert call(d_take=take.data_ptr(), nsamples=1) == INVALID
    assert call(d_done=frame.done.data_ptr(), first_sample=1) == INVALID
    for mode in (2, -1, PT | rt.SPT_COUNT_RAYS, DL | rt.SPT_COST_MAX, PT | rt.SPT_LIST_SET):
        assert call(mode=mode) == INVALID, mode
    assert call(nlist=2 ** 31) == INVALID
    assert call(nlist=0) == 0
    torch.cuda.synchronize()
    assert (frame.colors == -7.0).all() and (frame.pixels == rt.device._i32(0xA5A5A5A5)).all()
    assert (frame.seeds == 0x12345678).all() and (frame.done == 9).all() and (frame.m2 == -2.0).all()
    with pytest.raises(rt.RTError):
        frame.render_pixels(pixels, take, nsamples=2, stats=True)


def test_plan_argument_errors(rt):
    import torch
    w, h = 8, 8
    col = torch.full((3 * w * h,), 1.0, device="cuda")
    m2 = torch.full((w * h,), 4.0, device="cuda")
    done = torch.full((w * h,), 4, dtype=torch.int32, device="cuda")
    lst = torch.full((w * h,), 77, dtype=torch.int32, device="cuda")
    take = torch.full((w * h,), 88, dtype=torch.int32, device="cuda")
    err = torch.full((w * h,), -1.0, device="cuda")
    tot = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    L = rt.lib()
    assert L.spt_frame_plan_scratch_bytes(w, h) >= 12 and L.spt_frame_plan_scratch_bytes(1920, 1080) >= 12 * 240 * 135
    assert L.spt_frame_plan_scratch_bytes(0, 8) == 0 and L.spt_frame_plan_scratch_bytes(1 << 16, 1 << 15) == 0
    scratch = torch.full((L.spt_frame_plan_scratch_bytes(w, h) // 8,), 5, dtype=torch.int64, device="cuda")
    good = dict(min_samples=2, max_samples=8, step=2, tol=0.1, floor=1e-3)
    ok = dict(d_colors=col.data_ptr(), d_m2=m2.data_ptr(), d_done=done.data_ptr(), w=w, h=h, params=good,
              d_list=lst.data_ptr(), d_take=take.data_ptr(), cap=w * h, d_error=err.data_ptr(), d_totals=tot.data_ptr(),
              d_scratch=scratch.data_ptr(), stream=None)

    def call(**kw):
        a = {**ok, **kw}
        if a["params"] is not None:
            p = rt._lib.PlanParams(**{**good, **a["params"]})
            a["params"] = C.byref(p)
        return L.spt_frame_plan_async(*a.values())

    for null in ("d_colors", "d_m2", "d_done", "params", "d_list", "d_take", "d_scratch"):
        assert call(**{null: None}) == INVALID, null
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(h=-1) == INVALID
    assert call(w=1 << 16, h=1 << 15) == INVALID
    for bad in (dict(min_samples=0), dict(max_samples=1), dict(step=0), dict(step=-4), dict(tol=float("nan")),
                dict(tol=-0.5), dict(floor=float("nan")), dict(floor=-1e-3)):
        assert call(params=bad) == INVALID, bad
    assert call(cap=2 ** 31) == INVALID
    torch.cuda.synchronize()
    assert (lst == 77).all() and (take == 88).all() and (err == -1.0).all() and (tot == -1).all() and (scratch == 5).all()
    # what is legal: cap == 0 without lists, no error plane, no totals; tol = +inf, floor = 0
    assert call(cap=0, d_list=None, d_take=None) == 0
    torch.cuda.synchronize()
    assert (lst == 77).all() and (take == 88).all() and tuple(tot.cpu().numpy()) == (64, 128) and (err > 0).all()
    assert call(d_error=None, d_totals=None, params=dict(tol=float("inf"), floor=0.0)) == 0
    torch.cuda.synchronize()
    assert (lst == -1).all() and (take == 0).all()
