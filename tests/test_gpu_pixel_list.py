"""GPU parity of the pixel lists (spt_scene_render_pixels_async,
csrc/spt_pixels.h; SmallptDeviceFrame.render_pixels) with the oracle, with no
tolerance: every listed and every unlisted pixel of the frame is compared --
colours as bits, seeds, packed pixels and sample counts as integers.  The
reference is tests/pixel_list_ref.py (pinned on the CPU by
tests/test_pixel_list_ref.py): each pixel from the oracle's frame after as
many samples as the pixel has had.  Covered: every kernel family and hierarchy
layout in both modes with mixed takes over two calls, refill under skewed
takes on a one-block grid, pixels left untouched, equality with the renderer,
the scalar and the per-entry form, ordering after in-place edits, graph
capture, budget maps, argument errors."""
import numpy as np
import pytest

import pixel_list_ref as plr
import ray_query_ref as rq
import scenes_layouts as sl
from test_gpu_radiance import FAMILIES, HOOKS, MODES, SCENES, _moved

pytestmark = pytest.mark.gpu

PT, DL = 0, 1
DIFF, SPEC, REFR = 0, 1, 2
W, H = 37, 19                                   # the mixed-take frame: lanes past both tile edges
TAKES = np.array([0, 0, 1, 1, 2, 3, 5], np.int32)
WS, HS, TALL = 40, 24, 40                       # the skew frame and its one long take
INVALID = -1


def _clean(monkeypatch, **env):
    for k in HOOKS + ("RT_SPT_PIXELS_REFILL",):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def world(rt):
    """spheres(name) -> (S, n); snaps(name, w, h, nmax, mode) -> the oracle's
    snapshots, computed once and read-only; scene(name, env, monkeypatch) -> a
    prepared SmallptScene, kept for the module."""
    sph, refs, scenes = {}, {}, {}

    def spheres(name):
        if name not in sph:
            sph[name] = SCENES[name][0]()
        return sph[name]

    def snaps(name, w, h, nmax, mode):
        key = (name, w, h, nmax, mode)
        if key not in refs:
            S, n = spheres(name)
            refs[key] = plr.snapshots(S, n, SCENES[name][1](w, h), w, h, nmax, mode)
        return refs[key]

    def scene(name, env, monkeypatch):
        key = (name, tuple(sorted(env.items())))
        _clean(monkeypatch, **env)
        if key not in scenes:
            scenes[key] = rt.SmallptScene(*spheres(name))
        return scenes[key]

    yield spheres, snaps, scene
    for sc in scenes.values():
        sc.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def _start(frame):
    """A progressive frame's start: zero colours, pixels and counts, the seed fill."""
    frame.reset()
    frame.seeds.copy_(frame.seeds0)
    return frame


def _state(frame):
    """(colours as bits, seeds, pixels, done) on the host."""
    col, seeds, px = frame.host()
    return col.view(np.uint32), seeds, px, frame.done.cpu().numpy()


def _assert_expected(frame, snaps, totals, what=""):
    """Every word of the four buffers is the snapshot's of the pixel's total."""
    ecol, eseeds, epx, edone = plr.expected(snaps, totals)
    col, seeds, px, done = _state(frame)
    w = frame.w
    bad = np.flatnonzero((col.reshape(-1, 3) != ecol.view(np.uint32).reshape(-1, 3)).any(axis=1)
                         | (seeds.reshape(-1, 2) != eseeds.reshape(-1, 2)).any(axis=1) | (done != edone))
    assert len(bad) == 0, "%s: %d slots differ, first slot %d (x %d, row %d from the top of the buffer): done %d want %d" % (
        what, len(bad), bad[0], bad[0] % w, bad[0] // w, done[bad[0]], edone[bad[0]])
    badp = np.flatnonzero(px != epx)
    assert len(badp) == 0, "%s: %d packed pixels differ, first %d: %08x want %08x" % (
        what, len(badp), badp[0], px[badp[0]], epx[badp[0]])


def _totals(w, h, pixels, take):
    """The [h, w] map of samples a list adds (entries outside the frame dropped)."""
    t = np.zeros(w * h, np.int64)
    ok = (pixels >= 0) & (pixels < w * h)
    np.add.at(t, pixels[ok], np.maximum(take[ok], 0))
    return t.reshape(h, w)


# ---- 1. mixed takes, every family, both modes -------------------------------------------
def _cornell_coverage(S, n, cam, snaps, pixels, take):
    """What the Cornell list must exercise: first hits of the listed pixels
    (with a take) on diffuse, mirror, glass and emitting spheres, from the
    full-scan restatement along the pixel centres' rays, and shadow rays and
    bounces from the oracle's counters."""
    import rtamd
    rows = sl.rows_of(S, n)
    p = pixels[take > 0]
    rays = rtamd.scenes.camera_rays(cam, W, H, p % W, p // W)
    first = rq.scan(S, n, rays)["nearest"][1]
    hit = first >= 0
    emits = (rows[first, 4] != 0) | (rows[first, 6] != 0)
    refl = rows[first, 10].view(np.int32)
    for kind in (DIFF, SPEC, REFR):
        assert (hit & ~emits & (refl == kind)).any(), kind
    cnt = snaps["cnt"][1]
    assert cnt[1] > 0                                           # IntersectP calls: shadow rays were traced
    assert cnt[0] >= 3 * cnt[3]                                 # Intersect calls >= 3 x samples: paths bounce


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,env,family,leaf", FAMILIES)
def test_mixed_takes_equal_oracle(rt, world, monkeypatch, name, env, family, leaf, mode):
    """A seeded permutation of all 37 x 19 pixels with takes from {0, 0, 1, 1,
    2, 3, 5}, then a second permutation with other takes, both numbered by
    `done`: every buffer equals the oracle's for the summed totals."""
    sc = world[2](name, env, monkeypatch)
    info = sc.info()
    assert info["family"] == family and info["leaf_max"] == leaf, info
    cam = SCENES[name][1](W, H)
    rng = np.random.default_rng(17)
    lists = [(rng.permutation(W * H).astype(np.int32), TAKES[rng.integers(0, len(TAKES), W * H)]) for _ in range(2)]
    totals = sum(_totals(W, H, p, t) for p, t in lists)
    assert totals.min() == 0 and totals.max() >= 6 and len(np.unique(totals)) >= 7
    snaps = world[1](name, W, H, 2 * int(TAKES.max()), mode)
    if name == "cornell" and mode == PT:
        _cornell_coverage(*world[0](name), cam, snaps, *lists[0])
    frame = _start(rt.SmallptDeviceFrame(sc, cam, W, H))
    frame.render_pixels(_dev(lists[0][0]), _dev(lists[0][1]), mode=mode)
    _assert_expected(frame, snaps, _totals(W, H, *lists[0]), "%s first call" % name)
    frame.render_pixels(_dev(lists[1][0]), _dev(lists[1][1]), mode=mode)
    _assert_expected(frame, snaps, totals, "%s second call" % name)


# ---- 2. refill under skew, one block -----------------------------------------------------
def _skew_list(count, rng):
    """`count` entries over distinct pixels of the 40 x 24 frame: takes of 1
    but for TALL at positions 0, 63, 64 and the last, (long lists) a stretch
    of 70 zero takes, and entries -1 and w * h sprinkled in."""
    pixels = rng.permutation(WS * HS)[:count].astype(np.int32)
    take = np.ones(count, np.int32)
    tall = sorted({q for q in (0, 63, 64, count - 1) if q < count})
    take[tall] = TALL
    if count >= 400:
        take[200:270] = 0
        assert (take[200:270] == 0).all() and 270 - 200 > 64
    for q in range(5, count, 37):
        if q not in tall:
            pixels[q] = -1 if (q // 37) % 2 else WS * HS
            take[q] = 3
    return pixels, take


@pytest.mark.parametrize("mode", MODES)
def test_refill_under_skew_on_a_one_block_grid(rt, world, monkeypatch, mode):
    """One block of four waves: lists of 1, 63, 64, 65, 129 and 900 entries
    (900 > 64 x 4 x 3: every wave takes a fourth chunk), one lane at 40
    samples among lanes at 1.  Each pixel is the oracle's at its own take."""
    sc = world[2]("cornell", {}, monkeypatch)
    monkeypatch.setenv("RT_SPT_QUERY_BLOCKS", "1")
    cam = SCENES["cornell"][1](WS, HS)
    snaps = world[1]("cornell", WS, HS, TALL, mode)
    frame = rt.SmallptDeviceFrame(sc, cam, WS, HS)
    rng = np.random.default_rng(23)
    for count in (1, 63, 64, 65, 129, 900):
        assert count <= WS * HS
        pixels, take = _skew_list(count, rng)
        _start(frame).render_pixels(_dev(pixels), _dev(take), mode=mode)
        totals = _totals(WS, HS, pixels, take)
        assert totals.max() == TALL and (count < 2 or (totals == 1).sum() > count // 2)
        _assert_expected(frame, snaps, totals, "%d entries" % count)


def test_refill_hook_changes_no_bit(rt, world, monkeypatch):
    """RT_SPT_PIXELS_REFILL=0, the chunk-synchronous form the timing tool
    compares with: the same frame."""
    sc = world[2]("cornell", {}, monkeypatch)
    monkeypatch.setenv("RT_SPT_QUERY_BLOCKS", "1")
    monkeypatch.setenv("RT_SPT_PIXELS_REFILL", "0")
    cam = SCENES["cornell"][1](WS, HS)
    snaps = world[1]("cornell", WS, HS, TALL, PT)
    pixels, take = _skew_list(900, np.random.default_rng(29))
    frame = _start(rt.SmallptDeviceFrame(sc, cam, WS, HS))
    frame.render_pixels(_dev(pixels), _dev(take))
    _assert_expected(frame, snaps, _totals(WS, HS, pixels, take), "no refill")


# ---- 3. unlisted pixels -----------------------------------------------------------------
@pytest.mark.parametrize("in_place", [False, True], ids=["distinct-seeds", "seeds-in-place"])
def test_unlisted_pixels_are_untouched(rt, world, monkeypatch, in_place):
    """Patterns in all four buffers, every third pixel listed (every fifth of
    those with a take of 0): all other words keep their patterns; a zero take
    moves the two seed words and nothing else."""
    sc = world[2]("cornell", {}, monkeypatch)
    cam = SCENES["cornell"][1](W, H)
    frame = rt.SmallptDeviceFrame(sc, cam, W, H)
    CP, PP, SP, DP = -7.25, 0xA5A5A5A5, 0x12345678, 5
    frame.reset(colors=CP, pixels=PP, seeds=SP)
    frame.done.fill_(DP)
    pixels = np.arange(0, W * H, 3, dtype=np.int32)
    take = np.where(np.arange(len(pixels)) % 5 == 0, 0, 2).astype(np.int32)
    frame.render_pixels(_dev(pixels), _dev(take), seeds_in=frame.seeds if in_place else frame.seeds0)
    col, seeds, px, done = _state(frame)
    seeds0 = frame.seeds0.cpu().numpy().view(np.uint32)
    x, y = pixels % W, pixels // W
    slot = (H - y - 1) * W + x
    listed = np.zeros(W * H, bool)
    listed[slot[take > 0]] = True
    zero = np.zeros(W * H, bool)
    zero[slot[take == 0]] = True
    cp = np.array([CP], np.float32).view(np.uint32)[0]
    col, seeds = col.reshape(-1, 3), seeds.reshape(-1, 2)
    assert (col[~listed] == cp).all() and (done[~listed] == DP).all()
    assert (seeds[~listed & ~zero] == SP).all()
    assert (seeds[zero] == (SP if in_place else seeds0.reshape(-1, 2)[zero])).all()
    listed_px = np.zeros(W * H, bool)
    listed_px[pixels[take > 0]] = True
    assert (px[~listed_px] == PP).all() and (px[listed_px] != PP).all()
    assert (done[listed] == DP + 2).all() and (col[listed] != cp).all() and (seeds[listed] != SP).any(axis=1).all()


# ---- 4. against the renderer ---------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["cornell", "cloud3000"])
def test_all_pixels_listed_continue_a_rendered_frame(rt, world, monkeypatch, name, mode):
    """render(2), then every pixel listed with nsamples = 3 from first_sample
    = 2 and no `done`: the bits of render(5)."""
    sc = world[2](name, {}, monkeypatch)
    w, h = 40, 24
    cam = SCENES[name][1](w, h)
    a, b = rt.SmallptDeviceFrame(sc, cam, w, h), rt.SmallptDeviceFrame(sc, cam, w, h)
    a.reset().render(2, mode=mode)
    pixels = _dev(np.random.default_rng(3).permutation(w * h))
    a.render_pixels(pixels, nsamples=3, use_done=False, first_sample=2, mode=mode, seeds_in=a.seeds)
    b.reset().render(5, mode=mode)
    assert a.same_bits(b)
    assert a._done is None and b.pixels.any()


# ---- 5. the scalar and the per-entry form ----------------------------------------------------
@pytest.mark.parametrize("name,env", [("cornell", {}), ("cloud3000", {}), ("cloud3000", {"RT_SPT_WIDE": "0"})],
                         ids=["cornell", "cloud3000-wide", "cloud3000-binary"])
def test_scalar_and_per_entry_takes_agree(rt, world, monkeypatch, name, env):
    import torch
    sc = world[2](name, env, monkeypatch)
    cam = SCENES[name][1](W, H)
    a, b = rt.SmallptDeviceFrame(sc, cam, W, H), rt.SmallptDeviceFrame(sc, cam, W, H)
    pixels = _dev(np.random.default_rng(4).permutation(W * H)[:500])
    _start(a).render_pixels(pixels, nsamples=3)
    _start(b).render_pixels(pixels, torch.full_like(pixels, 3))
    assert a.same_bits(b) and torch.equal(a.done, b.done) and int(a.done.sum()) == 1500
    assert a.pixels.any()


# ---- 6. ordering, capture ------------------------------------------------------------------------
@pytest.mark.parametrize("env,family", [({}, "GEO_WIDE"), ({"RT_SPT_WIDE": "0"}, "GEO_BVH")], ids=["wide", "binary"])
def test_pixels_after_update_see_the_edited_spheres(rt, world, monkeypatch, env, family):
    """update() then render_pixels() on one stream, nothing in between: the
    frame of a scene created from the edited array (and not the old one)."""
    import torch
    _clean(monkeypatch, **env)
    rows = sl.cloud_rows(sl.N_LEAF8)
    S, n = sl.pack(rows)
    S2, _ = sl.pack(_moved(rows, 1))
    cam = sl.cloud_camera(W, H)
    pixels = _dev(np.random.default_rng(6).permutation(W * H))
    sc, fresh = rt.SmallptScene(S, n), rt.SmallptScene(S2, n)
    try:
        assert sc.info()["family"] == family == fresh.info()["family"]
        old, want, got = (rt.SmallptDeviceFrame(s, cam, W, H) for s in (sc, fresh, sc))
        _start(old).render_pixels(pixels, nsamples=2)
        _start(want).render_pixels(pixels, nsamples=2)
        _start(got)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            sc.update(S2, stream=st)
            got.render_pixels(pixels, nsamples=2, stream=st)
        st.synchronize()
        assert got.same_bits(want) and torch.equal(got.done, want.done)
        assert not got.same_bits(old), "the edit must change the frame"
    finally:
        sc.close()
        fresh.close()


@pytest.mark.parametrize("name", ["cornell", "cloud3000"])
def test_a_captured_call_replays_the_eager_bits(rt, world, monkeypatch, name):
    """One call with `done` and the seeds in place, captured: two replays are
    two eager calls (samples 0-1 and 2-4 of the listed pixels)."""
    import torch
    sc = world[2](name, {}, monkeypatch)
    cam = SCENES[name][1](W, H)
    rng = np.random.default_rng(8)
    pixels = _dev(rng.permutation(W * H)[:600])
    take = _dev(TAKES[rng.integers(0, len(TAKES), 600)])
    eager, frame = rt.SmallptDeviceFrame(sc, cam, W, H), rt.SmallptDeviceFrame(sc, cam, W, H)
    _start(eager)
    _start(frame)
    frame.done                                              # (made before the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        frame.render_pixels(pixels, take)
    _start(frame)
    for _ in range(2):
        eager.render_pixels(pixels, take)
        g.replay()
        torch.cuda.synchronize()
        assert frame.same_bits(eager) and torch.equal(frame.done, eager.done)
    assert int(frame.done.max()) == 2 * int(TAKES.max())
    del g


def test_seventy_calls_capture_into_one_graph(rt, world, monkeypatch):
    """More calls of one scene than it has work-counter entries (64): the
    pixel lists take none.  Call k lists pixel k alone; the replay renders
    the first 70 pixels once."""
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    cam = SCENES["cornell"][1](W, H)
    frame = _start(rt.SmallptDeviceFrame(sc, cam, W, H))
    frame.done
    lists = [_dev([k]) for k in range(70)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for px in lists:
            assert frame.render_pixels(px, nsamples=1) == 0
    g.replay()
    torch.cuda.synchronize()
    totals = np.zeros(W * H, np.int64)
    totals[:70] = 1
    _assert_expected(frame, world[1]("cornell", W, H, 2 * int(TAKES.max()), PT), totals.reshape(H, W), "70 calls")
    del g


# ---- 7. budget maps ----------------------------------------------------------------------------------
def test_budget_list_is_the_map_in_tile_order(rt, world, monkeypatch):
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    cam = SCENES["cornell"][1](W, H)
    frame = _start(rt.SmallptDeviceFrame(sc, cam, W, H))
    budget = TAKES[np.random.default_rng(12).integers(0, len(TAKES), (H, W))]
    for b in (budget, torch.from_numpy(budget.astype(np.int64)), torch.from_numpy(budget).cuda()):
        pixels, take = frame.budget_list(b)
        assert pixels.dtype == take.dtype == torch.int32 and pixels.is_cuda and take.is_cuda
        p, t = pixels.cpu().numpy(), take.cpu().numpy()
        assert len(p) == (budget > 0).sum() == len(set(p)) and (t == budget.reshape(-1)[p]).all() and (t > 0).all()
        x, y = p % W, p // W
        key = ((y // 8) * ((W + 7) // 8) + x // 8) * 64 + (y % 8) * 8 + x % 8
        assert (np.diff(key) > 0).all()                         # tiles row by row, a tile's pixels row by row
    p, t = (v.cpu().numpy() for v in frame.budget_list(budget, order="row"))
    assert (p == np.flatnonzero(budget.reshape(-1))).all() and (t == budget.reshape(-1)[p]).all()
    with pytest.raises(ValueError):
        frame.budget_list(budget, order="column")
    full, _ = frame.budget_list(np.ones((H, W), np.int32))
    assert (full[:64].cpu().numpy() == (np.arange(64) // 8) * W + np.arange(64) % 8).all()
    with pytest.raises(ValueError):
        frame.budget_list(budget[:-1])
    with pytest.raises(ValueError):
        frame.budget_list(budget.astype(np.float32))
    with pytest.raises(ValueError):
        frame.budget_list(budget - 1)
    frame.render_pixels(*frame.budget_list(budget))
    _assert_expected(frame, world[1]("cornell", W, H, 2 * int(TAKES.max()), PT), budget, "budget map")
    frame.reset()
    assert not frame.done.any()


# ---- 8. argument errors --------------------------------------------------------------------------------
def test_argument_errors(rt, world, monkeypatch):
    import ctypes as C
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    w, h = 8, 8
    cam = SCENES["cornell"][1](w, h)
    frame = rt.SmallptDeviceFrame(sc, cam, w, h)
    frame.reset(colors=-7.0, pixels=0xA5A5A5A5, seeds=0x12345678)
    frame.done.fill_(9)
    seeds0 = frame.seeds0.clone()
    pixels, take = _dev(np.arange(16)), _dev(np.ones(16))
    f = rt.lib().spt_scene_render_pixels_async
    ok = dict(scene=sc.handle, camera=C.byref(cam), d_colors=frame.colors.data_ptr(), d_seeds_in=frame.seeds0.data_ptr(),
              d_seeds_out=frame.seeds.data_ptr(), d_pixels=frame.pixels.data_ptr(), w=w, h=h, d_list=pixels.data_ptr(),
              d_take=None, nlist=16, nsamples=1, d_done=None, first_sample=0, mode=PT, stream=None)

    def call(**kw):
        return f(*{**ok, **kw}.values())

    for null in ("scene", "camera", "d_colors", "d_seeds_in", "d_seeds_out", "d_pixels", "d_list"):
        assert call(**{null: None}) == INVALID, null
    assert call(w=0) == INVALID and call(h=0) == INVALID and call(w=-3) == INVALID
    assert call(nsamples=-1) == INVALID and call(first_sample=-1) == INVALID
    assert call(d_take=take.data_ptr(), nsamples=1) == INVALID              # both a take list and nsamples
    assert call(d_done=frame.done.data_ptr(), first_sample=1) == INVALID    # both a count plane and first_sample
    for mode in (2, -1, PT | rt.SPT_COUNT_RAYS, DL | rt.SPT_COST_MAX, PT | rt.SPT_LIST_SET):
        assert call(mode=mode) == INVALID, mode
    assert call(nlist=2 ** 31) == INVALID
    if rt.device_count() > 1:                                               # another current device
        rt.set_device(1)
        try:
            assert call() == INVALID
        finally:
            rt.set_device(0)
    assert call(nlist=0) == 0                                               # nothing to do
    assert frame.render_pixels(pixels[:0], use_done=False) == 0
    torch.cuda.synchronize()
    assert (frame.colors == -7.0).all() and (frame.pixels == rt.device._i32(0xA5A5A5A5)).all()
    assert (frame.seeds == 0x12345678).all() and (frame.done == 9).all() and torch.equal(frame.seeds0, seeds0)
    assert call(d_take=take.data_ptr(), nsamples=0, d_done=frame.done.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (frame.done.cpu().numpy().reshape(h, w)[::-1].reshape(-1)[:16] == 10).all() and int(frame.done.sum()) == 9 * 64 + 16
    with pytest.raises(ValueError):
        frame.render_pixels(pixels.to(torch.int64))
    with pytest.raises(ValueError):
        frame.render_pixels(pixels, take[:5])
    with pytest.raises(ValueError):
        frame.render_pixels(pixels.cpu())
    with pytest.raises(rt.RTError):
        frame.render_pixels(pixels, take, nsamples=2)
    assert frame.render_pixels(pixels, take, nsamples=2, check=False) == INVALID
