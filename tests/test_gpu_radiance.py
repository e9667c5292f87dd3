"""GPU parity of the radiance queries (spt_scene_radiance_async,
csrc/spt_radiance.h) with the oracle, ray by ray and with no tolerance:
radiance as bits, RNG states as integers, every ray compared.  The reference
per ray is tests/radiance_ref.py's 1 x 1 ors_render call (pinned on the CPU by
tests/test_radiance_ref.py).  Covered: every kernel family and hierarchy
layout in both modes, a second light and rays from inside the glass sphere,
batch sizes around the wave size on a one-block grid, several samples per
call, rays that miss, ordering after in-place edits, graph capture, frames
left untouched, equality with the renderer's own frame, argument errors."""
import numpy as np
import pytest

import radiance_ref as rr
import ray_query_ref as rq
import scenes_layouts as sl

pytestmark = pytest.mark.gpu

HOOKS = ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE", "RT_SPT_SCHED", "RT_SPT_DUAL",
         "RT_SPT_QUERY_BLOCKS")
PT, DL = 0, 1                                   # SPT_PATH_TRACING, SPT_DIRECT_LIGHTING
DIFF, SPEC, REFR = 0, 1, 2
TWO_LIGHTS = (3.0, (30.0, 20.0, 90.0), (6.0, 5.0, 4.0), (0.0, 0.0, 0.0), DIFF)   # test_gpu_smallpt_accept.py's row
GLASS = 7                                       # CornellSpheres' REFR sphere


def _clean(monkeypatch, **env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _cornell():
    import rtamd
    return rtamd.scenes.cornell()


def _cornell_two_lights():
    import rtamd
    rows = list(rtamd.scenes._CORNELL) + [TWO_LIGHTS]
    arr = (rtamd.Sphere * len(rows))()
    for s, r in zip(arr, rows):
        rtamd.scenes._sphere(s, *r)
    return arr, len(rows)


def _cornell_camera(w, h):
    import rtamd
    return rtamd.scenes.cornell_camera(w, h)


# name -> (scene, camera, rays, camera grid, reference options)
SCENES = {
    "cornell": (_cornell, _cornell_camera, 1024, (32, 16), {"box": rr.CORNELL_ROOM}),
    "cornell2": (_cornell_two_lights, _cornell_camera, 768, (16, 16),
                 {"box": rr.CORNELL_ROOM, "inside": GLASS, "ninside": 256}),
    "n255": (sl.n255, sl.small_camera, 1024, (32, 16), {}),
    "cloud3000": (lambda: sl.cloud(sl.N_LEAF8), sl.cloud_camera, 1024, (32, 16), {}),
    "cloud30000": (lambda: sl.cloud(sl.N_LEAF12), sl.cloud_camera, 256, (16, 8), {}),
    "cloud43000": (lambda: sl.cloud(sl.N_LEAF16), sl.cloud_camera, 256, (16, 8), {}),
    "cloud56000": (lambda: sl.cloud(sl.N_NOWIDE), sl.cloud_camera, 256, (16, 8), {}),
}

# (scene, creation hooks, family, leaf size)
FAMILIES = [
    pytest.param("cornell", {}, "GEO_LDS", 0, id="lds-cornell"),
    pytest.param("n255", {"RT_SPT_GEO": "global"}, "GEO_GLOBAL", 0, id="global-n255"),
    pytest.param("cloud3000", {"RT_SPT_WIDE": "0"}, "GEO_BVH", 0, id="binary-cloud3000"),
    pytest.param("cloud3000", {}, "GEO_WIDE", 8, id="wide8-cloud3000"),
    pytest.param("cloud30000", {}, "GEO_WIDE", 12, id="wide12-cloud30000"),
    pytest.param("cloud43000", {}, "GEO_WIDE", 16, id="wide16-cloud43000"),
    pytest.param("cloud56000", {}, "GEO_BVH", 0, id="nowide-cloud56000"),
]
MODES = [pytest.param(PT, id="path"), pytest.param(DL, id="direct")]


@pytest.fixture(scope="module")
def world(rt):
    """spheres(name) -> (S, n); ref(name, mode) -> rr.reference's two samples,
    computed once and read-only; scene(name, env, monkeypatch) -> a prepared
    SmallptScene, kept for the module."""
    sph, refs, scenes = {}, {}, {}

    def spheres(name):
        if name not in sph:
            sph[name] = SCENES[name][0]()
        return sph[name]

    def ref(name, mode):
        if (name, mode) not in refs:
            S, n = spheres(name)
            _, cam, count, grid, opts = SCENES[name]
            refs[(name, mode)] = rr.reference(S, n, cam, grid, count, mode, **opts)
        return refs[(name, mode)]

    def scene(name, env, monkeypatch):
        key = (name, tuple(sorted(env.items())))
        _clean(monkeypatch, **env)
        if key not in scenes:
            scenes[key] = rt.SmallptScene(*spheres(name))
        return scenes[key]

    yield spheres, ref, scene
    for sc in scenes.values():
        sc.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _bits(x):
    """A device tensor as uint32 on the host."""
    import torch
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _assert_same(out, seeds, col, seeds_ref, what=""):
    got, gs = _bits(out), _bits(seeds)
    bad = np.flatnonzero((got != col.view(np.uint32)).any(axis=1) | (gs != seeds_ref).any(axis=1))
    assert len(bad) == 0, "%s: %d of %d rays differ, first %d: got %r %r want %r %r" % (
        what, len(bad), len(col), bad[0], got[bad[0]].view(np.float32), gs[bad[0]], col[bad[0]], seeds_ref[bad[0]])


def _two_samples(sc, ref, mode, what):
    """Two successive single-sample calls, the host drawing the camera's
    jitter from the returned states in between; each compared with the oracle."""
    out, after = None, ref[0]["seeds_in"]
    for k, step in enumerate(ref):
        out, so = sc.radiance(_dev(step["rays"]), _dev(after), 1, k, mode, out=out)
        _assert_same(out, so, step["col"], step["seeds_out"], "%s sample %d" % (what, k))
        after = rr.after_jitter(_bits(so))[0]


# ---- 1. every family, both modes --------------------------------------------------
def _cornell_coverage(S, n, ref):
    """What the Cornell set must exercise, read from the oracle's counters and
    outputs (and the first hits from the full-scan restatement)."""
    rows = sl.rows_of(S, n)
    cnt = sum(step["cnt"].sum(axis=0) for step in ref)
    assert cnt[1] > 0                                           # IntersectP calls: shadow rays were traced
    assert cnt[0] >= 3 * cnt[3]                                 # Intersect calls >= 3 x samples: paths bounce
    first = rq.scan(S, n, ref[0]["rays"])["nearest"][1]
    hit = first >= 0
    emits = (rows[first, 4] != 0) | (rows[first, 6] != 0)       # viszero (vec.h: x and z)
    refl = rows[first, 10].view(np.int32)
    for kind in (DIFF, SPEC, REFR):
        assert (hit & ~emits & (refl == kind)).any(), kind
    assert (hit & emits).any()
    assert (ref[0]["col"] == 0).all(axis=1).any()               # a zero-radiance ray


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,env,family,leaf", FAMILIES)
def test_radiance_equals_oracle(world, monkeypatch, name, env, family, leaf, mode):
    sc = world[2](name, env, monkeypatch)
    info = sc.info()
    assert info["family"] == family and info["leaf_max"] == leaf, info
    ref = world[1](name, mode)
    if name == "cornell" and mode == PT:
        _cornell_coverage(*world[0](name), ref)
    assert (ref[1]["col"] != 0).any(axis=1).sum() > len(ref[1]["col"]) // 8        # light arrives along many rays
    _two_samples(sc, ref, mode, name)


# ---- 2. a second light, rays from inside the glass -----------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_two_lights_and_rays_from_inside_glass(world, monkeypatch, mode):
    """Cornell plus a second emitter (SampleLights' loop takes two turns per
    DIFF vertex); a third of the rays start inside the glass sphere with
    uniform directions, so they leave it by refraction, by reflection (both
    outcomes of the roulette) and, past the critical angle, by total internal
    reflection."""
    sc = world[2]("cornell2", {}, monkeypatch)
    assert sc.info()["nlights"] == 2
    ref = world[1]("cornell2", mode)
    S, n = world[0]("cornell2")
    inside = ref[0]["rays"][-256:]
    assert (rq.scan(S, n, inside)["nearest"][1] == GLASS).all()  # their first hit is the glass, from within
    _two_samples(sc, ref, mode, "cornell2")


# ---- 3. chunk edges and grid wrap ------------------------------------------------------
def test_batch_sizes_on_a_one_block_grid(world, monkeypatch):
    """1, 63, 64, 65 and 257 rays with the grid capped at one block (257 rays:
    five chunks on four waves, so a wave takes a second one): each ray's result
    does not depend on its batch, and nothing is written past the batch."""
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    step = world[1]("cornell", PT)[0]
    monkeypatch.setenv("RT_SPT_QUERY_BLOCKS", "1")
    for count in (1, 63, 64, 65, 257):
        out = torch.full((count + 64, 3), -7.0, dtype=torch.float32, device="cuda")
        so = torch.full((count + 64, 2), -7, dtype=torch.int32, device="cuda")
        sc.radiance(_dev(step["rays"][:count]), _dev(step["seeds_in"][:count]), out=out[:count], seeds_out=so[:count])
        _assert_same(out[:count], so[:count], step["col"][:count], step["seeds_out"][:count], "x %d" % count)
        assert (out[count:].cpu().numpy() == -7.0).all() and (so[count:].cpu().numpy() == -7).all()
    e = torch.empty((0, 6), dtype=torch.float32, device="cuda")
    out, so = sc.radiance(e, torch.empty((0, 2), dtype=torch.int32, device="cuda"))
    assert out.shape == (0, 3) and so.shape == (0, 2)


# ---- 4. samples in one call -------------------------------------------------------------
@pytest.mark.parametrize("name,env", [("cornell", {}), ("cloud3000", {}), ("cloud3000", {"RT_SPT_WIDE": "0"})],
                         ids=["cornell", "cloud3000-wide", "cloud3000-binary"])
@pytest.mark.parametrize("mode", MODES)
def test_samples_in_one_call(world, monkeypatch, name, env, mode):
    import torch
    sc = world[2](name, env, monkeypatch)
    S, n = world[0](name)
    step = world[1](name, mode)[0]
    rays, s0 = _dev(step["rays"]), _dev(step["seeds_in"])
    # four calls of one sample, the states carried in place
    out1 = torch.zeros((len(step["rays"]), 3), dtype=torch.float32, device="cuda")
    s1 = s0.clone()
    for k in range(4):
        sc.radiance(rays, s1, 1, k, mode, out=out1, seeds_out=s1)
    # one call of four, distinct seed buffers
    out4, s4 = sc.radiance(rays, s0, 4, 0, mode)
    assert torch.equal(s0, _dev(step["seeds_in"]))              # the input states are only read
    assert (_bits(out4) == _bits(out1)).all() and (_bits(s4) == _bits(s1)).all()
    assert (_bits(s4) != _bits(s0)).any()
    # ... and aliased ones
    s4a = s0.clone()
    out4a, _ = sc.radiance(rays, s4a, 4, 0, mode, seeds_out=s4a)
    assert (_bits(out4a) == _bits(out4)).all() and (_bits(s4a) == _bits(s4)).all()
    # first_sample = 5 continues an accumulator: two samples at once = one by one
    acc = torch.from_numpy(np.random.default_rng(3).uniform(0, 2, (len(step["rays"]), 3)).astype(np.float32)).cuda()
    a2, sa2 = sc.radiance(rays, s0, 2, 5, mode, out=acc.clone())
    a1, sa1 = sc.radiance(rays, s0, 1, 5, mode, out=acc.clone())
    first = a1.clone()
    sc.radiance(rays, sa1, 1, 6, mode, out=a1, seeds_out=sa1)
    assert (_bits(a2) == _bits(a1)).all() and (_bits(sa2) == _bits(sa1)).all()
    # ... and is the oracle's sample 5 on that accumulator (the first 128 rays)
    m = 128
    D, O = step["pairs"]
    col, _, _ = rr.oracle_sample(S, n, D[:m], O[:m], step["seeds_before"][:m], acc.cpu().numpy()[:m], 5, mode)
    assert (_bits(first)[:m] == col.view(np.uint32)).all() and (_bits(first) != _bits(acc)).any()
    # nsamples = 0: the seeds are copied, the radiance is left alone
    out0 = torch.full((len(step["rays"]), 3), -7.0, dtype=torch.float32, device="cuda")
    _, sz = sc.radiance(rays, s0, 0, 0, mode, out=out0)
    assert torch.equal(sz, s0) and (out0.cpu().numpy() == -7.0).all()


# ---- 5. rays that miss -------------------------------------------------------------------
@pytest.mark.parametrize("name,env", [("cornell", {}), ("n255", {"RT_SPT_GEO": "global"}), ("cloud3000", {}),
                                      ("cloud3000", {"RT_SPT_WIDE": "0"})],
                         ids=["cornell", "n255-global", "cloud3000-wide", "cloud3000-binary"])
def test_missing_rays_return_zeros_and_draw_nothing(world, monkeypatch, name, env):
    """Every ray of the query tests' mix (|d| = 2, d = 0, axis-aligned, ...)
    and of the non-finite set that query("nearest") reports as a miss: zeros,
    the states unchanged -- in a batch with ordinary rays that hit."""
    import torch
    sc = world[2](name, env, monkeypatch)
    S, n = world[0](name)
    cand = np.concatenate([rq.ray_set(S, n, SCENES[name][1], 2048)[0], rq.non_finite_rays(S, n, 256),
                           np.array([[0, 0, 0, 0, 0, 0], [1e30, 0, 0, 1, 0, 0]], np.float32)])
    _, ids = sc.query(_dev(cand))
    miss = cand[ids.cpu().numpy() < 0]
    assert (~np.isfinite(miss)).any(axis=1).sum() >= 256 and np.isfinite(miss).all(axis=1).sum() > 50
    assert (np.abs(np.linalg.norm(miss[np.isfinite(miss).all(axis=1), 3:], axis=1) - 2.0) < 1e-3).any()   # |d| = 2
    step = world[1](name, PT)[0]
    rays = np.concatenate([miss, step["rays"][:192]])
    order = np.random.default_rng(9).permutation(len(rays))     # misses and hits side by side in a wave
    rays, is_miss = rays[order], (np.arange(len(rays)) < len(miss))[order]
    seeds = rr.seeds_for(len(rays), seed=4)
    for mode in (PT, DL):
        out = torch.full((len(rays), 3), -7.0, dtype=torch.float32, device="cuda")
        out, so = sc.radiance(_dev(rays), _dev(seeds), 2, 0, mode, out=out)
        got, gs = out.cpu().numpy(), _bits(so)
        assert (got[is_miss].view(np.uint32) == 0).all()        # +0.0, not -0.0
        assert (gs[is_miss] == seeds[is_miss]).all()
        assert (gs[~is_miss] != seeds[~is_miss]).any() and (got[~is_miss] != -7.0).all()


# ---- 6. ordering, capture, frames -----------------------------------------------------------
def _moved(rows, seed):
    """A tenth of the spheres (never the first four: ground and lights) moved
    by up to 3 % of the cloud's extent."""
    rng = np.random.default_rng(seed)
    n = len(rows)
    out = rows.copy()
    pick = 4 + rng.choice(n - 4, n // 10, replace=False)
    ext = float(np.ptp(rows[4:, 1:4], axis=0).max())
    out[pick, 1:4] += rng.uniform(-0.03 * ext, 0.03 * ext, (len(pick), 3)).astype(np.float32)
    return out


@pytest.mark.parametrize("name,env,family", [("cloud3000", {}, "GEO_WIDE"), ("cloud3000", {"RT_SPT_WIDE": "0"}, "GEO_BVH"),
                                             ("n255", {}, "GEO_LDS")],
                         ids=["cloud3000-wide", "cloud3000-binary", "n255"])
def test_radiance_after_update_sees_the_edited_spheres(rt, world, monkeypatch, name, env, family):
    """update() then radiance() on one stream, nothing in between: the results
    of a scene created from the edited array (and not the old ones)."""
    import torch
    _clean(monkeypatch, **env)
    rows = sl.cloud_rows(sl.N_LEAF8) if name == "cloud3000" else sl.cloud_rows(256, 7, sl._SMALL_HALF, sl._SMALL_EXP)[:255]
    step = world[1](name, PT)[0]
    rays, seeds = _dev(step["rays"]), _dev(step["seeds_in"])
    S, n = sl.pack(rows)
    S2, _ = sl.pack(_moved(rows, 1))
    sc, fresh = rt.SmallptScene(S, n), rt.SmallptScene(S2, n)
    try:
        assert sc.info()["family"] == family == fresh.info()["family"]
        old = sc.radiance(rays, seeds, 2)
        want = fresh.radiance(rays, seeds, 2)
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            sc.update(S2, stream=st)
            got = sc.radiance(rays, seeds, 2, stream=st)
        st.synchronize()
        assert (_bits(got[0]) == _bits(want[0])).all() and (_bits(got[1]) == _bits(want[1])).all()
        assert (_bits(got[0]) != _bits(old[0])).any(axis=1).sum() > 10, "the edit must change some results"
    finally:
        sc.close()
        fresh.close()


@pytest.mark.parametrize("name", ["cornell", "cloud3000"])
def test_captured_calls_replay_the_eager_bits(world, monkeypatch, name):
    """Two calls (samples 0 and 1, the states carried in place) captured into
    one graph: a replay on fresh inputs gives the eager calls' bits."""
    import torch
    sc = world[2](name, {}, monkeypatch)
    step = world[1](name, PT)[0]
    rays = _dev(step["rays"])
    s_eager = _dev(step["seeds_in"])
    out_eager = torch.zeros((len(step["rays"]), 3), dtype=torch.float32, device="cuda")
    for k in (0, 1):
        sc.radiance(rays, s_eager, 1, k, out=out_eager, seeds_out=s_eager)
    s = torch.zeros_like(s_eager)
    out = torch.zeros_like(out_eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for k in (0, 1):
            sc.radiance(rays, s, 1, k, out=out, seeds_out=s)
    for _ in range(2):
        s.copy_(_dev(step["seeds_in"]))
        out.fill_(-7.0)
        g.replay()
        torch.cuda.synchronize()
        assert (_bits(out) == _bits(out_eager)).all() and (_bits(s) == _bits(s_eager)).all()
    del g


@pytest.mark.parametrize("name,env", [("cornell", {}), ("cloud3000", {}), ("cloud3000", {"RT_SPT_WIDE": "0"})],
                         ids=["cornell", "cloud3000-wide", "cloud3000-binary"])
def test_frame_is_untouched_by_radiance_calls(rt, world, monkeypatch, name, env):
    """1 spp before and after radiance calls in both modes on the same scene: equal bits."""
    sc = world[2](name, env, monkeypatch)
    w, h = 64, 48
    frame = rt.SmallptDeviceFrame(sc, SCENES[name][1](w, h), w, h)
    frame.reset().render(1)
    before = [a.copy() for a in frame.host()]
    step = world[1](name, PT)[0]
    for mode in (PT, DL):
        sc.radiance(_dev(step["rays"]), _dev(step["seeds_in"]), 2, 0, mode)
    frame.reset().render(1)
    after = frame.host()
    assert (before[0].view(np.uint32) == after[0].view(np.uint32)).all()
    assert (before[1] == after[1]).all() and (before[2] == after[2]).all()
    assert before[2].any()


# ---- 7. against the renderer -------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_jittered_camera_rays_give_the_rendered_frame(rt, world, monkeypatch, mode):
    """Cornell 64 x 48 at sample 0: the radiance along every pixel's jittered
    camera ray, the jitter drawn on the host from the frame's initial seeds,
    is SmallptDeviceFrame.render(1)'s colour in the pixel's flipped slot, and
    the states are the frame's."""
    sc = world[2]("cornell", {}, monkeypatch)
    w, h = 64, 48
    cam = rt.scenes.cornell_camera(w, h)
    frame = rt.SmallptDeviceFrame(sc, cam, w, h)
    frame.reset().render(1, mode=mode)
    col, seeds, _ = frame.host()
    i = np.arange(w * h)
    x, y = i % w, h - 1 - i // w                                # slot i = (h - y - 1) * w + x
    after, r1, r2 = rr.after_jitter(rt.scenes.seeds(w, h).reshape(-1, 2))
    rays = rt.scenes.camera_rays(cam, w, h, x, y, r1, r2)
    out, so = sc.radiance(_dev(rays), _dev(after), 1, 0, mode)
    _assert_same(out, so, col.reshape(-1, 3), seeds.reshape(-1, 2), "frame")


# ---- 8. argument errors ----------------------------------------------------------------------------
def test_argument_errors(rt, world, monkeypatch):
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    f = rt.lib().spt_scene_radiance_async
    step = world[1]("cornell", PT)[0]
    rays, seeds = _dev(step["rays"][:4]), _dev(step["seeds_in"][:4])
    out = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    so = torch.full((4, 2), -7, dtype=torch.int32, device="cuda")
    h, r, s, o, p = sc.handle, rays.data_ptr(), seeds.data_ptr(), so.data_ptr(), out.data_ptr()
    INVALID = -1
    assert f(None, r, 4, s, o, p, 0, 1, PT, None) == INVALID            # null scene
    assert f(h, None, 4, s, o, p, 0, 1, PT, None) == INVALID            # null rays
    assert f(h, r, 4, None, o, p, 0, 1, PT, None) == INVALID            # null seeds
    assert f(h, r, 4, s, None, p, 0, 1, PT, None) == INVALID
    assert f(h, r, 4, s, o, None, 0, 1, PT, None) == INVALID            # null radiance
    assert f(h, r, 4, s, o, p, 0, -1, PT, None) == INVALID              # negative nsamples
    assert f(h, r, 4, s, o, p, -1, 1, PT, None) == INVALID              # negative first_sample
    assert f(h, r, 4, s, o, p, 0, 1, 2, None) == INVALID                # unknown mode
    assert f(h, r, 4, s, o, p, 0, 1, -1, None) == INVALID
    assert f(h, r, 4, s, o, p, 0, 1, PT | rt.SPT_COUNT_RAYS, None) == INVALID   # flag bits
    assert f(h, r, 4, s, o, p, 0, 1, DL | rt.SPT_COST_MAX, None) == INVALID
    assert f(h, r, 2 ** 31, s, o, p, 0, 1, PT, None) == INVALID         # above INT32_MAX
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (so.cpu().numpy() == -7).all()
    assert f(h, r, 0, s, o, p, 0, 1, PT, None) == 0                     # nothing to do
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (so.cpu().numpy() == -7).all()
    assert f(h, r, 4, s, o, p, 0, 1, PT, None) == 0
    _assert_same(out, so, step["col"][:4], step["seeds_out"][:4], "raw call")
    with pytest.raises(ValueError):
        sc.radiance(rays[:, :5].contiguous(), seeds)
    with pytest.raises(ValueError):
        sc.radiance(rays, seeds.view(torch.float32))                    # dtype
    with pytest.raises(ValueError):
        sc.radiance(rays, seeds[:3])                                    # shape
    with pytest.raises(ValueError):
        sc.radiance(rays, seeds.t().contiguous().t())                   # contiguity
    with pytest.raises(ValueError):
        sc.radiance(rays, seeds, out=out.double())
    with pytest.raises(ValueError):
        sc.radiance(rays, seeds, first_sample=3)                        # nothing to continue
    with pytest.raises(ValueError):
        sc.radiance(rays, seeds, nsamples=-1)
