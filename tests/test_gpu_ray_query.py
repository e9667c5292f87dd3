"""GPU parity of the ray queries (spt_scene_query_async, csrc/spt_query.h)
with the numpy restatement of the reference's full scan
(tests/ray_query_ref.py), ray by ray and with no tolerance: t as bits, id as
integers -- on every kernel family and hierarchy layout the library picks,
after in-place edits, from a captured graph, at batch sizes around the wave
size, with every output combination; and a frame is the same before and
after queries.  Test rays are the mix of ray_query_ref.ray_set."""
import numpy as np
import pytest

import ray_query_ref as rq
import scenes_layouts as sl

pytestmark = pytest.mark.gpu

HOOKS = ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE", "RT_SPT_SCHED", "RT_SPT_DUAL",
         "RT_SPT_QUERY_BLOCKS")


def _clean(monkeypatch, **env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _cornell():
    import rtamd
    return rtamd.scenes.cornell()


def _cornell_camera(w, h):
    import rtamd
    return rtamd.scenes.cornell_camera(w, h)


# name -> (scene, camera, centres the ray set also aims at)
SCENES = {
    "cornell": (_cornell, _cornell_camera, ()),
    "n255": (sl.n255, sl.small_camera, ()),
    "cloud3000": (lambda: sl.cloud(sl.N_LEAF8), sl.cloud_camera, ()),
    "cloud30000": (lambda: sl.cloud(sl.N_LEAF12), sl.cloud_camera, ()),
    "cloud43000": (lambda: sl.cloud(sl.N_LEAF16), sl.cloud_camera, ()),
    "cloud56000": (lambda: sl.cloud(sl.N_NOWIDE), sl.cloud_camera, ()),
    "no_always": (sl.EDGE_SCENES["no_always"][0], sl.EDGE_SCENES["no_always"][1], ()),
    "many_always": (sl.EDGE_SCENES["many_always"][0], sl.EDGE_SCENES["many_always"][1], ()),
    "n256": (sl.EDGE_SCENES["n256"][0], sl.EDGE_SCENES["n256"][1], ()),
    "coincident": (sl.EDGE_SCENES["coincident"][0], sl.EDGE_SCENES["coincident"][1],
                   (sl.COINCIDENT_DUPE[:3], sl.COINCIDENT_CENTRE)),
}
NRAYS = {"cloud30000": 1024, "cloud43000": 1024, "cloud56000": 1024}

# (scene, creation hooks, family, leaf size)
FAMILIES = [
    pytest.param("cornell", {}, "GEO_LDS", 0, id="lds-cornell"),
    pytest.param("n255", {}, "GEO_LDS", 0, id="lds-n255"),
    pytest.param("n255", {"RT_SPT_GEO": "global"}, "GEO_GLOBAL", 0, id="global-n255"),
    pytest.param("cloud3000", {"RT_SPT_WIDE": "0"}, "GEO_BVH", 0, id="binary-cloud3000"),
    pytest.param("cloud3000", {}, "GEO_WIDE", 8, id="wide8-cloud3000"),
    pytest.param("cloud30000", {}, "GEO_WIDE", 12, id="wide12-cloud30000"),
    pytest.param("cloud43000", {}, "GEO_WIDE", 16, id="wide16-cloud43000"),
    pytest.param("cloud56000", {}, "GEO_BVH", 0, id="nowide-cloud56000"),
    pytest.param("no_always", {}, "GEO_WIDE", 8, id="edge-no_always"),
    pytest.param("many_always", {}, "GEO_WIDE", 8, id="edge-many_always"),
    pytest.param("n256", {}, "GEO_WIDE", 8, id="edge-n256"),
    pytest.param("coincident", {}, "GEO_WIDE", 8, id="edge-coincident"),
]


@pytest.fixture(scope="module")
def world(rt):
    """spheres(name) -> (S, n); rays(name, count) -> (rays, tmax, expected of
    rq.scan with that tmax), computed once and read-only; scene(name, env,
    monkeypatch) -> a prepared SmallptScene, kept for the module."""
    import torch  # noqa: F401
    sph, sets, scenes = {}, {}, {}

    def spheres(name):
        if name not in sph:
            sph[name] = SCENES[name][0]()
        return sph[name]

    def rays(name, count=None):
        count = count or NRAYS.get(name, 2048)
        if (name, count) not in sets:
            S, n = spheres(name)
            r, tm = rq.ray_set(S, n, SCENES[name][1], count, aim=SCENES[name][2])
            sets[(name, count)] = (r, tm, rq.scan(S, n, r, tm))
        return sets[(name, count)]

    def scene(name, env, monkeypatch):
        key = (name, tuple(sorted(env.items())))
        _clean(monkeypatch, **env)
        if key not in scenes:
            scenes[key] = rt.SmallptScene(*spheres(name))
        return scenes[key]

    yield spheres, rays, scene
    for sc in scenes.values():
        sc.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(x):
    return None if x is None else x.cpu().numpy()


def _run(sc, rays, tmax, kind, **kw):
    t, ids = sc.query(_dev(rays), None if tmax is None else _dev(tmax), kind=kind, **kw)
    return _host(t), _host(ids)


def _assert_same(got, ref, kind, what=""):
    t, ids = got
    if kind == "nearest":
        rt_, ri = ref["nearest"]
        bad = np.flatnonzero((ids != ri) | (t.view(np.uint32) != rt_.view(np.uint32)))
        assert len(bad) == 0, "%s nearest: %d of %d rays differ, first %d: got (%r, %d) want (%r, %d)" % (
            what, len(bad), len(ids), bad[0], t[bad[0]], ids[bad[0]], rt_[bad[0]], ri[bad[0]])
    else:
        assert t is None
        bad = np.flatnonzero(ids != ref[kind])
        assert len(bad) == 0, "%s %s: %d of %d rays differ, first %d: got %d want %d" % (
            what, kind, len(bad), len(ids), bad[0], ids[bad[0]], ref[kind][bad[0]])


# ---- 1. every family, every kind ------------------------------------------------
@pytest.mark.parametrize("kind", rq.KINDS)
@pytest.mark.parametrize("name,env,family,leaf", FAMILIES)
def test_query_equals_full_scan(world, monkeypatch, name, env, family, leaf, kind):
    """The family the scene runs answers every ray of the mix as the full
    scan does; the mix holds hits, misses and occluded rays on this scene."""
    sc = world[2](name, env, monkeypatch)
    info = sc.info()
    assert info["family"] == family and info["leaf_max"] == leaf, info
    rays, tmax, ref = world[1](name)
    hits = ref["nearest"][1] >= 0
    assert 100 < hits.sum() < len(rays) - 100 and ref["any"].sum() > 100
    _assert_same(_run(sc, rays, tmax, kind), ref, kind, name)
    if name == "coincident" and kind == "nearest":
        ids = ref["nearest"][1]
        on = np.isin(ids, sl.COINCIDENT_DUPES)
        assert on.sum() > 100 and (ids[on] == sl.COINCIDENT_DUPES[-1]).all()       # the tie's highest index
        assert np.isin(ids, sl.COINCIDENT_SHARED).sum() > 50


@pytest.mark.parametrize("name,env", [("cornell", {}), ("cloud3000", {}), ("cloud3000", {"RT_SPT_WIDE": "0"})],
                         ids=["cornell", "cloud3000-wide", "cloud3000-binary"])
def test_nearest_without_tmax_is_intersect(world, monkeypatch, name, env):
    """tmax = None: the bound 1e20f of Intersect, returned on a miss."""
    sc = world[2](name, env, monkeypatch)
    rays, _, _ = world[1](name)
    S, n = world[0](name)
    ref = rq.scan(S, n, rays)
    t, ids = _run(sc, rays, None, "nearest")
    _assert_same((t, ids), ref, "nearest", name)
    assert (t[ids < 0] == np.float32(1e20)).all() and (ids < 0).sum() > 50


@pytest.mark.parametrize("name,env", [("cornell", {}), ("n255", {"RT_SPT_GEO": "global"}), ("cloud3000", {}),
                                      ("cloud3000", {"RT_SPT_WIDE": "0"}), ("coincident", {})],
                         ids=["cornell", "n255-global", "cloud3000-wide", "cloud3000-binary", "coincident"])
def test_bound_is_strict(world, monkeypatch, name, env):
    """A bound equal to the nearest distance itself rejects that sphere (d <
    bound, strictly: every kind reports what lies nearer -- nothing); the next
    float above it accepts it again, ties still to the highest index."""
    sc = world[2](name, env, monkeypatch)
    rays, _, _ = world[1](name)
    S, n = world[0](name)
    t0, i0 = rq.scan(S, n, rays)["nearest"]
    hit = np.flatnonzero(i0 >= 0)
    assert len(hit) > 300
    rays, t0, i0 = rays[hit], t0[hit], i0[hit]
    for bound, same in ((t0, False), (np.nextafter(t0, np.float32(np.inf)), True)):
        ref = rq.scan(S, n, rays, bound)
        assert ((ref["nearest"][1] == i0) == same).all() and ((ref["occluder"] >= 0) == same).all()
        for kind in rq.KINDS:
            _assert_same(_run(sc, rays, bound, kind), ref, kind, name)


# ---- 2. batch sizes ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "cloud3000"])
def test_batch_sizes(world, monkeypatch, name):
    """1, 63, 64, 65 and 257 rays, and 4,097 on a grid capped at two blocks
    (several rounds per block): each ray's answer does not depend on the batch
    it came in, and nothing is written past the batch."""
    import torch
    sc = world[2](name, {}, monkeypatch)
    rays, tmax, ref = world[1](name, 4097)
    for count, blocks in ((1, None), (63, None), (64, None), (65, None), (257, None), (4097, "2")):
        if blocks:
            monkeypatch.setenv("RT_SPT_QUERY_BLOCKS", blocks)
        sub = {"nearest": (ref["nearest"][0][:count], ref["nearest"][1][:count]), "any": ref["any"][:count],
               "occluder": ref["occluder"][:count]}
        for kind in rq.KINDS:
            # outputs with a guard row behind the batch
            t = torch.full((count + 64,), -7.0, dtype=torch.float32, device="cuda")
            ids = torch.full((count + 64,), -7, dtype=torch.int32, device="cuda")
            sc.query(_dev(rays[:count]), _dev(tmax[:count]), kind=kind, out=(t[:count], ids[:count]))
            got = (_host(t[:count]) if kind == "nearest" else None, _host(ids[:count]))
            _assert_same(got, sub, kind, "%s x %d" % (name, count))
            assert (_host(t[count:]) == -7.0).all() and (_host(ids[count:]) == -7).all()
            if kind != "nearest":
                assert (_host(t) == -7.0).all()                 # d_t is not written
    # no rays: RT_OK, nothing launched
    e = torch.empty((0, 6), dtype=torch.float32, device="cuda")
    t, ids = sc.query(e)
    assert t.numel() == 0 and ids.numel() == 0


# ---- 3. after in-place edits -------------------------------------------------------
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
def test_query_after_update_sees_the_edited_spheres(rt, monkeypatch, name, env, family):
    """update() then query() on one stream, nothing in between: the answers
    are the full scan's of the edited array (and differ from the old ones)."""
    import torch
    _clean(monkeypatch, **env)
    rows = sl.cloud_rows(sl.N_LEAF8) if name == "cloud3000" else sl.cloud_rows(256, 7, sl._SMALL_HALF, sl._SMALL_EXP)[:255]
    S, n = sl.pack(rows)
    cam = sl.cloud_camera if name == "cloud3000" else sl.small_camera
    rays, tmax = rq.ray_set(S, n, cam, 2048, seed=3)
    old = rq.scan(S, n, rays, tmax)
    sc = rt.SmallptScene(S, n)
    try:
        assert sc.info()["family"] == family
        st = torch.cuda.Stream()
        d_rays, d_tmax = _dev(rays), _dev(tmax)
        torch.cuda.synchronize()
        for step in (1, 2):
            rows = _moved(rows, step)
            S2, _ = sl.pack(rows)
            got = {}
            with torch.cuda.stream(st):
                sc.update(S2, stream=st)
                for kind in rq.KINDS:
                    got[kind] = sc.query(d_rays, d_tmax, kind=kind, stream=st)
            st.synchronize()
            ref = rq.scan(S2, n, rays, tmax)
            for kind in rq.KINDS:
                _assert_same((_host(got[kind][0]), _host(got[kind][1])), ref, kind, "%s step %d" % (name, step))
            assert (ref["nearest"][1] != old["nearest"][1]).sum() > 10, "the edit must change some answers"
        assert sc.update_info()["updates"] == 2
    finally:
        sc.close()


# ---- 4. graph capture -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "cloud3000"])
def test_captured_query_replays_with_new_rays(world, monkeypatch, name):
    """One query captured into a graph; two replays, each after new ray
    contents were copied into the captured tensors."""
    import torch
    sc = world[2](name, {}, monkeypatch)
    rays, tmax, ref = world[1](name)
    S, n = world[0](name)
    count = 1000
    d_rays = torch.zeros((count, 6), dtype=torch.float32, device="cuda")
    d_tmax = torch.full((count,), 1e20, dtype=torch.float32, device="cuda")
    t = torch.zeros(count, dtype=torch.float32, device="cuda")
    ids = torch.zeros(count, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        sc.query(d_rays, d_tmax, kind="nearest", out=(t, ids))
    for lo in (0, 1000):
        d_rays.copy_(_dev(rays[lo:lo + count]))
        d_tmax.copy_(_dev(tmax[lo:lo + count]))
        t.fill_(-7.0)
        ids.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        sub = {"nearest": (ref["nearest"][0][lo:lo + count], ref["nearest"][1][lo:lo + count])}
        _assert_same((_host(t), _host(ids)), sub, "nearest", "%s replay at %d" % (name, lo))
    del g


# ---- 5. outputs and errors ------------------------------------------------------------
def test_output_combinations(world, monkeypatch):
    import torch
    sc = world[2]("cloud3000", {}, monkeypatch)
    rays, tmax, ref = world[1]("cloud3000")
    d_rays, d_tmax = _dev(rays), _dev(tmax)
    n = len(rays)
    t = torch.full((n,), -7.0, dtype=torch.float32, device="cuda")
    ids = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    rt_, ri = ref["nearest"]
    got = sc.query(d_rays, d_tmax, out=(t, None))
    assert got[1] is None and (_host(t).view(np.uint32) == rt_.view(np.uint32)).all() and (_host(ids) == -7).all()
    t.fill_(-7.0)
    got = sc.query(d_rays, d_tmax, out=(None, ids))
    assert got[0] is None and (_host(ids) == ri).all() and (_host(t) == -7.0).all()
    for kind in ("any", "occluder"):
        ids.fill_(-7)
        got = sc.query(d_rays, d_tmax, kind=kind, out=(t, ids))
        assert got[0] is None and (_host(ids) == ref[kind]).all() and (_host(t) == -7.0).all()


def test_argument_errors(rt, world, monkeypatch):
    import torch
    sc = world[2]("cornell", {}, monkeypatch)
    q = rt.lib().spt_scene_query_async
    rays = torch.zeros((4, 6), dtype=torch.float32, device="cuda")
    rays[:, 2] = 1e6                                                    # outside every sphere, direction zero
    tmax = torch.ones(4, dtype=torch.float32, device="cuda")
    t = torch.zeros(4, dtype=torch.float32, device="cuda")
    ids = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    h, r, m, pt, pi = sc.handle, rays.data_ptr(), tmax.data_ptr(), t.data_ptr(), ids.data_ptr()
    INVALID = -1
    assert q(None, r, m, 4, 0, pt, pi, None) == INVALID                 # null scene
    assert q(h, None, m, 4, 0, pt, pi, None) == INVALID                 # null rays
    assert q(h, r, m, 4, 0, None, None, None) == INVALID                # no output
    assert q(h, r, None, 4, 1, None, pi, None) == INVALID               # any-hit needs tmax
    assert q(h, r, None, 4, 2, None, pi, None) == INVALID
    assert q(h, r, m, 4, 1, pt, None, None) == INVALID                  # ... and d_id, the one output it writes
    assert q(h, r, m, 4, 3, pt, pi, None) == INVALID                    # unknown kind
    assert q(h, r, m, 4, -1, pt, pi, None) == INVALID
    assert q(h, r, m, 2 ** 31, 0, pt, pi, None) == INVALID              # above INT32_MAX
    torch.cuda.synchronize()
    assert (_host(ids) == -7).all()
    assert q(h, r, m, 0, 0, pt, pi, None) == 0                          # nothing to do
    assert q(h, r, None, 4, 0, pt, pi, None) == 0                       # nearest without tmax
    torch.cuda.synchronize()
    assert (_host(ids) == -1).all() and (_host(t) == np.float32(1e20)).all()   # a zero direction from outside: misses
    with pytest.raises(ValueError):
        sc.query(rays, kind="first")
    with pytest.raises(ValueError):
        sc.query(rays[:, :5])
    with pytest.raises(rt.RTError):
        sc.query(rays, kind="any")                                      # tmax missing


# ---- 6. picking, and frames ------------------------------------------------------------
def test_pick_returns_the_pixels_first_hit(rt, world, monkeypatch):
    sc = world[2]("cornell", {}, monkeypatch)
    S, n = world[0]("cornell")
    w, h = 64, 48
    cam = rt.scenes.cornell_camera(w, h)
    ref = rq.scan(S, n, rt.scenes.camera_rays(cam, w, h))["nearest"]
    for x, y in ((w // 2, h // 2), (0, 0), (w - 1, h - 1), (20, 30)):
        i, t = sc.pick(cam, w, h, x, y)
        assert i == ref[1][y * w + x] and np.float32(t) == ref[0][y * w + x]
    assert sc.pick(cam, w, h, w // 2, h // 2)[0] == 2
    with pytest.raises(ValueError):
        sc.pick(cam, w, h, w, 0)


@pytest.mark.parametrize("name,env", [("cornell", {}), ("cloud3000", {}), ("cloud3000", {"RT_SPT_WIDE": "0"})],
                         ids=["cornell", "cloud3000-wide", "cloud3000-binary"])
def test_frame_is_untouched_by_queries(rt, world, monkeypatch, name, env):
    """1 spp before and after a query of each kind on the same scene: equal bits."""
    sc = world[2](name, env, monkeypatch)
    w, h = 64, 48
    frame = rt.SmallptDeviceFrame(sc, SCENES[name][1](w, h), w, h)
    frame.reset().render(1)
    before = [a.copy() for a in frame.host()]
    rays, tmax, ref = world[1](name)
    for kind in rq.KINDS:
        _assert_same(_run(sc, rays, tmax, kind), ref, kind, name)
    frame.reset().render(1)
    after = frame.host()
    assert (before[0].view(np.uint32) == after[0].view(np.uint32)).all()
    assert (before[1] == after[1]).all() and (before[2] == after[2]).all()
    assert before[2].any()
