"""GPU parity of the in-place scene update (spt_scene_update_async and the
refit kernels of csrc/spt_refit.h).

Two references, both bit for bit:
  * the hierarchy the device holds after an update (SmallptScene.hierarchy)
    against the host run of the same header (tests/refit_check.py), section by
    section -- no rendering involved;
  * frames after an update against the oracle's full scan of the edited
    scene (oracle.smallpt_render), computed once per (scene, edit, mode): HDR
    colours, seeds, pixels and all four counters of a counted launch -- the
    comparison of test_gpu_smallpt_layouts.py.

Frames are 64 x 48 at 2 spp."""
import ctypes as C

import numpy as np
import pytest

import refit_check as rc
import scenes_layouts as sl
import spt_check

pytestmark = pytest.mark.gpu

SPP = 2
FRAME = (64, 48)
NTILES = ((FRAME[0] + 7) // 8) * ((FRAME[1] + 7) // 8)
MODES = [pytest.param(0, id="pt"), pytest.param(1, id="dl")]
HOOKS = ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE", "RT_SPT_SCHED", "RT_SPT_DUAL")

CAMERAS = {"n256": sl.small_camera, "n255": sl.small_camera, "no_always": sl.no_always_camera,
           "many_always": sl.many_always_camera, "coincident": sl.coincident_camera, "cloud3000": sl.cloud_camera,
           "one_light1500": sl.cloud_camera}


def _order(S, n):
    """(hierarchy order, tree entries) of a scene, from the host builders."""
    host = rc.Host(S, n)
    try:
        return host.sections()["ids"].copy(), host.nb
    finally:
        host.close()


@pytest.fixture(scope="module")
def world(oracle):
    """base(name) -> (spheres, n, raw rows); edited(name, k) -> raw rows of
    edit k; ref(name, rows, tag, mode) -> the oracle's frame of `rows` (cached
    by (name, tag, mode); read-only)."""
    import rtamd
    frames = spt_check.frame_cache(oracle)
    bases, orders, edits = {}, {}, {}

    def base(name):
        if name not in bases:
            if name == "cornell":
                S, n = rtamd.scenes.cornell()
            elif name == "n255":
                S, n = sl.n255()
            elif name == "one_light1500":
                S, n = sl.cloud_one_light(1500)
            else:
                S, n = rc.SCENES[name]()
            bases[name] = (S, n, rc.raw_rows(S, n))
        return bases[name]

    def edited(name, k):
        if (name, k) not in edits:
            S, n, rows = base(name)
            if name not in orders:
                # a scene without a hierarchy: every sphere counts as a tree entry
                orders[name] = _order(S, n) if n >= 256 else (np.arange(n), n)
            edits[(name, k)] = rc.edit(k, rows, *orders[name])
        return edits[(name, k)]

    def ref(name, rows, tag, mode):
        w, h = FRAME
        cam = rtamd.scenes.cornell_camera if name == "cornell" else CAMERAS[name]
        return frames(w, h, [SPP], mode, None, name="%s/%s" % (name, tag),
                      make=lambda: ((rc.from_raw(rows), len(rows)), cam(w, h)))

    return base, edited, ref


class Launcher:
    """One prepared scene and a device frame."""

    def __init__(self, rt, S, n, name):
        import torch
        w, h = FRAME
        cam = rt.scenes.cornell_camera if name == "cornell" else CAMERAS[name]
        self.sc = rt.SmallptScene(S, n)
        self.frame = rt.SmallptDeviceFrame(self.sc, cam(w, h), w, h)
        self.all_groups = torch.arange(self.frame.groups_total, dtype=torch.int32, device=self.frame.device)

    def render(self, mode, counted, as_list=False):
        f = self.frame.reset()
        f.render(SPP, mode=mode, counted=counted, groups=self.all_groups if as_list else None)
        return f.host() + (f.counters.tolist() if counted else None,)

    def close(self):
        self.sc.close()


def _clean(monkeypatch, **env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _both(lz, ref, mode, as_list=False):
    """A counted and an uncounted launch, both the oracle's frame."""
    for counted in (True, False):
        spt_check.assert_same(lz.render(mode, counted, as_list=as_list), ref)


def _differs(a, b):
    return (a[0].view(np.uint32) != b[0].view(np.uint32)).any()


# ---- 1. the device refit equals the host's --------------------------------------
@pytest.mark.parametrize("name", list(rc.SCENES))
def test_device_refit_equals_host_arithmetic(rt, world, monkeypatch, name):
    """Edits 1..5 in turn on one prepared scene: after each update the five
    sections the device holds are the host refit's, byte for byte.  On the
    degenerate kinds' base cloud, three more steps per kind: to the kind, back,
    and the base again against the builders' bytes."""
    _clean(monkeypatch)
    S, n, rows = world[0](name)
    host = rc.Host(S, n)
    sc = rt.SmallptScene(S, n)
    try:
        info = sc.info()
        assert info["leaf_max"] == rc.LEAF[name] and info["nodes"] == host.nodes and info["wnodes"] == host.wnodes
        assert sc.update_info() == dict.fromkeys(sc.UPDATE_INFO, 0)
        built = sc.hierarchy()
        for k, v in host.sections().items():
            assert (built[k].view(np.uint32) == v.view(np.uint32)).all(), ("as created", k)
        for k in rc.EDITS:
            new = rc.from_raw(world[1](name, k))
            sc.update(new)
            got, want = sc.hierarchy(), host.refit(new).sections()
            for sec in rc.SECTIONS:
                a, b = got[sec].view(np.uint32), want[sec].view(np.uint32)
                assert a.shape == b.shape
                assert (a == b).all(), "edit %d, %s: %d words differ, first at %s" % (
                    k, sec, (a != b).sum(), np.argwhere(a != b)[0])
            ui = sc.update_info()
            assert ui["updates"] == k and ui["refits"] == k and ui["reallocations"] == 0, ui
            assert ui["metadata_bytes"] == host.meta_bytes, (ui, host.meta_bytes)
        if name == "degenerate":
            # Negative, zero and non-finite radii and centres (scenes_layouts.degenerate): base to each
            # kind, that kind back to base, and base again -- which must be the builders' bytes.
            updates = len(rc.EDITS)
            builders = rc.Host(S, n)
            fresh = {k: v.copy() for k, v in builders.sections().items()}
            builders.close()
            for kind in sl.DEGENERATE_KINDS:
                for step, arr in ((kind, sl.degenerate(kind)[0]), ("back from " + kind, S), ("base again", S)):
                    sc.update(arr)
                    updates += 1
                    got, want = sc.hierarchy(), host.refit(arr).sections()
                    if step == "base again":
                        want = fresh
                    for sec in rc.SECTIONS:
                        a, b = got[sec].view(np.uint32), want[sec].view(np.uint32)
                        assert a.shape == b.shape
                        assert (a == b).all(), "%s, %s: %d words differ, first at %s" % (
                            step, sec, (a != b).sum(), np.argwhere(a != b)[0])
                    assert host.check() == (0, ""), step
            ui = sc.update_info()
            assert ui["updates"] == updates and ui["refits"] == updates and ui["reallocations"] == 0, ui
        assert sc.info()["leaf_max"] == info["leaf_max"] and sc.info()["family"] == info["family"]
    finally:
        sc.close()
        host.close()


# ---- 2. frames of hierarchy scenes ---------------------------------------------
COOP = {"RT_SPT_TUNE": "coop=%d,coop_g=8" % NTILES}
TARGETS = [pytest.param("n256", {}, "GEO_WIDE", (1,), id="n256"),
           pytest.param("cloud3000", {}, "GEO_WIDE", (1,), id="cloud3000-wide"),
           pytest.param("cloud3000", {"RT_SPT_WIDE": "0"}, "GEO_BVH", (1,), id="cloud3000-binary"),
           pytest.param("cloud3000", COOP, "GEO_WIDE", (1,), id="cloud3000-coop8"),
           pytest.param("many_always", {}, "GEO_WIDE", (1, 4), id="many_always"),
           pytest.param("coincident", {}, "GEO_WIDE", (1,), id="coincident")]


def _frames_after_edits(rt, world, monkeypatch, name, env, family, ks, mode, hierarchy=True):
    _clean(monkeypatch, **env)
    S, n, rows = world[0](name)
    coop = "RT_SPT_TUNE" in env
    lz = Launcher(rt, S, n, name)
    try:
        info = lz.sc.info()
        assert info["family"] == family, info
        before = lz.render(mode, False, as_list=coop)
        for i, k in enumerate(ks):
            new = world[1](name, k)
            lz.sc.update(rc.from_raw(new))
            ref = world[2](name, new, "edit%d" % k, mode)
            _both(lz, ref, mode, as_list=coop)
            assert _differs(before, ref), "the edit must change the frame"
            ui, now = lz.sc.update_info(), lz.sc.info()
            assert ui["updates"] == i + 1 and ui["refits"] == (i + 1 if hierarchy else 0) and ui["reallocations"] == 0
            assert now["family"] == family and now["leaf_max"] == info["leaf_max"]
            if coop:
                assert now["cg"] == 8 and now["n1"] == NTILES, now
    finally:
        lz.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,env,family,ks", TARGETS)
def test_frames_after_a_refit(rt, world, monkeypatch, name, env, family, ks, mode):
    """After edit 1 (and after edit 4 on many_always: a tree sphere past the
    partition rule, an always sphere below it) counted and uncounted launches
    render the oracle's frame of the edited scene, in both estimators; the
    family and the leaf size stay, a refit ran, nothing was reallocated."""
    _frames_after_edits(rt, world, monkeypatch, name, env, family, ks, mode)


# ---- 3. scenes without a hierarchy ---------------------------------------------
FLAT = [pytest.param("cornell", {}, "GEO_LDS", id="cornell"),
        pytest.param("n255", {}, "GEO_LDS", id="n255"),
        pytest.param("cloud3000", {"RT_SPT_NO_BVH": "1"}, "GEO_GLOBAL", id="cloud3000-scan")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,env,family", FLAT)
def test_frames_after_an_update_without_a_hierarchy(rt, world, monkeypatch, name, env, family, mode):
    _frames_after_edits(rt, world, monkeypatch, name, env, family, (1,), mode, hierarchy=False)


@pytest.mark.parametrize("mode", MODES)
def test_the_viewers_edit_on_cornell(rt, world, monkeypatch, mode):
    """The drop-in's own edit: S[6].p.x += 1, the whole array uploaded."""
    _clean(monkeypatch)
    S, n, rows = world[0]("cornell")
    new = rows.copy()
    new[6, 1] += np.float32(1.0)
    lz = Launcher(rt, S, n, "cornell")
    try:
        _both(lz, world[2]("cornell", rows, "base", mode), mode)
        lz.sc.update(rc.from_raw(new))
        _both(lz, world[2]("cornell", new, "moved", mode), mode)
        assert lz.sc.info()["two_query"] == (mode == 0)
    finally:
        lz.close()


# ---- 4. materials ----------------------------------------------------------------
def test_lights_switched_off(rt, world, monkeypatch):
    """cloud(3000): emitters 2 and 3 stop emitting -- three lights become one."""
    _clean(monkeypatch)
    S, n, rows = world[0]("cloud3000")
    new = rows.copy()
    new[2:4, 4:7] = 0.0
    lz = Launcher(rt, S, n, "cloud3000")
    try:
        assert lz.sc.info()["nlights"] == 3
        lz.sc.update(rc.from_raw(new[2:4]), first=2)
        assert lz.sc.info()["nlights"] == 1 and lz.sc.update_info()["light_rebuilds"] == 1
        for mode in (0, 1):
            _both(lz, world[2]("cloud3000", new, "one-light", mode), mode)
        assert lz.sc.update_info()["reallocations"] == 0
    finally:
        lz.close()


def test_lights_switched_on_grown_and_refraction_removed(rt, world, monkeypatch):
    """cloud_one_light(1500), scanned in full: path tracing runs the
    two-query kernel while the scene has one light.  Spheres 2 and 3 start
    to emit (three lights: the one-query kernel, and more light records than
    the scene was created with -- a reallocation); a non-emitter becomes a
    fourth light (a second reallocation: the array grows to at least twice its
    records, here from three to six); every REFR sphere becomes SPEC (no_refr
    flips).  Each frame equals the oracle's."""
    _clean(monkeypatch, RT_SPT_NO_BVH="1")
    S, n, rows = world[0]("one_light1500")
    cloud = sl.cloud_rows(1500)
    lz = Launcher(rt, S, n, "one_light1500")
    try:
        info = lz.sc.info()
        assert info["nlights"] == 1 and info["nodes"] == 0 and not info["no_refr"]
        _both(lz, world[2]("one_light1500", rows, "base", 0), 0)
        assert lz.sc.info()["two_query"]
        three = rows.copy()
        three[2:4, 4:10] = cloud[2:4, 4:10]
        lz.sc.update(rc.from_raw(three[2:4]), first=2)
        _both(lz, world[2]("one_light1500", three, "three-lights", 0), 0)
        info = lz.sc.info()
        assert info["nlights"] == 3 and not info["two_query"]
        assert lz.sc.update_info()["reallocations"] == 1
        four = three.copy()
        assert (four[700, 4:7] == 0).all()
        four[700, 4:7] = [6.0, 5.0, 4.0]
        lz.sc.update(rc.from_raw(four[700:701]), first=700)
        for mode in (0, 1):
            _both(lz, world[2]("one_light1500", four, "four-lights", mode), mode)
        assert lz.sc.info()["nlights"] == 4 and lz.sc.update_info()["reallocations"] == 2
        spec = four.copy()
        refl = spec[:, 10].view(np.int32)
        assert (refl == sl.REFR).any()
        refl[refl == sl.REFR] = sl.SPEC
        lz.sc.update(rc.from_raw(spec))
        assert lz.sc.info()["no_refr"] and lz.sc.info()["nlights"] == 4
        _both(lz, world[2]("one_light1500", spec, "no-refr", 0), 0)
        ui = lz.sc.update_info()
        assert ui["updates"] == 3 and ui["refits"] == 0 and ui["light_rebuilds"] == 3 and ui["reallocations"] == 2, ui
    finally:
        lz.close()


# ---- 5. a partial range ------------------------------------------------------------
def test_partial_range(rt, world, monkeypatch):
    """first=100, count=50 on n256; then the whole edited array again (an
    identity update): the device's sections are the host refit's both times,
    so nothing outside the range moved."""
    _clean(monkeypatch)
    S, n, rows = world[0]("n256")
    new = rows.copy()
    rng = np.random.default_rng(50)
    new[100:150, 1:4] += rng.uniform(-2, 2, (50, 3)).astype(np.float32)
    new[100:150, 0] *= np.float32(1.5)
    host = rc.Host(S, n)
    lz = Launcher(rt, S, n, "n256")
    try:
        want = host.refit(rc.from_raw(new)).sections()
        lz.sc.update(rc.from_raw(new[100:150]), first=100, count=50)
        ref = world[2]("n256", new, "partial", 0)
        _both(lz, ref, 0)
        got = lz.sc.hierarchy()
        for sec in rc.SECTIONS:
            assert (got[sec].view(np.uint32) == want[sec].view(np.uint32)).all(), sec
        lz.sc.update(rc.from_raw(new))
        got = lz.sc.hierarchy()
        for sec in rc.SECTIONS:
            assert (got[sec].view(np.uint32) == want[sec].view(np.uint32)).all(), ("identity", sec)
        _both(lz, ref, 0)
        _both(lz, world[2]("n256", new, "partial", 1), 1)
    finally:
        lz.close()
        host.close()


# ---- 6. stream order -----------------------------------------------------------------
@pytest.mark.parametrize("name", ["n256", "cornell"])
def test_stream_order(rt, world, monkeypatch, name):
    """A render, an update and a render on one stream with no host
    synchronisation between them: the first frame is the old scene's, the
    second the new one's."""
    import torch
    _clean(monkeypatch)
    S, n, rows = world[0](name)
    new = world[1](name, 1)
    w, h = FRAME
    sc = rt.SmallptScene(S, n)
    try:
        cam = (rt.scenes.cornell_camera if name == "cornell" else CAMERAS[name])(w, h)
        a, b = (rt.SmallptDeviceFrame(sc, cam, w, h) for _ in range(2))
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        arr = rc.from_raw(new)
        a.render(SPP, counted=True, stream=s)
        sc.update(arr, stream=s)
        C.memset(arr, 0xFF, C.sizeof(arr))          # the array is the caller's again
        b.render(SPP, counted=True, stream=s)
        spt_check.assert_same(a, world[2](name, rows, "base", 0))
        spt_check.assert_same(b, world[2](name, new, "edit1", 0))
    finally:
        sc.close()


# ---- 7. the learnt order survives -----------------------------------------------------
def test_learnt_order_survives_an_update(rt, world, monkeypatch):
    """cloud(3000), direct lighting: three launches until the learnt order's
    cooperative tier is in use; after an update the next launch still uses it."""
    _clean(monkeypatch)
    S, n, rows = world[0]("cloud3000")
    new = world[1]("cloud3000", 1)
    lz = Launcher(rt, S, n, "cloud3000")
    try:
        for i in range(3):
            lz.render(1, False)
        info = lz.sc.info()
        assert info["family"] == "GEO_WIDE" and info["cg"] == 8 and info["n1"] > 0, info
        lz.sc.update(rc.from_raw(new))
        got = lz.render(1, False)
        info = lz.sc.info()
        assert info["cg"] == 8 and info["n1"] > 0, info
        spt_check.assert_same(got, world[2]("cloud3000", new, "edit1", 1))
    finally:
        lz.close()


# ---- 8. rejected calls ------------------------------------------------------------------
def test_rejected_updates_leave_the_scene(rt, world, monkeypatch):
    import torch
    _clean(monkeypatch)
    S, n, rows = world[0]("n256")
    new = rc.from_raw(world[1]("n256", 1))
    INVALID = rt._lib.RT_ERR_INVALID
    lz = Launcher(rt, S, n, "n256")
    try:
        for case in ("before any update", "after one"):
            ui = lz.sc.update_info()
            with pytest.raises(rt.RTError) as e:
                lz.sc.update(new, first=200, count=100)       # past the end
            assert e.value.code == INVALID
            with pytest.raises(rt.RTError) as e:
                lz.sc.update(new, first=n, count=1)
            assert e.value.code == INVALID
            with pytest.raises(rt.RTError) as e:
                lz.sc.update(None, count=1)                   # a null array
            assert e.value.code == INVALID
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="relaxed"):
                with pytest.raises(rt.RTError) as e:
                    lz.sc.update(new)                         # (the capture's stream is the current one in here)
            assert e.value.code == INVALID
            del g
            torch.cuda.synchronize()
            assert lz.sc.update_info() == ui, case
            _both(lz, world[2]("n256", rows, "base", 0), 0)
            lz.sc.update(S)                                   # an accepted one (the same spheres), then again
        assert lz.sc.update_info()["updates"] == 2
    finally:
        lz.close()


# ---- 9. the multi-GPU frame ----------------------------------------------------------------
def test_multi_update_scene(rt):
    """SmallptMulti.update_scene with the viewer's Cornell edit on two bands of
    one device: the frame of a fresh SmallptFrame of the edited scene; the
    cached band context of spt_render_multi is not involved."""
    w, h = 160, 120
    S, n, cam = rt.scenes.smallpt("cornell", w, h)
    info = (C.c_uint64 * 2)()
    rt.check(rt.lib().spt_multi_cache_info(info))
    before = list(info)
    m = rt.SmallptMulti(w, h, [0, 0], S, n)
    try:
        m.upload(rt.scenes.seeds(w, h))
        m.render(cam, 0, 2)
        S[6].p.x += 1.0
        m.update_scene(S)
        m.upload(rt.scenes.seeds(w, h), np.zeros(3 * w * h, np.float32))
        m.render(cam, 0, 2)
        col, px = np.empty(3 * w * h, np.float32), np.empty(w * h, np.uint32)
        m.download(col, None, px)
        rt.check(rt.lib().spt_multi_cache_info(info))
        assert list(info) == before
        f = rt.SmallptFrame(w, h, spheres=S, nspheres=n)
        f.render(2)
        assert (col.view(np.uint32) == f.colors.view(np.uint32)).all() and (px == f.pixels).all()
        with pytest.raises(rt.RTError):
            m.update_scene(S, first=5, count=n)
    finally:
        m.close()
