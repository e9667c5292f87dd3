"""GPU parity of the device-memory move (spt_scene_move_async and the gather
of csrc/spt_move.h): a prepared scene's centres and radii taken from a device
tensor.

The statement under test: after a move the scene is, bit for bit, the scene
spt_scene_update_async leaves from the same edited spheres.  Three references,
as for the update (tests/test_gpu_scene_update.py, whose scenes, cameras,
launcher and frame cache serve here):
  * the hierarchy the device holds (SmallptScene.hierarchy) against the host
    refit of the edited rows (tests/refit_check.py; after a regroup
    tests/regroup_check.py), section by section;
  * the device's AoS array (SmallptScene.spheres) against the edited rows;
  * frames against the oracle's full scan of the edited scene: HDR colours,
    seeds, pixels and all four counters of a counted launch.

Graphs.  A graph that holds a move together with a render is recorded on
scenes without a hierarchy only; a hierarchy scene's graph holds the move
alone and the frames after its replays are ordinary launches (DESIGN.md,
section 3, "Captured graphs across scene edits").

Frames are 64 x 48 at 2 spp."""
import numpy as np
import pytest

import refit_check as rc
import regroup_check as rg
import scenes_layouts as sl
import spt_check
import test_gpu_scene_update as su

pytestmark = pytest.mark.gpu

SPP, FRAME, MODES = su.SPP, su.FRAME, su.MODES
world = su.world                                      # (the module-scoped fixture, computed once for this module)
HIERARCHY_SCENES = ("n256", "no_always", "many_always", "coincident", "cloud3000")


def geom(rows):
    """float32 [count, 4] of p.x, p.y, p.z, rad from raw rows (rad first)."""
    return np.ascontiguousarray(np.concatenate([rows[:, 1:4], rows[:, 0:1]], axis=1), np.float32)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def moved(rows, to, a, b):
    """`rows` with the centres and radii of [a, b) taken from `to`."""
    out = rows.copy()
    out[a:b, 0:4] = to[a:b, 0:4]
    return out


def same_rows(sc, rows):
    got = sc.spheres()
    bad = got.view(np.uint32) != np.ascontiguousarray(rows, np.float32).view(np.uint32)
    assert not bad.any(), "spheres(): %d words differ, first at %s" % (bad.sum(), np.argwhere(bad)[0])


def same_sections(sc, host, rows, what):
    diff = rg.first_difference(sc.hierarchy(), host.refit(rc.from_raw(rows)).sections())
    assert diff == "", "%s: %s" % (what, diff)


def camera_of(rt, name):
    return rt.scenes.cornell_camera if name == "cornell" else su.CAMERAS[name]


# ---- 1. move equals update ----------------------------------------------------------
@pytest.mark.parametrize("name", HIERARCHY_SCENES)
def test_move_equals_the_host_refit(rt, world, monkeypatch, name):
    """One sphere (edit 2's: 10^3 x the extent away, the exponents grow), a
    middle range (edit 1's spheres of the second and third quarter) and the
    whole scene (edit 5: every tree sphere on one point), each from a device
    tensor: the five sections are the host refit's of the rows so far and the
    AoS array is those rows."""
    su._clean(monkeypatch)
    S, n, rows = world[0](name)
    host = rc.Host(S, n)
    sc = rt.SmallptScene(S, n)
    try:
        info = sc.info()
        assert sc.move_info() == dict.fromkeys(sc.MOVE_INFO, 0)
        same_rows(sc, rows)
        e2, e1, e5 = (world[1](name, k) for k in (2, 1, 5))
        one = int(np.flatnonzero((e2 != rows).any(1))[0])
        cur = rows
        for i, (to, a, b) in enumerate(((e2, one, one + 1), (e1, n // 4, 3 * n // 4), (e5, 0, n))):
            cur = moved(cur, to, a, b)
            sc.move(dev(geom(cur[a:b])), first=a)
            same_sections(sc, host, cur, "range [%d, %d)" % (a, b))
            same_rows(sc, cur)
            assert sc.move_info() == {"moves": i + 1, "captured": 0, "refits": i + 1}
        ui = sc.update_info()
        assert ui["updates"] == 0 and ui["refits"] == 0 and ui["metadata_bytes"] == host.meta_bytes, ui
        now = sc.info()
        for key in ("family", "leaf_max", "nodes", "wnodes", "nlights", "no_refr"):
            assert now[key] == info[key], key
    finally:
        sc.close()
        host.close()


# ---- 2. frames, every family ----------------------------------------------------------
FAMILIES = [pytest.param("cornell", {}, "GEO_LDS", id="cornell-lds"),
            pytest.param("n255", {"RT_SPT_GEO": "global"}, "GEO_GLOBAL", id="n255-global"),
            pytest.param("cloud3000", {"RT_SPT_WIDE": "0"}, "GEO_BVH", id="cloud3000-binary"),
            pytest.param("cloud3000", {}, "GEO_WIDE", id="cloud3000-wide")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,env,family", FAMILIES)
def test_frames_after_a_move(rt, world, monkeypatch, name, env, family, mode):
    """Edit 1 changes centres and radii alone, so a whole-scene move to it
    gives the scene the update tests render: counted and uncounted launches
    are the oracle's frame of the edited scene."""
    su._clean(monkeypatch, **env)
    S, n, rows = world[0](name)
    new = world[1](name, 1)
    lz = su.Launcher(rt, S, n, name)
    try:
        info = lz.sc.info()
        assert info["family"] == family, info
        before = lz.render(mode, False)
        lz.sc.move(dev(geom(new)))
        ref = world[2](name, new, "edit1", mode)
        su._both(lz, ref, mode)
        assert su._differs(before, ref), "the move must change the frame"
        same_rows(lz.sc, new)
        mi, now = lz.sc.move_info(), lz.sc.info()
        assert mi == {"moves": 1, "captured": 0, "refits": 1 if n >= 256 else 0}, mi
        assert now["family"] == family and now["leaf_max"] == info["leaf_max"] and now["nlights"] == info["nlights"]
    finally:
        lz.close()


# ---- 3. a moved emitter ------------------------------------------------------------------
def _emitter_case(name, rows):
    """(index, new radius and centre) of the emitter moved and resized."""
    new = rows.copy()
    if name == "cornell":
        i = int(np.flatnonzero((rows[:, 4:7] != 0).any(1))[0])
        new[i, 0:4] = [5.0, 40.0, 60.0, 75.0]             # (7 at (50, 66.6, 81.6))
    else:
        i = 2
        new[i, 0:4] = [1.25, 4.0, 9.0, -2.0]              # (0.5 at (10, 5, -5))
    return i, new


@pytest.mark.parametrize("name", ["cloud3000", "cornell"])
def test_a_moved_emitter(rt, world, monkeypatch, name):
    """The light record follows its sphere: both estimators render the
    oracle's frame (Cornell's one light: path tracing runs the one-light
    two-query kernel); the light count stays."""
    su._clean(monkeypatch)
    S, n, rows = world[0](name)
    i, new = _emitter_case(name, rows)
    lz = su.Launcher(rt, S, n, name)
    try:
        nlights = lz.sc.info()["nlights"]
        assert nlights == (1 if name == "cornell" else 3)
        base = lz.render(1, False)
        lz.sc.move(dev(geom(new[i:i + 1])), first=i)
        for mode in (0, 1):
            su._both(lz, world[2](name, new, "emitter-moved", mode), mode)
            if name == "cornell":
                assert lz.sc.info()["two_query"] == (mode == 0)
        assert su._differs(base, world[2](name, new, "emitter-moved", 1))
        assert lz.sc.info()["nlights"] == nlights
        same_rows(lz.sc, new)
        assert lz.sc.update_info()["light_rebuilds"] == 0
    finally:
        lz.close()


# ---- 4. any floats -----------------------------------------------------------------------
def _degenerate_geometry(rt, sc, cam, rows):
    """`rows` with seven spheres the camera sees (first hits of the pixel
    centres' rays; not the ground, not a light) given a NaN centre, an
    infinite, a NaN, a negative, a zero and a -0.0 radius, and a centre at
    3e38 whose box overflows."""
    import torch
    w, h = FRAME
    _, ids = sc.query(torch.from_numpy(rt.scenes.camera_rays(cam, w, h)).cuda())
    ids = ids.cpu().numpy()
    seen, counts = np.unique(ids[ids >= 4], return_counts=True)
    seen = seen[np.argsort(-counts, kind="stable")][:7]
    assert len(seen) == 7, "the camera must see seven plain spheres"
    out = rows.copy()
    out[seen[0], 2] = np.nan
    out[seen[1], 0] = np.inf
    out[seen[2], 0] = np.nan
    out[seen[3], 0] *= np.float32(-2.0)
    out[seen[4], 0] = 0.0
    out[seen[5], 0] = -0.0
    out[seen[6], 0:2] = [1e38, 3e38]
    assert np.signbit(out[seen[5], 0])
    return out


@pytest.mark.parametrize("env,family", [pytest.param({}, "GEO_WIDE", id="wide"),
                                        pytest.param({"RT_SPT_WIDE": "0"}, "GEO_BVH", id="binary")])
def test_any_floats(rt, world, monkeypatch, env, family):
    su._clean(monkeypatch, **env)
    S, n, rows = world[0]("n256")
    host = rc.Host(S, n, wide=not env)
    lz = su.Launcher(rt, S, n, "n256")
    try:
        assert lz.sc.info()["family"] == family
        new = _degenerate_geometry(rt, lz.sc, lz.frame.camera, rows)
        before = lz.render(0, False)
        lz.sc.move(dev(geom(new)))
        same_sections(lz.sc, host, new, "degenerate entries")
        assert host.check() == (0, "")
        same_rows(lz.sc, new)
        for mode in (0, 1):
            su._both(lz, world[2]("n256", new, "any-floats", mode), mode)
        assert su._differs(before, world[2]("n256", new, "any-floats", 0))
        # and back: the finite scene again
        lz.sc.move(dev(geom(rows)))
        same_sections(lz.sc, host, rows, "back")
        su._both(lz, world[2]("n256", rows, "base", 0), 0)
    finally:
        lz.close()
        host.close()


# ---- 5. stream order without a synchronise --------------------------------------------------
@pytest.mark.parametrize("name", ["n256", "cornell"])
def test_stream_order(rt, world, monkeypatch, name):
    """Frame A, a torch op that writes the geometry tensor, the move, a torch
    op that overwrites the tensor, frame B -- back to back on one stream: A is
    the old scene's frame, B the edited scene's."""
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0](name)
    new = world[1](name, 1)
    w, h = FRAME
    sc = rt.SmallptScene(S, n)
    try:
        cam = camera_of(rt, name)(w, h)
        a, b = (rt.SmallptDeviceFrame(sc, cam, w, h) for _ in range(2))
        src, G = dev(geom(new)), torch.zeros((n, 4), dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        sc.move_prepare()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            a.render(SPP, counted=True, stream=s)
            G.copy_(src)
            sc.move(G)                                  # (torch's current stream: s)
            G.fill_(float("nan"))
            b.render(SPP, counted=True, stream=s)
        spt_check.assert_same(a, world[2](name, rows, "base", 0))
        spt_check.assert_same(b, world[2](name, new, "edit1", 0))
        same_rows(sc, new)
    finally:
        sc.close()


# ---- 6. interplay -----------------------------------------------------------------------------
def test_move_update_regroup_move(rt, world, monkeypatch):
    """cloud(3000): a move; a host update of another range that changes a
    material and adds an emitter; a regroup; a move of the whole scene (the
    new emitter with it).  After each step the frames are the oracle's of the
    scene so far, after the regroup the hierarchy is regroup_check's."""
    su._clean(monkeypatch)
    S, n, rows = world[0]("cloud3000")
    e1 = world[1]("cloud3000", 1)
    host = rg.Host(S, n)
    lz = su.Launcher(rt, S, n, "cloud3000")

    def frames(cur, tag):
        for mode in (0, 1):
            su._both(lz, world[2]("cloud3000", cur, tag, mode), mode)

    try:
        sc = lz.sc
        cur = moved(rows, e1, 100, 400)
        sc.move(dev(geom(cur[100:400])), first=100)
        frames(cur, "interplay-1")
        same_sections(sc, host, cur, "move")

        cur = moved(cur, e1, 1000, 1200)
        assert (cur[1001, 4:7] == 0).all()
        cur[1000, 7:10] = [0.9, 0.2, 0.1]
        cur[1000, 10:11].view(np.int32)[:] = sl.SPEC if cur[1000, 10:11].view(np.int32)[0] != sl.SPEC else sl.DIFF
        cur[1001, 4:7] = [6.0, 5.0, 4.0]
        sc.update(rc.from_raw(cur[1000:1200]), first=1000)
        assert sc.info()["nlights"] == 4
        frames(cur, "interplay-2")
        same_sections(sc, host, cur, "update")
        same_rows(sc, cur)

        sc.regroup()
        diff = rg.first_difference(sc.hierarchy(), host.regroup(rc.from_raw(cur)).sections())
        assert diff == "", "regroup: " + diff
        frames(cur, "interplay-2")

        cur = cur.copy()                                # everything but the ground and the first light moves,
        cur[4:, 1:4] += np.random.default_rng(6).uniform(-1.5, 1.5, (n - 4, 3)).astype(np.float32)
        cur[[2, 1001], 0] *= np.float32(2.0)            # an old and the new emitter grow,
        cur[3, 1:4] += np.array([2.0, -3.0, 1.0], np.float32)   # another one moves
        sc.move(dev(geom(cur)))
        same_sections(sc, host, cur, "move after the regroup")
        same_rows(sc, cur)
        frames(cur, "interplay-4")

        ui = sc.update_info()
        assert (ui["updates"], ui["refits"], ui["light_rebuilds"], ui["reallocations"]) == (1, 1, 1, 1), ui
        assert sc.regroup_info()["regroups"] == 1
        assert sc.move_info() == {"moves": 2, "captured": 0, "refits": 2}
        assert sc.info()["nlights"] == 4
    finally:
        lz.close()
        host.close()


# ---- 7. capture, a scene without a hierarchy ----------------------------------------------------
def test_captured_move_and_frame_on_cornell(rt, world, monkeypatch):
    """A graph of {move of spheres 6..8 (the two balls and the light) from G,
    frame}, captured once and replayed three times with G rewritten by a
    torch op before each replay: every replay's frame is the oracle's of that
    step's spheres."""
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("cornell")
    assert n == 9 and (rows[8, 4:7] != 0).all()
    steps = []
    for k in range(3):
        new = rows.copy()
        new[6, 1] += np.float32(4.0 * (k + 1))             # the mirror ball to the right
        new[7, 0] *= np.float32(1.0 - 0.2 * (k + 1))       # the glass ball shrinks
        new[8, 0:4] = [7.0 - k, 50.0 - 8 * k, 66.6 - 3 * k, 81.6]   # the light smaller, lower, to the left
        steps.append(new)
    lz = su.Launcher(rt, S, n, "cornell")
    try:
        sc, f = lz.sc, lz.frame
        sc.move_prepare()
        for _ in range(3):                                 # (uncaptured launches first, as the other graph tests do)
            f.reset().render(SPP)
        G = dev(geom(rows[6:9]))
        src = [dev(geom(new[6:9])) for new in steps]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="relaxed"):
            sc.move(G, first=6)
            f.render(SPP)
        torch.cuda.synchronize()
        assert sc.move_info() == {"moves": 1, "captured": 1, "refits": 0}
        same_rows(sc, rows)                                # (recording moves nothing)
        for k, new in enumerate(steps):
            G.copy_(src[k])
            f.reset(colors=-1.0, pixels=1, seeds=1)
            g.replay()
            spt_check.assert_same(f, world[2]("cornell", new, "captured-%d" % k, 0), counted=False)
            same_rows(sc, new)
        assert sc.move_info()["moves"] == 1
        del g
        torch.cuda.synchronize()
    finally:
        lz.close()


# ---- 8. capture, a hierarchy scene: the move alone -------------------------------------------------
def test_captured_move_alone_on_n256(rt, world, monkeypatch):
    """After move_prepare a graph of {move from G} is captured and replayed
    twice with G rewritten; the frames after each replay are ordinary
    launches and the oracle's, the hierarchy is the host refit's."""
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("n256")
    host = rc.Host(S, n)
    lz = su.Launcher(rt, S, n, "n256")
    try:
        sc = lz.sc
        sc.move_prepare()
        same_sections(sc, host, rows, "prepared")
        su._both(lz, world[2]("n256", rows, "base", 0), 0)
        G = dev(geom(rows))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="relaxed"):
            sc.move(G)
        torch.cuda.synchronize()
        assert sc.move_info() == {"moves": 1, "captured": 1, "refits": 1}
        for k in (1, 5):
            new = world[1]("n256", k)
            G.copy_(dev(geom(new)))
            g.replay()
            su._both(lz, world[2]("n256", new, "edit%d" % k, 0), 0)
            same_sections(sc, host, new, "replay to edit %d" % k)
            same_rows(sc, new)
        del g
        torch.cuda.synchronize()
    finally:
        lz.close()
        host.close()


def test_capturing_a_move_of_an_unprepared_scene_fails(rt, world, monkeypatch):
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("n256")
    new = world[1]("n256", 1)
    lz = su.Launcher(rt, S, n, "n256")
    try:
        G = dev(geom(new))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="relaxed"):
            with pytest.raises(rt.RTError) as e:
                lz.sc.move(G)                              # (the capture's stream is the current one in here)
        assert e.value.code == rt._lib.RT_ERR_INVALID
        del g
        torch.cuda.synchronize()
        assert lz.sc.move_info() == dict.fromkeys(lz.sc.MOVE_INFO, 0)
        su._both(lz, world[2]("n256", rows, "base", 0), 0)
        lz.sc.move(G)                                      # usable: an uncaptured move prepares the scene itself
        su._both(lz, world[2]("n256", new, "edit1", 0), 0)
    finally:
        lz.close()


# ---- 9. rejected calls ---------------------------------------------------------------------------------
def test_rejected_moves_leave_the_scene(rt, world, monkeypatch):
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("n256")
    INVALID = rt._lib.RT_ERR_INVALID
    move = rt._lib.entry("spt_scene_move_async")
    lz = su.Launcher(rt, S, n, "n256")
    try:
        big = dev(np.zeros(4 * n + 4, np.float32))
        G = big[:4 * n].view(n, 4)
        odd = big[1:4 * n + 1].view(n, 4)                  # contiguous, 4 bytes off a 16-byte boundary
        assert G.data_ptr() % 16 == 0 and odd.data_ptr() % 16 == 4 and odd.is_contiguous()
        for case in ("before any move", "after one"):
            mi, held = lz.sc.move_info(), lz.sc.hierarchy()
            for what, call in (
                    ("past the end", lambda: lz.sc.move(G[:100], first=200)),
                    ("first at the end", lambda: lz.sc.move(G[:1], first=n)),
                    ("misaligned", lambda: lz.sc.move(odd)),
                    ("null geometry", lambda: rt.check(move(lz.sc.handle, None, 0, 1, None))),
                    ("null scene", lambda: rt.check(move(None, G.data_ptr(), 0, 1, None)))):
                with pytest.raises(rt.RTError) as e:
                    call()
                assert e.value.code == INVALID, what
            if torch.cuda.device_count() > 1:              # another current device
                rt.set_device(1)
                try:
                    with pytest.raises(rt.RTError) as e:
                        rt.check(move(lz.sc.handle, G.data_ptr(), 0, 1, None))
                    assert e.value.code == INVALID
                finally:
                    rt.set_device(0)
            with pytest.raises(ValueError):
                lz.sc.move(G.view(-1))                     # not [count, 4]
            rt.check(move(lz.sc.handle, G.data_ptr(), 0, 0, None))       # count == 0: RT_OK, nothing launched
            rt.check(move(lz.sc.handle, G.data_ptr(), n, 0, None))
            assert lz.sc.move_info() == mi, case
            assert rg.first_difference(lz.sc.hierarchy(), held) == "", case
            same_rows(lz.sc, rows)
            su._both(lz, world[2]("n256", rows, "base", 0), 0)
            G.copy_(dev(geom(rows)))
            lz.sc.move(G)                                  # an accepted one (the same geometry), then again
        assert lz.sc.move_info() == {"moves": 2, "captured": 0, "refits": 2}
    finally:
        lz.close()
