"""GPU parity of the hierarchy regroup (spt_scene_regroup_async and the
kernels of csrc/spt_regroup.h).

Two references, both bit for bit, as for the in-place update
(tests/test_gpu_scene_update.py, whose scenes, cameras, targets and launcher
serve here):
  * the hierarchy the device holds after a regroup (SmallptScene.hierarchy)
    against the host run of the same header (tests/regroup_check.py), section
    by section;
  * frames, queries and radiance after a regroup against what they were before
    it, and frames against the oracle's full scan of the edited scene.

Frames are 64 x 48 at 2 spp."""
import ctypes as C

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


# ---- 6. the device regroup equals the host's ------------------------------------
@pytest.mark.parametrize("name", list(rc.SCENES))
def test_device_regroup_equals_host(rt, world, monkeypatch, name):
    """update(edit 1), regroup, update(edit 5), regroup on one prepared scene:
    after each regroup the five sections the device holds are regroup_host's,
    byte for byte; the launch parameters and the update's bookkeeping stay."""
    su._clean(monkeypatch)
    S, n, rows = world[0](name)
    host = rg.Host(S, n)
    sc = rt.SmallptScene(S, n)
    try:
        info = sc.info()
        assert sc.regroup_info() == dict.fromkeys(sc.REGROUP_INFO, 0)
        levels, glob, subs = host.plan()
        for i, k in enumerate((1, 5)):
            new = rc.from_raw(world[1](name, k))
            sc.update(new)
            ui = sc.update_info()
            sc.regroup()
            got, want = sc.hierarchy(), host.regroup(new).sections()
            diff = rg.first_difference(got, want)
            assert diff == "", "edit %d: %s" % (k, diff)
            assert host.check() == (0, "")
            ri = sc.regroup_info()
            assert ri["regroups"] == i + 1 and ri["levels"] == levels and ri["global_levels"] == glob, ri
            assert ri["bytes"] >= 8 * host.nb + 16 * host.nodes
            assert sc.update_info() == ui
            now = sc.info()
            for key in ("family", "leaf_max", "nodes", "wnodes", "wdepth", "nalways"):
                assert now[key] == info[key], key
        assert (glob > 0) == (host.nb > 256)
    finally:
        sc.close()
        host.close()


@pytest.mark.parametrize("name,sub_max", [("n256", 0), ("cloud3000", 0), ("cloud3000", 4096)])
def test_other_tier_sizes_equal_host(rt, world, monkeypatch, name, sub_max):
    """RT_SPT_REGROUP_LDS=0 (every level sorted by passes of its own, the form
    the LDS tier is measured against) and =4096 (the whole tree of cloud(3000)
    in one block, sixteen entries a lane): the same bytes."""
    su._clean(monkeypatch, RT_SPT_REGROUP_LDS=str(sub_max))
    S, n, rows = world[0](name)
    host = rg.Host(S, n)
    sc = rt.SmallptScene(S, n)
    try:
        new = rc.from_raw(world[1](name, 1))
        sc.update(new)
        sc.regroup()
        assert rg.first_difference(sc.hierarchy(), host.regroup(new).sections()) == ""
        levels, glob, subs = host.plan(sub_max)
        ri = sc.regroup_info()
        assert ri["levels"] == levels and ri["global_levels"] == glob == (0 if sub_max else levels - 1), ri
    finally:
        sc.close()
        host.close()


# ---- 7. frames ---------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,env,family,ks", su.TARGETS)
def test_frames_after_a_regroup(rt, world, monkeypatch, name, env, family, ks, mode):
    """A regroup of the scene as created (never updated), then update(edit k)
    and regroup: counted and uncounted launches render the oracle's frame of
    the scene as it then is.  (The counted launches read the highest-index
    table, which a regroup rewrites.)"""
    su._clean(monkeypatch, **env)
    S, n, rows = world[0](name)
    coop = "RT_SPT_TUNE" in env
    lz = su.Launcher(rt, S, n, name)
    try:
        info = lz.sc.info()
        assert info["family"] == family, info
        lz.sc.regroup()
        assert lz.sc.regroup_info()["regroups"] == 1 and lz.sc.update_info()["updates"] == 0
        su._both(lz, world[2](name, rows, "base", mode), mode, as_list=coop)
        for i, k in enumerate(ks):
            new = world[1](name, k)
            lz.sc.update(rc.from_raw(new))
            lz.sc.regroup()
            su._both(lz, world[2](name, new, "edit%d" % k, mode), mode, as_list=coop)
            now = lz.sc.info()
            assert now["family"] == family and now["leaf_max"] == info["leaf_max"]
            assert lz.sc.regroup_info()["regroups"] == i + 2
    finally:
        lz.close()


# ---- 8. queries and radiance ----------------------------------------------------------
def test_queries_and_radiance_keep_their_values(rt, world, monkeypatch):
    """cloud(3000) after edit 1: all three query kinds and the radiance along
    the same rays, before a regroup and after it."""
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("cloud3000")
    new = world[1]("cloud3000", 1)
    sc = rt.SmallptScene(S, n)
    try:
        sc.update(rc.from_raw(new))
        cen = new[4:, 1:4].astype(np.float64)
        r = rc.rays(np.random.default_rng(80), cen, (1.0, 2.0, 25.0), 4096, 3.0)
        rays = torch.from_numpy(r).cuda()
        seeds = torch.from_numpy(rt.scenes.seeds(64, 64).view(np.int32).reshape(-1, 2).copy()).cuda()

        def everything():
            t, hit = sc.query(rays)
            tmax = torch.where(hit >= 0, t * 1.5, torch.full_like(t, 30.0))
            _, anyhit = sc.query(rays, tmax, kind="any")
            _, occ = sc.query(rays, tmax, kind="occluder")
            rad, so = sc.radiance(rays, seeds, nsamples=2)
            torch.cuda.synchronize()
            return [x.cpu().numpy() for x in (t, hit, anyhit, occ, rad, so)]

        before = everything()
        assert (before[1] >= 0).any() and (before[3] >= 0).any()
        sc.regroup()
        after = everything()
        for name, a, b in zip(("t", "id", "any", "occluder", "radiance", "seeds"), before, after):
            assert a.tobytes() == b.tobytes(), name
    finally:
        sc.close()


# ---- 9. stream order, capture ---------------------------------------------------------
def test_stream_order(rt, world, monkeypatch):
    """Frame A, update, frame B, regroup, frame C on one stream, one
    synchronise at the end: A is the old scene's frame, B and C the edited
    scene's."""
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("n256")
    new = world[1]("n256", 1)
    w, h = FRAME
    sc = rt.SmallptScene(S, n)
    try:
        cam = su.CAMERAS["n256"](w, h)
        a, b, c = (rt.SmallptDeviceFrame(sc, cam, w, h) for _ in range(3))
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        a.render(SPP, counted=True, stream=s)
        sc.update(rc.from_raw(new), stream=s)
        b.render(SPP, counted=True, stream=s)
        sc.regroup(stream=s)
        c.render(SPP, counted=True, stream=s)
        spt_check.assert_same(a, world[2]("n256", rows, "base", 0))
        spt_check.assert_same(b, world[2]("n256", new, "edit1", 0))
        spt_check.assert_same(c, world[2]("n256", new, "edit1", 0))
    finally:
        sc.close()


def test_rejected_regroups_leave_the_scene(rt, world, monkeypatch):
    """A regroup on a capturing stream and a regroup of a null scene are
    rejected, with the scene untouched."""
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("cloud3000")
    new = world[1]("cloud3000", 1)
    lz = su.Launcher(rt, S, n, "cloud3000")
    try:
        lz.sc.update(rc.from_raw(new))
        held = lz.sc.hierarchy()
        ri, ui = lz.sc.regroup_info(), lz.sc.update_info()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="relaxed"):
            with pytest.raises(rt.RTError) as e:
                lz.sc.regroup()                        # (the capture's stream is the current one in here)
        assert e.value.code == rt._lib.RT_ERR_INVALID
        del g
        torch.cuda.synchronize()
        with pytest.raises(rt.RTError) as e:
            rt.check(rt._lib.entry("spt_scene_regroup_async")(None, None))       # a null scene
        assert e.value.code == rt._lib.RT_ERR_INVALID
        assert lz.sc.regroup_info() == ri and lz.sc.update_info() == ui
        assert rg.first_difference(lz.sc.hierarchy(), held) == ""
        su._both(lz, world[2]("cloud3000", new, "edit1", 0), 0)
    finally:
        lz.close()


def test_graph_captured_before_a_regroup_replays_after_it(rt, world, monkeypatch):
    """No address and no launch parameter changes: the replay renders the
    oracle's frame of the edited scene over the regrouped tree.  (The scene's
    hierarchy is not read back in here: a replay once left the frame's
    sentinels in place with SmallptScene.hierarchy() called before the capture
    and before the replay.  The read-back is not the trigger; what was
    narrowed down is in DESIGN.md, section 3, "Captured graphs across scene
    edits".)"""
    import torch
    su._clean(monkeypatch)
    S, n, rows = world[0]("cloud3000")
    new = world[1]("cloud3000", 1)
    lz = su.Launcher(rt, S, n, "cloud3000")
    try:
        lz.sc.update(rc.from_raw(new))
        f = lz.frame
        for _ in range(3):                             # (uncaptured launches first, as the other graph tests do)
            f.reset().render(SPP)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="relaxed"):
            f.render(SPP)
        torch.cuda.synchronize()
        lz.sc.regroup()
        assert lz.sc.regroup_info()["regroups"] == 1
        f.reset(colors=-1.0, pixels=1, seeds=1)
        g.replay()
        spt_check.assert_same(f, world[2]("cloud3000", new, "edit1", 0), counted=False)
        del g
        torch.cuda.synchronize()
    finally:
        lz.close()


# ---- 10. scenes without a hierarchy ------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "n255"])
def test_no_hierarchy(rt, world, monkeypatch, name):
    su._clean(monkeypatch)
    S, n, rows = world[0](name)
    lz = su.Launcher(rt, S, n, name)
    try:
        ref = world[2](name, rows, "base", 0)
        su._both(lz, ref, 0)
        lz.sc.regroup()
        assert lz.sc.regroup_info() == dict.fromkeys(lz.sc.REGROUP_INFO, 0)
        assert lz.sc.update_info() == dict.fromkeys(lz.sc.UPDATE_INFO, 0)
        su._both(lz, ref, 0)
    finally:
        lz.close()


# ---- 11. the multi-GPU frame ---------------------------------------------------------------
def test_multi_regroup_scene(rt, world):
    """SmallptMulti.update_scene and regroup_scene on two bands of one device,
    on cloud(3000) with edit 1: the frame of a fresh SmallptFrame of the
    edited scene."""
    w, h = 160, 120
    S, n, rows = world[0]("cloud3000")
    new = rc.from_raw(world[1]("cloud3000", 1))
    cam = sl.cloud_camera(w, h)
    m = rt.SmallptMulti(w, h, [0, 0], S, n)
    try:
        m.upload(rt.scenes.seeds(w, h))
        m.render(cam, 0, 2)
        m.update_scene(new)
        m.regroup_scene()
        m.upload(rt.scenes.seeds(w, h), np.zeros(3 * w * h, np.float32))
        m.render(cam, 0, 2)
        col, px = np.empty(3 * w * h, np.float32), np.empty(w * h, np.uint32)
        m.download(col, None, px)
        f = rt.SmallptFrame(w, h, spheres=new, nspheres=n, camera=cam)
        f.render(2)
        assert (col.view(np.uint32) == f.colors.view(np.uint32)).all() and (px == f.pixels).all()
    finally:
        m.close()
