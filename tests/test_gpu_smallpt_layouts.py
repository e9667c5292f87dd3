"""GPU parity of smallpt's hierarchy kernels at the layouts a scene picks on
its own (tests/scenes_layouts.py): 8-wide trees with leaves of 12 and 16
spheres, the binary walk a scene falls back to when no 8-wide tree fits, the
cooperative walks (eight, four and two lanes per pixel) on scenes with SPEC
and REFR spheres, several lights and direct lighting, the edges of the
always / tree partition, frames smaller than one block, and the dynamic LDS
each kernel family's launch asks for (csrc/spt_layout.h, restated here).

The reference is always the oracle's full scan (oracle.smallpt_render, the
restatement of Intersect / IntersectP), computed once per (scene, frame,
mode); every comparison is bit for bit -- HDR colours, seeds, pixels, and all
four counters of a counted launch.  Every case first asserts through
spt_scene_info (SmallptScene.info) the kernel family, leaf size and tier it
means to run, so none can pass on another path."""
import numpy as np
import pytest

import scenes_layouts as sl
import spt_check

pytestmark = pytest.mark.gpu

SPP = 2
MODES = [pytest.param(0, id="pt"), pytest.param(1, id="dl")]
FRAME = (64, 48)        # 24 tiles in six groups: one persistent block


@pytest.fixture(scope="module")
def world(oracle):
    """Scenes (built once) and oracle frames (computed once per scene, frame,
    window and mode; read-only)."""
    scenes = {}
    frames = spt_check.frame_cache(oracle)

    def scene(name):
        if name not in scenes:
            if name in sl.LAYOUT_SCENES:
                S, n = sl.cloud(sl.LAYOUT_SCENES[name][0])
                cam = sl.cloud_camera
            elif name == "n255":
                (S, n), cam = sl.n255(), sl.small_camera
            elif name == "cornell":
                import rtamd
                (S, n), cam = rtamd.scenes.cornell(), rtamd.scenes.cornell_camera
            else:
                make, cam = sl.EDGE_SCENES[name]
                S, n = make()
            scenes[name] = (S, n, cam)
        return scenes[name]

    def ref(name, w, h, mode, rows=None):
        S, n, cam = scene(name)
        return frames(w, h, [SPP], mode, rows, name=name, make=lambda: ((S, n), cam(w, h)))

    return scene, ref


class Launcher:
    """One prepared scene and a device frame of one size."""

    def __init__(self, rt, S, n, cam, w, h):
        import torch
        self.sc = rt.SmallptScene(S, n)
        self.frame = rt.SmallptDeviceFrame(self.sc, cam, w, h)
        self.all_groups = torch.arange(self.frame.groups_total, dtype=torch.int32, device=self.frame.device)

    def render(self, mode, counted, as_list=False, rows=None):
        """One launch of SPP samples from the initial state into the zeroed
        frame: (colours, seeds, pixels, counters or None).  as_list: the whole
        frame as a group list without a cost pointer (an order, so the tiers
        apply)."""
        f = self.frame.reset()
        f.render(SPP, mode=mode, counted=counted, rows=rows, groups=self.all_groups if as_list else None)
        return f.host() + (f.counters.tolist() if counted else None,)

    def close(self):
        self.sc.close()


def _open(rt, world, name, w, h):
    S, n, cam = world[0](name)
    return Launcher(rt, S, n, cam(w, h), w, h)


def _counted_and_uncounted(lz, ref, mode, expect, **kw):
    """A counted and an uncounted launch, both equal to the oracle's frame
    (so the uncounted launch gives the counted one's bits); after each, the
    launch words of info() must contain `expect`."""
    for counted in (True, False):
        before = lz.sc.info()["launches"]
        got = lz.render(mode, counted, **kw)
        info = lz.sc.info()
        assert info["launches"] == before + 1
        for k, v in expect.items():
            assert info[k] == v, (k, info)
        spt_check.assert_same(got, ref)     # HDR bits, seeds, pixels, a counted launch's four counters


# ---- layouts -------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["leaf12", "leaf16", "nowide"])
def test_layouts_the_library_picks(rt, world, monkeypatch, name, mode):
    """No environment variable set: cloud(30,000) walks an 8-wide tree with
    leaves of up to 12 spheres (three four-sphere passes per leaf), cloud(43,000)
    one with leaves of 16, cloud(56,000) fits no 8-wide tree and walks the
    binary one."""
    for k in ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE"):
        monkeypatch.delenv(k, raising=False)
    w, h = FRAME
    lz = _open(rt, world, name, w, h)
    try:
        info = lz.sc.info()
        n, leaf = sl.LAYOUT_SCENES[name]
        assert info["nspheres"] == n and info["nlights"] == 3 and info["nalways"] == 2 and not info["no_refr"]
        assert info["launches"] == 0
        if leaf:
            assert info["family"] == "GEO_WIDE" and info["leaf_max"] == leaf and info["wdepth"] >= 2, info
        else:
            assert info["family"] == "GEO_BVH" and info["leaf_max"] == 0 and info["wnodes"] == 0, info
        assert info["nodes"] > n // 4
        _counted_and_uncounted(lz, world[1](name, w, h, mode), mode, {"cg": 0, "two_query": False})
        if leaf:
            # the last launch was uncounted: the nodes without the counted walk's 32 B of
            # highest indices each, and one 256-B stack level per wave and level below the root
            assert lz.sc.info()["lds_bytes"] == 112 * info["wnodes"] + 16 * 256 * (info["wdepth"] - 1)
    finally:
        lz.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["leaf12", "leaf16"])
def test_binary_walk_on_the_large_trees(rt, world, monkeypatch, name, mode):
    """RT_SPT_WIDE=0 on the leaf-12 and leaf-16 scenes: the binary walk over
    trees other than configs[4]'s."""
    monkeypatch.setenv("RT_SPT_WIDE", "0")
    w, h = FRAME
    lz = _open(rt, world, name, w, h)
    try:
        info = lz.sc.info()
        assert info["family"] == "GEO_BVH" and info["leaf_max"] == 0 and info["nalways"] == 2, info
        _counted_and_uncounted(lz, world[1](name, w, h, mode), mode, {"cg": 0})
    finally:
        lz.close()


# ---- cooperative tiers -----------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("G", [8, 4, 2])
@pytest.mark.parametrize("name", ["leaf8", "leaf12", "leaf16"])
def test_cooperative_tiers_forced_in_one_launch(rt, world, monkeypatch, name, G, mode):
    """wide_walk_coop<G> on scenes with SPEC and REFR spheres and three
    lights, in both estimators: the whole frame as a list (an order, so the
    tiers apply at the first launch) with every tile cooperative."""
    w, h = FRAME
    ntiles = ((w + 7) // 8) * ((h + 7) // 8)
    monkeypatch.setenv("RT_SPT_TUNE", "coop=%d,coop_g=%d" % (ntiles, G))
    lz = _open(rt, world, name, w, h)
    try:
        info = lz.sc.info()
        assert info["family"] == "GEO_WIDE" and info["leaf_max"] == sl.LAYOUT_SCENES[name][1], info
        _counted_and_uncounted(lz, world[1](name, w, h, mode), mode, {"cg": G, "n1": ntiles, "n2": 0},
                               as_list=True)
    finally:
        lz.close()


def test_cooperative_tier_of_a_learnt_order(rt, world, monkeypatch):
    """The same key launched three times through spt_scene_render_async: the
    first launch records the tile costs, and by the third the learnt order is
    in use with the window class's default tier -- at this size eight lanes
    per pixel.  Direct lighting on cloud(3000); uncounted launches and
    counted ones (which learn an order of their own); every frame equals the
    oracle's."""
    monkeypatch.delenv("RT_SPT_TUNE", raising=False)
    monkeypatch.delenv("RT_SPT_SCHED", raising=False)
    w, h = FRAME
    lz = _open(rt, world, "leaf8", w, h)
    try:
        ref = world[1]("leaf8", w, h, 1)
        for counted in (False, True):
            for i in range(3):
                spt_check.assert_same(lz.render(1, counted), ref)
                info = lz.sc.info()
                if i == 0:
                    assert info["cg"] == 0 and info["n1"] == 0, info       # no order yet: a lane per pixel
            assert info["family"] == "GEO_WIDE" and info["cg"] == 8 and info["n1"] > 0, info
    finally:
        lz.close()


# ---- edges of the partition -------------------------------------------------
WALKS = [pytest.param("wide", id="wide"), pytest.param("binary", id="binary"), pytest.param("coop8", id="coop8")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("walk", WALKS)
@pytest.mark.parametrize("name", list(sl.EDGE_SCENES))
def test_partition_edges(rt, world, monkeypatch, name, walk, mode):
    """No always sphere; more candidates than MAX_ALWAYS (four huge spheres
    in the tree); the smallest tree; spheres sharing a centre and exact
    duplicates (the tie rule shows in the colour and in the counters)."""
    w, h = FRAME
    ntiles = ((w + 7) // 8) * ((h + 7) // 8)
    monkeypatch.delenv("RT_SPT_TUNE", raising=False)
    if walk == "binary":
        monkeypatch.setenv("RT_SPT_WIDE", "0")
    if walk == "coop8":
        monkeypatch.setenv("RT_SPT_TUNE", "coop=%d,coop_g=8" % ntiles)
    lz = _open(rt, world, name, w, h)
    try:
        info = lz.sc.info()
        assert info["family"] == ("GEO_BVH" if walk == "binary" else "GEO_WIDE"), info
        assert info["leaf_max"] == (0 if walk == "binary" else 8)
        assert info["nalways"] == {"no_always": 0, "many_always": 16, "n256": 1, "coincident": 1}[name], info
        expect = {"cg": 8, "n1": ntiles} if walk == "coop8" else {"cg": 0}
        _counted_and_uncounted(lz, world[1](name, w, h, mode), mode, expect, as_list=walk == "coop8")
    finally:
        lz.close()


@pytest.mark.parametrize("mode", MODES)
def test_one_sphere_below_the_threshold(rt, world, mode):
    """n256 without its last sphere gets no hierarchy: the LDS full scan."""
    w, h = FRAME
    lz = _open(rt, world, "n255", w, h)
    try:
        info = lz.sc.info()
        assert info["family"] == "GEO_LDS" and info["nspheres"] == 255 and info["nodes"] == 0, info
        _counted_and_uncounted(lz, world[1]("n255", w, h, mode), mode, {"cg": 0, "two_query": False})
    finally:
        lz.close()


# ---- tiny frames -------------------------------------------------------------
TINY = [(1, 1), (9, 3), (7, 70)]
TARGETS = [pytest.param("leaf8", {}, "GEO_WIDE", id="cloud-wide"),
           pytest.param("leaf8", {"RT_SPT_WIDE": "0"}, "GEO_BVH", id="cloud-binary"),
           pytest.param("cornell", {"RT_SPT_TUNE": "wpb=4"}, "GEO_LDS", id="cornell-wpb4"),
           pytest.param("cornell", {"RT_SPT_TUNE": "wpb=16"}, "GEO_LDS", id="cornell-wpb16")]


def _tiny_open(rt, world, monkeypatch, name, env, family, w, h):
    monkeypatch.delenv("RT_SPT_TUNE", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    lz = _open(rt, world, name, w, h)
    assert lz.sc.info()["family"] == family
    return lz


@pytest.mark.parametrize("name,env,family", TARGETS)
@pytest.mark.parametrize("w,h", TINY)
def test_tiny_frames(rt, world, monkeypatch, w, h, name, env, family):
    """Frames of one pixel, of one ragged tile row and of one ragged tile
    column: the persistent grid is one block of mostly idle waves."""
    lz = _tiny_open(rt, world, monkeypatch, name, env, family, w, h)
    try:
        ntiles = ((w + 7) // 8) * ((h + 7) // 8)
        expect = {"cg": 0, "two_query": name == "cornell"}
        if family == "GEO_WIDE":
            expect.update(wpb=16, nblocks=1)                   # fewer tiles than one block's waves
        elif family == "GEO_LDS":
            wpb = int(env["RT_SPT_TUNE"][4:])
            expect.update(wpb=wpb, nblocks=(ntiles + wpb - 1) // wpb)
        for mode in (0, 1):
            if mode == 1:
                expect["two_query"] = False
            _counted_and_uncounted(lz, world[1](name, w, h, mode), mode, expect)
    finally:
        lz.close()


@pytest.mark.parametrize("name,env,family", TARGETS)
def test_tiny_frame_row_window(rt, world, monkeypatch, name, env, family):
    """9x3, rows [1, 2): the window's row equals the oracle's and every
    colour, pixel and seed slot outside it keeps its sentinel."""
    w, h, r0, r1 = 9, 3, 1, 2
    lz = _tiny_open(rt, world, monkeypatch, name, env, family, w, h)
    try:
        S, n, cam = world[0](name)
        for mode in (0, 1):
            full = world[1](name, w, h, mode)                      # pixels are independent: the window's slots
            ref = world[1](name, w, h, mode, (r0, r1))             # ... and the oracle's own window render agree
            inside = np.zeros((h, w), bool)
            inside[h - r1:h - r0] = True                           # accumulator and seed rows are flipped
            ins = inside.reshape(-1)
            assert (ref[0].view(np.uint32).reshape(-1, 3)[ins] == full[0].view(np.uint32).reshape(-1, 3)[ins]).all()
            f = lz.frame.reset(colors=-7.25, pixels=0x25A5A5A5, seeds=0x5EADBEEF)
            f.render(SPP, mode=mode, counted=True, rows=(r0, r1))
            gcol, gs, gpx = f.host()
            gcol, gs, gpx = gcol.reshape(-1, 3), gs.reshape(-1, 2), gpx.reshape(h, w)
            assert (gcol[ins].view(np.uint32) == ref[0].reshape(-1, 3)[ins].view(np.uint32)).all()
            assert (gcol[~ins] == np.float32(-7.25)).all()
            assert (gpx[r0:r1] == ref[2].reshape(h, w)[r0:r1]).all()
            assert (np.delete(gpx, np.s_[r0:r1], 0) == 0x25A5A5A5).all()
            assert (gs[ins] == ref[1].reshape(-1, 2)[ins]).all() and (gs[~ins] == 0x5EADBEEF).all()
            assert tuple(f.counters.tolist()) == ref[3], (f.counters.tolist(), ref[3])
    finally:
        lz.close()


# ---- LDS bytes per family ---------------------------------------------------
# The figures of DESIGN.md §3's table, restated: 16 B per scene record, a 64-B
# head, 768 B per wave (the parked colour) or 5,440 B (with the deferred shadow
# rays' slots and ring), a 6,160-B strip per tile group, and at least 81 KiB
# for a 16-wave block.
SMALL = (40, 24)        # 15 tiles: one 16-wave block, four 4-wave ones
RESERVED = 81 * 1024


def _full_scan_bytes(records, wpb, deferred):
    b = 16 * records + 64 + wpb * (5440 if deferred else 768)
    return max(b, RESERVED) if wpb == 16 else b


@pytest.mark.parametrize("geo", [None, "global"])
@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("wpb", [4, 16])
def test_lds_bytes_of_the_full_scan_kernels(rt, world, monkeypatch, wpb, counted, geo):
    """Cornell (9 spheres, one light: 30 records), path tracing: the bytes
    each launch asks for, in both block shapes, uncounted (the two-query
    kernel with deferred shadow rays) and counted, with the scene copied into
    LDS and (RT_SPT_GEO=global) read from global memory -- no copy then."""
    monkeypatch.setenv("RT_SPT_TUNE", "wpb=%d" % wpb)
    monkeypatch.delenv("RT_SPT_GEO", raising=False)
    if geo:
        monkeypatch.setenv("RT_SPT_GEO", geo)
    w, h = SMALL
    lz = _open(rt, world, "cornell", w, h)
    try:
        assert lz.sc.info()["family"] == ("GEO_GLOBAL" if geo else "GEO_LDS")
        got = lz.render(0, counted)
        info = lz.sc.info()
        assert info["wpb"] == wpb and info["two_query"], info
        want = _full_scan_bytes(0 if geo else 30, wpb, not counted)
        if not geo:
            assert want == {(4, False): 22304, (16, False): 87584, (4, True): 480 + 64 + 4 * 768,
                            (16, True): 82944}[(wpb, counted)]
        assert info["lds_bytes"] == want, info
        spt_check.assert_same(got, world[1]("cornell", w, h, 0))
    finally:
        lz.close()


@pytest.mark.parametrize("wpb", [4, 16])
def test_lds_bytes_of_the_binary_walk(rt, world, monkeypatch, wpb):
    """The smallest hierarchy scene with RT_SPT_WIDE=0: one staging strip per
    tile group of the block, (wpb / 4) * 6160 B -- and for the 16-wave block
    the reservation that keeps it alone on its CU, as for every 16-wave block
    but the 8-wide kernels'."""
    monkeypatch.setenv("RT_SPT_WIDE", "0")
    monkeypatch.setenv("RT_SPT_TUNE", "wpb=%d" % wpb)
    w, h = SMALL
    lz = _open(rt, world, "n256", w, h)
    try:
        assert lz.sc.info()["family"] == "GEO_BVH"
        got = lz.render(0, False)
        info = lz.sc.info()
        assert info["wpb"] == wpb, info
        strips = (wpb // 4) * 6160
        assert info["lds_bytes"] == (strips if wpb == 4 else max(strips, RESERVED)), info
        spt_check.assert_same(got, world[1]("n256", w, h, 0))
    finally:
        lz.close()


@pytest.mark.parametrize("n,kept", [(1500, True), (1700, False)])
def test_lds_family_only_while_its_block_fits_a_cu(rt, monkeypatch, n, kept):
    """A one-light cloud scanned in full (RT_SPT_NO_BVH), uncounted, in the
    16-wave block shape: sixteen waves' rings take 87,104 B, so the scene copy
    fits beside them up to 1,597 spheres.  1,500 spheres launch the LDS family;
    1,700 -- still the LDS family by the scene's size -- launch the global-
    memory kernel of the same variant, inside a CU's 160 KiB.  Either way the
    frame equals the one RT_SPT_GEO=global renders, bit for bit."""
    monkeypatch.setenv("RT_SPT_NO_BVH", "1")
    monkeypatch.setenv("RT_SPT_TUNE", "wpb=16")
    w, h = SMALL
    S, ns = sl.cloud_one_light(n)
    frames = []
    for geo in (None, "global"):
        monkeypatch.delenv("RT_SPT_GEO", raising=False)
        if geo:
            monkeypatch.setenv("RT_SPT_GEO", geo)
        lz = Launcher(rt, S, ns, sl.cloud_camera(w, h), w, h)
        try:
            info = lz.sc.info()
            assert info["family"] == ("GEO_GLOBAL" if geo else "GEO_LDS") and info["nlights"] == 1, info
            assert info["nodes"] == 0
            frames.append(lz.render(0, False))
            info = lz.sc.info()
            assert info["family"] == ("GEO_GLOBAL" if geo else "GEO_LDS")       # the scene's family, whatever ran
            assert info["wpb"] == 16 and info["two_query"], info
            assert info["lds_bytes"] <= 163840, info
            assert info["lds_bytes"] == _full_scan_bytes(3 * n + 3 if kept and not geo else 0, 16, True), info
        finally:
            lz.close()
    spt_check.assert_same(frames[0], frames[1])       # colours, seeds, pixels
