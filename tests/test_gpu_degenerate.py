"""GPU parity on degenerate sphere data and non-finite colours: negative,
zero, denormal and non-finite radii, non-finite and huge centres
(tests/scenes_layouts.py, degenerate(kind)), an emitter with inf channels.
The reference uses a radius only as rad * rad and never hits a sphere with a
non-finite radius or centre (smallptgpu-v1.6/geomfunc.h:32-59), so every
kernel family must give the full scan's answers, bit for bit:

  * ray queries (spt_scene_query_async) on each 300-sphere kind in the 8-wide,
    binary and full-scan families, on a scene created from the kind and on one
    created from the base cloud and updated to it, against
    tests/ray_query_ref.py's numpy full scan: the 20,000 rays of
    tests/test_degenerate.py, all three query kinds;
  * frames (64 x 48, 3 samples, both estimators, counted and uncounted)
    against the oracle; one pixel-list and one radiance call;
  * a scene whose accumulators hold NaNs and infs, and spt_pack_pixels_async
    on a buffer of special values, against the oracle's toInt pack.

tests/test_gpu_scene_update.py compares the device refit with the host's on
the same kinds."""
import numpy as np
import pytest

import pixel_list_ref as plr
import radiance_ref as rr
import ray_query_ref as rq
import scenes_layouts as sl
import spt_check
from test_degenerate import MAXT, NRAYS, query_rays

pytestmark = pytest.mark.gpu

HOOKS = ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE", "RT_SPT_SCHED", "RT_SPT_DUAL",
         "RT_SPT_QUERY_BLOCKS", "RT_SPT_PIXELS_REFILL")
SPP = 3
FRAME = (64, 48)
MODES = [pytest.param(0, id="pt"), pytest.param(1, id="dl")]
# (creation hooks, the families they may give, hierarchy nodes expected)
TREE_FAMILIES = [pytest.param({}, ("GEO_WIDE",), True, id="wide"),
                 pytest.param({"RT_SPT_WIDE": "0"}, ("GEO_BVH",), True, id="binary"),
                 pytest.param({"RT_SPT_NO_BVH": "1"}, ("GEO_LDS", "GEO_GLOBAL"), False, id="scan")]
FLAT_FAMILIES = [pytest.param({}, ("GEO_LDS",), False, id="lds"),
                 pytest.param({"RT_SPT_GEO": "global"}, ("GEO_GLOBAL",), False, id="global")]


def _clean(monkeypatch, **env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def _bits(x):
    import torch
    return x.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _check_family(sc, families, tree):
    info = sc.info()
    assert info["family"] in families and (info["nodes"] > 0) == tree, info
    if families == ("GEO_WIDE",):
        assert info["leaf_max"] == 8 and info["wnodes"] > 0, info
    return info


@pytest.fixture(scope="module")
def world(oracle):
    """rays, tmax; scene(kind, small) -> (spheres, n); scan(kind) ->
    ray_query_ref.scan's answers with tmax = 30 and without a bound;
    frame(kind, small, mode) -> the oracle's frame.  Computed once, read-only."""
    rays = query_rays()
    tmax = np.full(NRAYS, MAXT, np.float32)
    scenes, scans = {}, {}
    frames = spt_check.frame_cache(oracle)

    def scene(kind, small=False):
        if (kind, small) not in scenes:
            if kind == "base":
                scenes[(kind, small)] = sl.degenerate_base()
            elif kind == "colours":
                scenes[(kind, small)] = sl.nonfinite_colours()
            else:
                scenes[(kind, small)] = sl.degenerate_small(kind) if small else sl.degenerate(kind)
        return scenes[(kind, small)]

    def scan(kind):
        if kind not in scans:
            S, n = scene(kind)
            scans[kind] = (rq.scan(S, n, rays, tmax), rq.scan(S, n, rays))
        return scans[kind]

    def frame(kind, small, mode):
        w, h = FRAME
        return frames(w, h, [SPP], mode, None, name="%s/%d" % (kind, small),
                      make=lambda: (scene(kind, small), sl.degenerate_camera(w, h)))

    return rays, tmax, scene, scan, frame


# ---- 1. ray queries -----------------------------------------------------------------
def _query_mismatches(sc, rays, tmax, refs):
    """Per query (kind, bounded): the rays whose answer differs from the scan's."""
    bounded, unbounded = refs
    out = {}
    d_rays, d_tmax = _dev(rays), _dev(tmax)
    for kind in rq.KINDS:
        t, ids = sc.query(d_rays, d_tmax, kind=kind)
        ids = ids.cpu().numpy()
        if kind == "nearest":
            rt_, ri = bounded["nearest"]
            out[(kind, True)] = np.flatnonzero((ids != ri) | (_bits(t) != rt_.view(np.uint32)))
        else:
            out[(kind, True)] = np.flatnonzero(ids != bounded[kind])
    t, ids = sc.query(d_rays, None, kind="nearest")
    rt_, ri = unbounded["nearest"]
    out[("nearest", False)] = np.flatnonzero((ids.cpu().numpy() != ri) | (_bits(t) != rt_.view(np.uint32)))
    return out


@pytest.mark.parametrize("env,families,tree", TREE_FAMILIES)
@pytest.mark.parametrize("kind", sl.DEGENERATE_KINDS)
def test_queries_equal_the_full_scan(rt, world, monkeypatch, kind, env, families, tree):
    """Created from the kind, and created from the base cloud and updated to
    the kind: nearest (with tmax = 30 and without a bound), any and occluder
    give the numpy full scan's answers on all 20,000 rays."""
    rays, tmax, scene, scan, _ = world
    _clean(monkeypatch, **env)
    S, n = scene(kind)
    refs = scan(kind)
    hits = refs[1]["nearest"][1]
    assert (hits >= 0).sum() >= NRAYS // 4 and refs[0]["any"].sum() >= NRAYS // 4
    if kind == "neg":
        assert (sl.degenerate_rows(kind)[np.maximum(hits, 0), 0] < 0)[hits >= 0].sum() >= NRAYS // 10
    created = rt.SmallptScene(S, n)
    updated = rt.SmallptScene(*scene("base"))
    try:
        updated.update(S)
        for what, sc in (("created", created), ("updated", updated)):
            _check_family(sc, families, tree)
            bad = _query_mismatches(sc, rays, tmax, refs)
            print(kind, what, {"%s%s" % (k, "" if b else "-unbounded"): len(v) for (k, b), v in bad.items()})
            for (k, b), v in bad.items():
                assert len(v) == 0, "%s, %s %s%s: %d of %d rays differ, first %d" % (
                    kind, what, k, "" if b else " without a bound", len(v), NRAYS, v[0])
        assert updated.update_info()["refits"] == (1 if tree else 0)
    finally:
        created.close()
        updated.close()


# ---- 2. frames -----------------------------------------------------------------------
class Launcher:
    """One prepared scene and a device frame."""

    def __init__(self, rt, S, n):
        w, h = FRAME
        self.sc = rt.SmallptScene(S, n)
        self.frame = rt.SmallptDeviceFrame(self.sc, sl.degenerate_camera(w, h), w, h)

    def render(self, mode, counted):
        f = self.frame.reset()
        f.render(SPP, mode=mode, counted=counted)
        return f.host() + (f.counters.tolist() if counted else None,)

    def close(self):
        self.sc.close()


def _frames(rt, monkeypatch, S, n, ref, env, families, tree, mode):
    _clean(monkeypatch, **env)
    lz = Launcher(rt, S, n)
    try:
        _check_family(lz.sc, families, tree)
        for counted in (True, False):
            spt_check.assert_same(lz.render(mode, counted), ref)
    finally:
        lz.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env,families,tree", TREE_FAMILIES)
@pytest.mark.parametrize("kind", ["neg", "mixed", "tree_nan"])
def test_frames_of_hierarchy_scenes(rt, world, monkeypatch, kind, env, families, tree, mode):
    ref = world[4](kind, False, mode)
    assert np.isfinite(ref[0]).all() and (ref[0] != 0).sum() > ref[0].size // 4      # something to show
    base = world[4]("base", False, mode)
    assert (ref[0].view(np.uint32) != base[0].view(np.uint32)).sum() > ref[0].size // 20, "the edit must reach the frame"
    _frames(rt, monkeypatch, *world[2](kind), ref, env, families, tree, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("env,families,tree", FLAT_FAMILIES)
@pytest.mark.parametrize("kind", sl.DEGENERATE_SMALL_KINDS)
def test_frames_of_small_scenes(rt, world, monkeypatch, kind, env, families, tree, mode):
    ref = world[4](kind, True, mode)
    assert np.isfinite(ref[0]).all() and (ref[0] != 0).sum() > ref[0].size // 4
    _frames(rt, monkeypatch, *world[2](kind, True), ref, env, families, tree, mode)


# ---- 3. one pixel list and one radiance call ----------------------------------------------
WL, HL = 37, 19
TAKES = np.array([0, 1, 1, 2, 3], np.int32)


@pytest.mark.parametrize("kind", ["neg", "mixed"])
def test_pixel_list(rt, world, monkeypatch, kind):
    """A permutation of all 37 x 19 pixels with takes from {0, 1, 1, 2, 3} on
    the 8-wide family: every buffer is the oracle's for each pixel's total."""
    _clean(monkeypatch)
    S, n = world[2](kind)
    cam = sl.degenerate_camera(WL, HL)
    snaps = plr.snapshots(S, n, cam, WL, HL, int(TAKES.max()), 0)
    rng = np.random.default_rng(41)
    pixels = rng.permutation(WL * HL).astype(np.int32)
    take = TAKES[rng.integers(0, len(TAKES), WL * HL)]
    totals = np.zeros(WL * HL, np.int64)
    totals[pixels] = take
    ecol, eseeds, epx, edone = plr.expected(snaps, totals.reshape(HL, WL))
    sc = rt.SmallptScene(S, n)
    try:
        _check_family(sc, ("GEO_WIDE",), True)
        frame = rt.SmallptDeviceFrame(sc, cam, WL, HL)
        frame.reset()
        frame.seeds.copy_(frame.seeds0)
        frame.render_pixels(_dev(pixels), _dev(take), mode=0)
        col, seeds, px = frame.host()
        assert (col.view(np.uint32) == ecol.view(np.uint32)).all()
        assert (seeds == eseeds).all() and (px == epx).all() and (frame.done.cpu().numpy() == edone).all()
    finally:
        sc.close()


@pytest.mark.parametrize("kind", ["neg", "mixed"])
def test_radiance(rt, world, monkeypatch, kind):
    """The 32 x 16 jittered camera rays, sample 0 of path tracing, on the
    8-wide family: radiance bits and RNG states are the oracle's ray by ray."""
    _clean(monkeypatch)
    S, n = world[2](kind)
    w, h = 32, 16
    before = rr.seeds_for(w * h)
    after, r1, r2 = rr.after_jitter(before)
    D, O = rr.camera_pairs(sl.degenerate_camera(w, h), w, h, r1, r2)
    col, seeds_out, cnt = rr.oracle_sample(S, n, D, O, before, np.zeros((w * h, 3), np.float32), 0, 0)
    assert (col != 0).any(axis=1).sum() > w * h // 8 and cnt[:, 1].sum() > 0
    sc = rt.SmallptScene(S, n)
    try:
        _check_family(sc, ("GEO_WIDE",), True)
        out, so = sc.radiance(_dev(rr.launch_rays(D, O)), _dev(after), 1, 0, 0)
        bad = np.flatnonzero((_bits(out) != col.view(np.uint32)).any(axis=1) | (_bits(so) != seeds_out).any(axis=1))
        assert len(bad) == 0, "%d of %d rays differ, first %d" % (len(bad), w * h, bad[0])
    finally:
        sc.close()


# ---- 4. non-finite colours -------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_frame_with_nonfinite_accumulators(rt, world, monkeypatch, mode):
    """An emitter (inf, 3e38, 20) over diffuse spheres with a zero colour
    channel: the oracle's accumulators hold NaNs (inf x 0) and infs, and its
    pixels the x86 conversion of a NaN (INT_MIN: bit 31 from the red channel)."""
    ref = world[4]("colours", True, mode)
    nan, inf = np.isnan(ref[0]).sum(), np.isinf(ref[0]).sum()
    print("oracle: NaN slots", nan, "inf slots", inf, "pixels with bit 31", (ref[2] >> 31).sum())
    assert nan >= 1 and inf >= 1 and (ref[2] >> 31).any()
    _frames(rt, monkeypatch, *world[2]("colours", True), ref, {}, ("GEO_LDS",), False, mode)


# ---- 5. the pixel pack ------------------------------------------------------------------------
def pack_values():
    """A 256 x 64 accumulator: every special value in every channel position
    (beside every special value in the other two), then three strides through
    [0, 1]."""
    f = np.float32
    one = f(1.0)
    nan_p, nan_n = np.array([0x7FC00000, 0xFFC00000], np.uint32).view(f)
    tiny = np.finfo(f).tiny
    special = np.array([nan_p, nan_n, np.inf, -np.inf, 0.0, -0.0, -1.0, -1e-3, -1e30, 1e-40, -1e-40, 1.4e-45, tiny,
                        1.0, np.nextafter(one, f(0)), np.nextafter(one, f(2)), 1.5, 2.0, 255.0, 1e10, 3e38,
                        np.finfo(f).max, -np.finfo(f).max, 0.5, 1e-3, 0.999], f)
    w, h = 256, 64
    col = np.empty((w * h, 3), f)
    ns = len(special)
    k = 3 * ns * ns
    i = np.arange(k)
    for c in range(3):                               # pixel i: special i % ns in channel (i // ns^2), others cycling
        col[:k, c] = special[(i // ns) % ns]
    for c in range(3):
        sel = (i // (ns * ns)) == c
        col[:k, c][sel] = special[i[sel] % ns]
    rest = w * h - k
    assert rest > 4096
    j = np.arange(rest, dtype=np.int64)[:, None]     # three strides through [0, 1], both ends included
    col[k:] = ((j * np.array([1, 37, 101])) % rest / float(rest - 1)).astype(f)
    return col.reshape(-1), w, h


def test_pack_pixels_equals_the_oracles_to_int(rt, oracle):
    import torch
    col, w, h = pack_values()
    want = oracle.smallpt_pack(col, w, h)
    c3 = col.reshape(-1, 3)
    for c in range(3):
        assert np.isnan(c3[:, c]).sum() >= 2 and np.isinf(c3[:, c]).sum() >= 2 and (c3[:, c] == np.finfo(np.float32).max).any()
    slot_nan_red = np.isnan(c3[:, 0]).reshape(h, w)[::-1].reshape(-1)             # at y * w + x
    assert (want[slot_nan_red] >> 31).all() and not (want[~slot_nan_red] >> 31).any()
    assert len(np.unique(want)) > 2000
    d_col = torch.from_numpy(col).cuda()
    px = torch.zeros(w * h, dtype=torch.int32, device="cuda")
    rt.check(rt.lib().spt_pack_pixels_async(d_col.data_ptr(), px.data_ptr(), w, h, 0, h,
                                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    got = px.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, "%d of %d pixels differ, first %d: %08x want %08x" % (len(bad), w * h, bad[0], got[bad[0]],
                                                                              want[bad[0]])
