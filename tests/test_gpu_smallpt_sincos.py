"""GPU parity of smallpt's kernels with rtm::sincos_2pi_draw in place of the
general rtm::sincosf (csrc/rt_glibc_math.h; smallpt.hip pass A and pass B,
spt_radiance.h), and sqrt_nr(1 - x2) without its range guard: every kernel
that evaluates an angle, against the oracle bit for bit -- HDR colours,
pixels, RNG states and a counted launch's four counters.  The functions
themselves are proved over all 2^23 draws by tests/test_sincos_draw.py (host)
and tests/test_gpu_sincos_draw.py (device); here the kernels call them, on
Cornell, on a small hierarchy scene (whose kernels keep the general form:
Variant::draw_trig()), through one radiance query, and on a frame whose seeds
are made so that the first light sample's and the first bounce's angles fall
on every quadrant boundary and on both ends of the draw's range."""
import numpy as np
import pytest

import radiance_ref as rr
import ray_query_ref as rq
import scenes_layouts as sl
import spt_check

pytestmark = pytest.mark.gpu

HOOKS = ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE", "RT_SPT_SCHED", "RT_SPT_DUAL",
         "RT_SPT_QUERY_BLOCKS")
DIFF = 0


def _clean(monkeypatch, **env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def refs(oracle):
    return spt_check.frame_cache(oracle)


# ---------------------------------------------------------------- oracle parity, kernel by kernel
# (kernel, environment, counted, what spt_scene_info must report of the launch)
FULL_SCAN = [
    pytest.param({}, False, {"family": "GEO_LDS", "two_query": True}, id="two_query"),
    pytest.param({}, True, {"family": "GEO_LDS", "two_query": True}, id="two_query_counted"),
    pytest.param({"RT_SPT_DUAL": "0"}, False, {"family": "GEO_LDS", "two_query": False}, id="one_query"),
    pytest.param({"RT_SPT_GEO": "global"}, False, {"family": "GEO_GLOBAL", "two_query": True}, id="global"),
    pytest.param({"RT_SPT_GEO": "global"}, True, {"family": "GEO_GLOBAL", "two_query": True}, id="global_counted"),
]


def _launch(rt, S, n, cam, w, h, spp, counted, expect):
    sc = rt.SmallptScene(S, n)
    try:
        f = rt.SmallptDeviceFrame(sc, cam, w, h).reset()
        f.render(spp, counted=counted)
        got = f.host() + (f.counters.tolist() if counted else None,)
        info = sc.info()
        for k, v in expect.items():
            assert info[k] == v, (k, info)
        return got
    finally:
        sc.close()


@pytest.mark.parametrize("env,counted,expect", FULL_SCAN)
def test_cornell_on_each_full_scan_kernel(rt, refs, monkeypatch, env, counted, expect):
    """Cornell 64x48 at 4 spp."""
    _clean(monkeypatch, **env)
    w, h, spp = 64, 48, 4
    S, n = rt.scenes.cornell()
    got = _launch(rt, S, n, rt.scenes.cornell_camera(w, h), w, h, spp, counted, expect)
    spt_check.assert_same(got, refs(w, h, [spp]), counted=counted)


@pytest.mark.parametrize("counted", [False, True], ids=["uncounted", "counted"])
@pytest.mark.parametrize("env,family", [({}, "GEO_WIDE"), ({"RT_SPT_WIDE": "0"}, "GEO_BVH")], ids=["wide8", "binary"])
def test_hierarchy_kernels(rt, refs, monkeypatch, env, family, counted):
    """The smallest scene above sptbvh::MIN_SPHERES (256 spheres, three
    lights), 64x48 at 4 spp, on the 8-wide and the binary walk."""
    _clean(monkeypatch, **env)
    w, h, spp = 64, 48, 4
    S, n = sl.n256()
    ref = refs(w, h, [spp], name="n256", make=lambda: ((S, n), sl.small_camera(w, h)))
    got = _launch(rt, S, n, sl.small_camera(w, h), w, h, spp, counted, {"family": family})
    spt_check.assert_same(got, ref, counted=counted)


# ---------------------------------------------------------------- one radiance query
def test_radiance_query_of_4096_rays(rt, monkeypatch):
    """spt_scene_radiance_async on Cornell, 4,096 rays in one batch (2,048
    jittered camera rays, 2,048 aimed at sphere centres from inside the room),
    path tracing: radiance and states against tests/radiance_ref.py."""
    import torch
    _clean(monkeypatch)
    S, n = rt.scenes.cornell()
    step = rr.reference(S, n, rt.scenes.cornell_camera, (64, 32), 4096, 0, samples=1, box=rr.CORNELL_ROOM)[0]
    assert step["cnt"][:, 1].sum() > 1000                       # shadow rays: light samples were drawn
    sc = rt.SmallptScene(S, n)
    try:
        rays = torch.from_numpy(step["rays"]).cuda()
        seeds = torch.from_numpy(step["seeds_in"].view(np.int32)).cuda()
        out, so = sc.radiance(rays, seeds, 1, 0, 0)
        got = out.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
        gs = so.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
    finally:
        sc.close()
    bad = np.flatnonzero((got != step["col"].view(np.uint32)).any(axis=1) | (gs != step["seeds_out"]).any(axis=1))
    assert len(bad) == 0, "%d of 4096 rays differ, first %d" % (len(bad), bad[0])


# ---------------------------------------------------------------- quadrant edges
Q = 1 << 20
EDGE_M = [0, 1, Q - 1, Q, 3 * Q - 1, 3 * Q, 5 * Q - 1, 5 * Q, 7 * Q - 1, 7 * Q, (1 << 23) - 1]
A0, A1 = 36969, 18000                                           # simplernd.h's two multipliers


def _state_before(m, rng):
    """An MWC state whose next draw has mantissa m: s1 is searched so that
    18000 * lo + hi has m's low 16 bits, s0 so that the low seven bits of
    36969 * lo + hi supply the rest; both stay below a * 2^16 so that
    _step_back can undo a draw."""
    while True:
        lo1 = int(rng.integers(1, 65536))
        hi1 = (m - A1 * lo1) % 65536
        if hi1 < A1 - 1:
            break
    n1 = A1 * lo1 + hi1
    need = (((m - n1) % (1 << 23)) >> 16) & 0x7f
    lo0 = int(rng.integers(1, 65536))
    hi0 = (need - A0 * lo0) % 128 + 128 * int(rng.integers(0, 256))
    return (hi0 << 16) | lo0, (hi1 << 16) | lo1


def _step_back(s0, s1):
    """A state that one draw turns into (s0, s1)."""
    return ((s0 % A0) << 16) | (s0 // A0), ((s1 % A1) << 16) | (s1 // A1)


def _mantissa_of_draw(s0, s1, k):
    """The mantissas of the k-th draw (1-based) from the states, as GetRandom makes them."""
    for _ in range(k):
        v, s0, s1 = rt_scenes().mwc_draw(s0, s1)
    return np.rint(v.astype(np.float64) * (1 << 23)).astype(np.int64)


def rt_scenes():
    import rtamd
    return rtamd.scenes


def test_angles_on_every_quadrant_boundary(rt, oracle, monkeypatch):
    """16x8 Cornell at 1 spp from hand-made seeds.  A pixel's draws are the
    camera's two, then -- its first hit being a DIFF surface that emits
    nothing -- the light sample's u2 (the angle; third draw) and u1, then the
    bounce's r1 (the angle; fifth draw).  Every m of EDGE_M is given to the
    third draw of some pixels and to the fifth draw of others; the test first
    shows, from the camera rays' first hits, that each is met at such a
    pixel, then compares the frame with the oracle's from the same seeds."""
    _clean(monkeypatch)
    w, h = 16, 8
    S, n = rt.scenes.cornell()
    cam = rt.scenes.cornell_camera(w, h)
    rng = np.random.default_rng(17)
    seeds = np.empty((w * h, 2), np.uint32)
    want = []
    for i in range(w * h):
        m, k = EDGE_M[i % len(EDGE_M)], (3, 5)[(i // len(EDGE_M)) % 2]
        s = _state_before(m, rng)
        for _ in range(k - 1):
            s = _step_back(*s)
        assert s[0] >= 2 and s[1] >= 2
        seeds[i] = s
        want.append((m, k))
    for k in (3, 5):
        got = _mantissa_of_draw(seeds[:, 0], seeds[:, 1], k)
        assert all(got[i] == m for i, (m, kk) in enumerate(want) if kk == k)
    # the pixels whose first hit is a DIFF surface that emits nothing
    i = np.arange(w * h)
    x, y = i % w, h - 1 - i // w                                # slot i = (h - y - 1) * w + x
    _, r1, r2 = rr.after_jitter(seeds)
    first = rq.scan(S, n, rt.scenes.camera_rays(cam, w, h, x, y, r1, r2))["nearest"][1]
    rows = sl.rows_of(S, n)
    plain = (first >= 0) & (rows[first, 10].view(np.int32) == DIFF) & (rows[first, 4:7] == 0).all(axis=1)
    for k in (3, 5):
        met = {m for j, (m, kk) in enumerate(want) if kk == k and plain[j]}
        assert met == set(EDGE_M), (k, sorted(set(EDGE_M) - met))
    # the oracle's frame and the kernel's, from those seeds
    col = np.zeros(3 * w * h, np.float32)
    px = np.zeros(w * h, np.uint32)
    oseeds = seeds.reshape(-1).copy()
    cnt = oracle.smallpt_render(S, n, cam, col, oseeds, px, w, h, 0, 1)
    for counted in (False, True):
        f = rt.SmallptFrame(w, h)
        f.seeds[:] = seeds.reshape(-1)
        f.render(1, counters=counted)
        spt_check.assert_same(f, (col, oseeds, px, tuple(cnt)), counted=counted)
