"""GPU parity of the one-light (two-query) smallpt kernels without a light
index, with the push and the owners' step of a flush pass in straight-line
code (smallpt.hip: pass_a under DUAL, the DQ branch; spt_policy.h sq_owners),
against the oracle bit for bit -- HDR colours, pixels, RNG states, and the
four counters where the kernel keeps them.  Cornell on each full-scan kernel;
small frames at 64 spp, where most samples end behind a parked one and folds
are frequent, one of them continuing a stored frame; scenes with two and three
emitters, which must stay on the one-query kernel and its several-lights loop;
and a one-light scene whose light lies at floor level, so that most light
samples yield no shadow ray and the bounce follows in the same iteration.
The owners' step itself is enumerated on the CPU by tests/test_owners_step.py."""
import pytest

import spt_check

pytestmark = pytest.mark.gpu

HOOKS = ("RT_SPT_WIDE", "RT_SPT_NO_BVH", "RT_SPT_GEO", "RT_SPT_TUNE", "RT_SPT_SCHED", "RT_SPT_DUAL",
         "RT_SPT_QUERY_BLOCKS")
DIFF, SPEC, REFR = 0, 1, 2


def _clean(monkeypatch, **env):
    for k in HOOKS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.fixture(scope="module")
def refs(oracle):
    return spt_check.frame_cache(oracle)


def _scene(rt, rows):
    arr = (rt.Sphere * len(rows))()
    for s, r in zip(arr, rows):
        rt.scenes._sphere(s, *r)
    return arr, len(rows)


def _launch(rt, S, n, cam, w, h, steps, counted, expect):
    """The frame after the progressive launches `steps` on a prepared scene,
    as (colors, seeds, pixels, the last launch's counters or None), after
    checking what spt_scene_info reports of the launch."""
    sc = rt.SmallptScene(S, n)
    try:
        f = rt.SmallptDeviceFrame(sc, cam, w, h).reset()
        first = 0
        for spp in steps:
            f.render(spp, first_sample=first, seeds_in=f.seeds if first else None, counted=counted)
            first += spp
        got = f.host() + (f.counters.tolist() if counted else None,)
        info = sc.info()
        for k, v in expect.items():
            assert info[k] == v, (k, info)
        return got
    finally:
        sc.close()


# (environment, counted, what spt_scene_info must report of the launch)
FULL_SCAN = [
    pytest.param({}, False, {"family": "GEO_LDS", "two_query": True}, id="two_query"),
    pytest.param({}, True, {"family": "GEO_LDS", "two_query": True}, id="two_query_counted"),
    pytest.param({"RT_SPT_GEO": "global"}, False, {"family": "GEO_GLOBAL", "two_query": True}, id="global"),
    pytest.param({"RT_SPT_GEO": "global"}, True, {"family": "GEO_GLOBAL", "two_query": True}, id="global_counted"),
    pytest.param({"RT_SPT_DUAL": "0"}, False, {"family": "GEO_LDS", "two_query": False}, id="one_query"),
]


@pytest.mark.parametrize("env,counted,expect", FULL_SCAN)
def test_cornell_on_each_full_scan_kernel(rt, refs, monkeypatch, env, counted, expect):
    """Cornell 64x48 at 4 spp."""
    _clean(monkeypatch, **env)
    w, h, spp = 64, 48, 4
    S, n = rt.scenes.cornell()
    got = _launch(rt, S, n, rt.scenes.cornell_camera(w, h), w, h, [spp], counted, expect)
    spt_check.assert_same(got, refs(w, h, [spp]), counted=counted)


@pytest.mark.parametrize("w,h,steps", [(8, 8, [64]), (16, 8, [3, 64])], ids=["8x8", "16x8_from_3"])
def test_many_parked_samples(rt, refs, monkeypatch, w, h, steps):
    """64 spp on one and two tiles: a lane finishes a sample every few
    iterations, mostly with terms still pending, so parked samples, folds and
    two-entry resolutions are the rule; 16x8 continues a stored 3-spp frame
    (first_sample = 3: the fold's sample number starts above zero)."""
    _clean(monkeypatch)
    S, n = rt.scenes.cornell()
    got = _launch(rt, S, n, rt.scenes.cornell_camera(w, h), w, h, steps, False, {"two_query": True})
    spt_check.assert_same(got, refs(w, h, steps), counted=False)


EMITTERS = [(3.0, (30.0, 20.0, 90.0), (6.0, 5.0, 4.0), (0.0, 0.0, 0.0), DIFF),
            (2.0, (75.0, 50.0, 60.0), (3.0, 7.0, 5.0), (0.0, 0.0, 0.0), DIFF)]


@pytest.mark.parametrize("counted", [False, True], ids=["uncounted", "counted"])
@pytest.mark.parametrize("extra", [1, 2], ids=["two_emitters", "three_emitters"])
def test_several_lights_keep_the_one_query_kernel(rt, oracle, monkeypatch, extra, counted):
    """Cornell with one and two more emitting spheres, 32x24 at 4 spp: the
    several-lights loop of pass A, on the one-query kernel."""
    _clean(monkeypatch)
    w, h, spp = 32, 24, 4
    S, n = _scene(rt, list(rt.scenes._CORNELL) + EMITTERS[:extra])
    cam = rt.scenes.cornell_camera(w, h)
    got = _launch(rt, S, n, cam, w, h, [spp], counted, {"nlights": 1 + extra, "two_query": False})
    spt_check.assert_same(got, spt_check.oracle_frame(oracle, w, h, [spp], scene=(S, n), cam=cam), counted=counted)


@pytest.mark.parametrize("counted", [False, True], ids=["uncounted", "counted"])
def test_light_at_floor_level(rt, oracle, monkeypatch, counted):
    """One light half sunk into a large floor sphere at the frame's side, and
    three DIFF spheres standing on the floor: for the floor beyond the light's
    horizon and for the spheres' far sides the light is below the surface
    (wi <= 0), and half of the light's sample points face away (wo <= 0), so
    most DIFF vertices draw a light sample that yields no shadow ray and
    bounce in the same iteration."""
    _clean(monkeypatch)
    rows = [(3.0, (34.0, 0.5, 0.0), (14.0, 12.0, 10.0), (0.0, 0.0, 0.0), DIFF),
            (1000.0, (0.0, -1000.0, 0.0), (0, 0, 0), (.75, .75, .75), DIFF),
            (5.0, (-7.0, 5.0, 0.0), (0, 0, 0), (.75, .25, .25), DIFF),
            (4.0, (6.0, 4.0, 3.0), (0, 0, 0), (.25, .25, .75), DIFF),
            (3.0, (18.0, 3.0, -6.0), (0, 0, 0), (.25, .75, .25), DIFF)]
    w, h, spp = 32, 16, 8
    S, n = _scene(rt, rows)
    cam = rt.Camera()
    cam.orig = rt.Vec3(0.0, 8.0, 40.0)
    cam.target = rt.Vec3(4.0, 4.0, 0.0)
    rt.scenes.update_camera(cam, w, h)
    got = _launch(rt, S, n, cam, w, h, [spp], counted, {"nlights": 1, "two_query": True})
    ref = spt_check.oracle_frame(oracle, w, h, [spp], scene=(S, n), cam=cam)
    if counted:     # the scene does what it is built for: fewer shadow rays than a third of the path rays
        assert 0 < ref[3][1] < ref[3][0] // 3, ref[3]
    spt_check.assert_same(got, ref, counted=counted)
