"""GPU parity of the deferred shadow rays of the uncounted two-query smallpt
kernel (smallpt.hip, DQ): a lit DIFF vertex pushes its shadow ray into a
per-wave ring in LDS, the path goes on at once, and a later any-hit pass of
all 64 lanes resolves the oldest entries.  The order of the float additions
into a sample's radiance and into the running average is the reference's, so
everything here is bit-exact against the oracle -- HDR colours, RGBA8 pixels,
RNG state -- at the places the deferral can go wrong: lanes that never push
(past the frame's edge), the final drain (1 spp: every sample is a pixel's
last), progressive launches, every flush threshold from "no batching" to the
ring's largest, both block shapes and geometry paths, and scenes built to
force each flush condition (a previous sample still unfolded, no free pending
slot, an emitter term behind a pending contribution)."""
import pytest

import spt_check

pytestmark = pytest.mark.gpu

DIFF, SPEC, REFR = 0, 1, 2
SQ_MAX = 49          # sptpolicy::SQ_RING - 63: the largest threshold the ring allows


@pytest.fixture(scope="module")
def refs(oracle):
    """Oracle Cornell frames, computed once per (w, h, passes), read-only."""
    return spt_check.frame_cache(oracle)


def _same(f, ref):
    spt_check.assert_same(f, ref, counted=False)      # every launch here is uncounted


def _scene(rt, rows):
    arr = (rt.Sphere * len(rows))()
    for s, r in zip(arr, rows):
        rt.scenes._sphere(s, *r)
    return arr, len(rows)


def _camera(rt, w, h, orig, target):
    cam = rt.Camera()
    cam.orig = rt.Vec3(*orig)
    cam.target = rt.Vec3(*target)
    rt.scenes.update_camera(cam, w, h)
    return cam


@pytest.mark.parametrize("spp", [1, 2, 7])
@pytest.mark.parametrize("w,h", [(40, 24), (36, 20)])
def test_cornell_whole_and_ragged_tiles(rt, refs, w, h, spp):
    """40x24 (whole 8x8 tiles) and 36x20 (lanes past the right and bottom
    edges, which never push).  At 1 spp every sample is its pixel's last: the
    final drain runs with entries from every lane."""
    f = rt.SmallptFrame(w, h)
    f.render(spp, counters=False)
    _same(f, refs(w, h, [spp]))


def test_progressive_state(rt, refs):
    """2 spp, then first_sample = 2 continuing the stored frame, then one
    more launch: the parked sample folds into an average that started from a
    stored colour."""
    w, h = 36, 20
    f = rt.SmallptFrame(w, h)
    f.render(2, counters=False)
    f.render(3, counters=False)
    _same(f, refs(w, h, [2, 3]))
    f.render(1, counters=False)
    _same(f, refs(w, h, [2, 3, 1]))


@pytest.mark.parametrize("geo", ["lds", "global"])
@pytest.mark.parametrize("tune", ["sq=1", "sq=33", "sq=%d" % SQ_MAX, "sq=64", "wpb=16", "wpb=16,sq=1",
                                  "wpb=4,sq=17"])
def test_threshold_and_shape_sweep(rt, refs, monkeypatch, tune, geo):
    """Flush thresholds from 1 (a pass every iteration: no batching) to the
    ring's largest (64 clamps to it), the one-block-per-CU shape, and the
    global-memory geometry path."""
    monkeypatch.setenv("RT_SPT_TUNE", tune)
    if geo == "global":
        monkeypatch.setenv("RT_SPT_GEO", "global")
    w, h = 36, 20
    f = rt.SmallptFrame(w, h)
    f.render(5, counters=False)
    _same(f, refs(w, h, [5]))


@pytest.mark.parametrize("tune", ["", "sq=1", "sq=%d" % SQ_MAX])
def test_open_scene_short_samples(rt, oracle, monkeypatch, tune):
    """One light and three DIFF spheres in the open: most samples end after
    one or two iterations, sooner than the ring flushes, so a sample finishes
    while the previous one is still unfolded and a lane runs out of pending
    slots."""
    if tune:
        monkeypatch.setenv("RT_SPT_TUNE", tune)
    rows = [(6.0, (0.0, 30.0, 0.0), (12.0, 12.0, 12.0), (0.0, 0.0, 0.0), DIFF),
            (1000.0, (0.0, -1000.0, 0.0), (0, 0, 0), (.75, .75, .75), DIFF),
            (5.0, (-7.0, 5.0, 0.0), (0, 0, 0), (.75, .25, .25), DIFF),
            (4.0, (6.0, 4.0, 3.0), (0, 0, 0), (.25, .25, .75), DIFF)]
    w, h = 32, 16
    S, n = _scene(rt, rows)
    cam = _camera(rt, w, h, (0.0, 8.0, 40.0), (0.0, 5.0, 0.0))
    f = rt.SmallptFrame(w, h, spheres=S, nspheres=n, camera=cam)
    f.render(8, counters=False)
    _same(f, spt_check.oracle_frame(oracle, w, h, [8], scene=(S, n), cam=cam))


@pytest.mark.parametrize("tune", ["", "sq=1", "sq=%d" % SQ_MAX])
def test_mirror_heavy_scene(rt, oracle, monkeypatch, tune):
    """One light, a DIFF floor, SPEC and REFR everywhere else: an emitter is
    reached through specular bounces right after a lit DIFF vertex, so its
    term must wait for the pending contribution."""
    if tune:
        monkeypatch.setenv("RT_SPT_TUNE", tune)
    rows = [(8.0, (0.0, 28.0, 0.0), (10.0, 10.0, 10.0), (0.0, 0.0, 0.0), DIFF),
            (1000.0, (0.0, -1000.0, 0.0), (0, 0, 0), (.7, .7, .7), DIFF),
            (1000.0, (0.0, 0.0, -1030.0), (0, 0, 0), (.9, .9, .9), SPEC),
            (1000.0, (-1030.0, 0.0, 0.0), (0, 0, 0), (.9, .9, .9), SPEC),
            (1000.0, (1030.0, 0.0, 0.0), (0, 0, 0), (.9, .9, .9), SPEC),
            (6.0, (-9.0, 6.0, 0.0), (0, 0, 0), (.95, .95, .95), SPEC),
            (6.0, (9.0, 6.0, 4.0), (0, 0, 0), (.95, .95, .95), REFR),
            (4.0, (0.0, 4.0, 10.0), (0, 0, 0), (.95, .95, .95), REFR)]
    w, h = 32, 16
    S, n = _scene(rt, rows)
    cam = _camera(rt, w, h, (0.0, 10.0, 45.0), (0.0, 6.0, 0.0))
    f = rt.SmallptFrame(w, h, spheres=S, nspheres=n, camera=cam)
    f.render(8, counters=False)
    _same(f, spt_check.oracle_frame(oracle, w, h, [8], scene=(S, n), cam=cam))


def test_two_light_scene_keeps_the_one_query_kernel(rt, oracle):
    """Two lights: the launch must still select the one-query kernel, and
    match the oracle."""
    rows = list(rt.scenes._CORNELL) + [(3.0, (30.0, 20.0, 90.0), (6.0, 5.0, 4.0), (0.0, 0.0, 0.0), DIFF)]
    w, h = 36, 20
    S, n = _scene(rt, rows)
    f = rt.SmallptFrame(w, h, spheres=S, nspheres=n)
    f.render(3, counters=False)
    _same(f, spt_check.oracle_frame(oracle, w, h, [3], scene=(S, n)))
    import torch
    sc = rt.SmallptScene(S, n)
    f = rt.SmallptDeviceFrame(sc, rt.scenes.cornell_camera(w, h), w, h)
    f.render(1)
    torch.cuda.synchronize()
    info = sc.info()
    sc.close()
    assert info["nlights"] == 2 and not info["two_query"]
