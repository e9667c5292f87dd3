"""GPU parity of the full-scan smallpt kernels' held LDS addresses: a lane's
parking address (head + wave x WAVE_DW + lane, smallpt.hip's park_ptr) and
its wave's ring base (ring_ptr) are computed once per wave before the pixel
loop and kept for the whole launch.  A held address can be wrong per wave
(the wave index times WAVE_DW), per lane, per block shape (wave indices 4-15
exist only in a 16-wave block) or per family (the parking area follows the
scene copy, or starts at 0 when the spheres are read from global memory), so
every case renders a frame of several blocks with ragged right and bottom
tiles and compares it with the oracle bit for bit -- HDR colours, RGBA8
pixels, RNG state, and the counters of a counted launch.

72x40 is 9 x 5 tiles of 8x8: 45 waves, twelve 4-wave blocks (or three
16-wave ones), a half-filled last tile row and a last group of one tile, so
there are lanes without a pixel that still pop ring entries."""
import pytest

import scenes_layouts as sl
import spt_check

pytestmark = pytest.mark.gpu

W, H, SPP = 72, 40, 8
SHAPES = ["wpb=4", "wpb=16"]


@pytest.fixture(scope="module")
def refs(oracle):
    """Oracle frames, computed once per key, read-only."""
    return spt_check.frame_cache(oracle)


def _many_lights(w, h):
    """scenes_layouts.n255: 255 spheres scanned in full, three of them lights."""
    return sl.n255(), sl.small_camera(w, h)


def _env(monkeypatch, tune="", geo="", dual=""):
    for k, v in (("RT_SPT_TUNE", tune), ("RT_SPT_GEO", geo), ("RT_SPT_DUAL", dual)):
        if v:
            monkeypatch.setenv(k, v)
        else:
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("geo", ["", "global"])
@pytest.mark.parametrize("sq", ["", "sq=1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_first_frame_then_continued(rt, refs, monkeypatch, shape, sq, geo):
    """The uncounted two-query kernel (ring and parked slots): 8 spp from
    first_sample 0, then 8 more from first_sample 8 -- the parked colour
    starts from `colors`.  sq=1 flushes every iteration; the default
    threshold fills both pending slots and parks `rad`."""
    _env(monkeypatch, tune=",".join(t for t in (shape, sq) if t), geo=geo)
    f = rt.SmallptFrame(W, H)
    f.render(SPP, counters=False)
    spt_check.assert_same(f, refs(W, H, [SPP]), counted=False)
    f.render(SPP, counters=False)
    spt_check.assert_same(f, refs(W, H, [SPP, SPP]), counted=False)


@pytest.mark.parametrize("geo", ["", "global"])
@pytest.mark.parametrize("shape", SHAPES)
def test_counted_first_frame(rt, refs, monkeypatch, shape, geo):
    """The counted two-query kernel (parked colour, no ring): the frame and
    all four counters equal the oracle's; then the continued launch."""
    _env(monkeypatch, tune=shape, geo=geo)
    f = rt.SmallptFrame(W, H)
    f.render(SPP, counters=True)
    spt_check.assert_same(f, refs(W, H, [SPP]), counted=True)
    f.render(SPP, counters=True)
    spt_check.assert_same(f, refs(W, H, [SPP, SPP]), counted=True)


@pytest.mark.parametrize("shape", SHAPES)
def test_rays_only_first_frame(rt, refs, monkeypatch, shape):
    """SPT_COUNT_RAYS (parked colour, lock-step two-query loop): the frame,
    and the call and sample counters; counters[2] is not kept in this mode."""
    _env(monkeypatch, tune=shape)
    f = rt.SmallptFrame(W, H, mode=rt.SPT_PATH_TRACING | rt.SPT_COUNT_RAYS)
    f.render(SPP, counters=True)
    ref = refs(W, H, [SPP])
    spt_check.assert_same(f, ref, counted=False)
    c, r = f.counters, ref[3]
    assert (c[0], c[1], c[3]) == (r[0], r[1], r[3]), (c, r)


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_one_query_kernel(rt, refs, monkeypatch, shape, counted):
    """RT_SPT_DUAL=0 on Cornell: the one-query PARK kernels, first frame and
    continued."""
    _env(monkeypatch, tune=shape, dual="0")
    f = rt.SmallptFrame(W, H)
    f.render(SPP, counters=counted)
    spt_check.assert_same(f, refs(W, H, [SPP]), counted=counted)
    f.render(SPP, counters=counted)
    spt_check.assert_same(f, refs(W, H, [SPP, SPP]), counted=counted)


@pytest.mark.parametrize("geo", ["", "global"])
@pytest.mark.parametrize("shape", SHAPES)
def test_many_light_scene(rt, refs, monkeypatch, shape, geo):
    """A scene with three lights: the one-query kernels with the light-only
    pass_a(false) loop, whose parking area follows a 12 KB scene copy (or
    none).  Uncounted, then a counted launch of the same first frame."""
    _env(monkeypatch, tune=shape, geo=geo)
    (S, n), cam = _many_lights(W, H)
    ref = refs(W, H, [SPP], name="n255", make=lambda: _many_lights(W, H))
    f = rt.SmallptFrame(W, H, spheres=S, nspheres=n, camera=cam)
    f.render(SPP, counters=False)
    spt_check.assert_same(f, ref, counted=False)
    g = rt.SmallptFrame(W, H, spheres=S, nspheres=n, camera=cam)
    g.render(SPP, counters=True)
    spt_check.assert_same(g, ref, counted=True)
