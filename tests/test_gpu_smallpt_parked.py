"""GPU parity of the full-scan smallpt kernels' parked state: the running-
average colour lives in a lane-private LDS area and the camera terms in a
per-block one (smallpt.hip, PARK).  Small Cornell frames against the oracle,
bit for bit -- HDR colours, RGBA8 pixels, RNG state -- at the places the
parking can go wrong: lanes past the frame's edge, both block shapes (the LDS
area is carved per wave of a 4- or a 16-wave block), a row window,
progressive launches that start from a stored colour, and both iteration
forms (one and two ray queries per iteration)."""
import numpy as np
import pytest

import spt_check

pytestmark = pytest.mark.gpu

FRAMES = [(37, 21), (64, 40)]       # lanes past the right and the top edge; more than one tile group
SHAPES = ["wpb=4", "wpb=16"]        # small frames pick 16 on their own, the 1080p frame 4


@pytest.fixture(scope="module")
def refs(oracle):
    """Oracle frames, computed once per (w, h, passes) and handed out as
    read-only arrays: colours, seeds, pixels, counters."""
    return spt_check.frame_cache(oracle)


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("tune", SHAPES)
@pytest.mark.parametrize("w,h", FRAMES)
def test_ragged_tiles_both_block_shapes(rt, refs, monkeypatch, w, h, tune, counted):
    """Frames whose last tile column and row hang over the edge, 3 spp, in the
    4-wave and the 16-wave block shape; the uncounted kernel (the one the
    benchmark times) and the counted one."""
    monkeypatch.setenv("RT_SPT_TUNE", tune)
    f = rt.SmallptFrame(w, h)
    f.render(3, counters=counted)
    spt_check.assert_same(f, refs(w, h, [3]), counted=counted)


@pytest.mark.parametrize("tune", SHAPES)
def test_row_window_leaves_other_rows_untouched(rt, oracle, monkeypatch, tune):
    """64x40, rows [8, 29): the window's pixels equal the oracle's and every
    colour, pixel and seed slot outside it keeps the value it had."""
    monkeypatch.setenv("RT_SPT_TUNE", tune)
    w, h, r0, r1, spp = 64, 40, 8, 29, 3
    S, n, cam = rt.scenes.smallpt("cornell", w, h)
    col0 = np.full(3 * w * h, -7.25, np.float32)
    px0 = np.full(w * h, 0xA5A5A5A5, np.uint32)
    seeds0 = rt.scenes.seeds(w, h)
    # the oracle renders in place: slots outside the window keep col0 / px0 / the initial seeds
    rcol, rpx, rseeds = col0.copy(), px0.copy(), seeds0.copy()
    OS, on = oracle.cornell()
    oracle.smallpt_render(OS, on, oracle.cornell_camera(w, h), rcol, rseeds, rpx, w, h, 0, spp,
                          row_begin=r0, row_end=r1)
    # seeds_out is a buffer of its own: the window's slots (accumulator and
    # seed rows are flipped: slot (h - y - 1) * w + x) get the oracle's state
    sentinel = np.uint32(0xDEADBEEF)
    inside = np.zeros((h, w), bool)
    inside[h - r1:h - r0] = True
    want_seeds = np.where(np.repeat(inside.reshape(-1), 2), rseeds, sentinel)

    sc = rt.SmallptScene(S, n)
    f = rt.SmallptDeviceFrame(sc, cam, w, h).reset(colors=-7.25, pixels=0xA5A5A5A5, seeds=sentinel)
    f.render(spp, rows=(r0, r1))
    col, sout, px = f.host()
    assert (col.view(np.uint32) == rcol.view(np.uint32)).all()
    assert (px == rpx).all()
    assert (sout == want_seeds).all()
    sc.close()


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("tune", SHAPES)
def test_progressive_state_through_the_parked_colour(rt, refs, monkeypatch, tune, counted):
    """2 spp, then 3 more from the first launch's colours and seeds
    (first_sample = 2: the parked colour starts from the stored one): equal
    to one 5-spp launch and to the oracle's progressive result."""
    monkeypatch.setenv("RT_SPT_TUNE", tune)
    w, h = 37, 21
    a = rt.SmallptFrame(w, h)
    a.render(2, counters=counted)
    a.render(3, counters=counted)
    b = rt.SmallptFrame(w, h)
    b.render(5, counters=counted)
    assert (a.colors.view(np.uint32) == b.colors.view(np.uint32)).all()
    assert (a.pixels == b.pixels).all() and (a.seeds == b.seeds).all()
    spt_check.assert_same(a, refs(w, h, [2, 3]), counted=counted)
    spt_check.assert_same(b, refs(w, h, [5]), counted=counted)


@pytest.mark.parametrize("tune", SHAPES)
def test_single_sample_launches(rt, refs, monkeypatch, tune):
    """nsamples = 1: the first sample only writes the parked colour; then one
    more single-sample launch reads it back from the stored frame."""
    monkeypatch.setenv("RT_SPT_TUNE", tune)
    w, h = 37, 21
    f = rt.SmallptFrame(w, h)
    f.render(1, counters=False)
    spt_check.assert_same(f, refs(w, h, [1]), counted=False)
    f.render(1, counters=False)
    spt_check.assert_same(f, refs(w, h, [1, 1]), counted=False)


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("tune", SHAPES)
@pytest.mark.parametrize("dual", ["0", "1"])
def test_both_iteration_forms(rt, refs, monkeypatch, dual, tune, counted):
    """RT_SPT_DUAL=0 (one query per iteration) and =1 (two): both full-scan
    loops carry the parked state."""
    monkeypatch.setenv("RT_SPT_DUAL", dual)
    monkeypatch.setenv("RT_SPT_TUNE", tune)
    w, h = 37, 21
    f = rt.SmallptFrame(w, h)
    f.render(3, counters=counted)
    spt_check.assert_same(f, refs(w, h, [3]), counted=counted)
