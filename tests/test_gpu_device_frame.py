"""rtamd.SmallptDeviceFrame: every way it launches (row window, interleaved
share, group list, progressive, under graph capture) gives the bits of
rtamd.SmallptFrame's blocking whole-frame render, which the other GPU tests pin
to the oracle.  Cornell at 36x20, 2 spp: the smallest frame with lanes past
both edges and more than one tile group."""
import numpy as np
import pytest

from spt_check import assert_same

pytestmark = pytest.mark.gpu

W, H, SPP = 36, 20, 2


@pytest.fixture(scope="module")
def whole(rt):
    """SmallptFrame's counted whole-frame render, as read-only arrays."""
    f = rt.SmallptFrame(W, H).render(SPP, counters=True)
    for a in (f.colors, f.seeds, f.pixels):
        a.setflags(write=False)
    return f.colors, f.seeds, f.pixels, tuple(f.counters)


@pytest.fixture
def frame(rt):
    S, n, cam = rt.scenes.smallpt("cornell", W, H)
    sc = rt.SmallptScene(S, n)
    yield rt.SmallptDeviceFrame(sc, cam, W, H)
    sc.close()


def test_whole_frame_counted(frame, whole):
    assert frame.groups_total > 1
    assert frame.render(SPP, counted=True) == 0
    assert_same(frame, whole, counted=True)


def test_row_window_into_sentinels(frame, whole):
    r0, r1 = 8, 16
    frame.reset(colors=-7.25, pixels=0xA5A5A5A5, seeds=0xDEADBEEF)
    frame.render(SPP, rows=(r0, r1))
    col, seeds, px = frame.host()
    inside = np.zeros((H, W), bool)
    inside[H - r1:H - r0] = True                       # accumulator and seed rows are flipped
    ins = inside.reshape(-1)
    assert (col.reshape(-1, 3)[ins].view(np.uint32) == whole[0].reshape(-1, 3)[ins].view(np.uint32)).all()
    assert (col.reshape(-1, 3)[~ins] == np.float32(-7.25)).all()
    assert (seeds.reshape(-1, 2)[ins] == whole[1].reshape(-1, 2)[ins]).all()
    assert (seeds.reshape(-1, 2)[~ins] == 0xDEADBEEF).all()
    px, ref = px.reshape(H, W), whole[2].reshape(H, W)
    assert (px[r0:r1] == ref[r0:r1]).all()
    assert (np.delete(px, np.s_[r0:r1], 0) == 0xA5A5A5A5).all()


def test_two_shares_make_the_frame(frame, whole):
    frame.render(SPP, counted=True, share=(0, 2))
    frame.render(SPP, counted=True, share=(1, 2))
    assert_same(frame, whole, counted=True)


def test_all_groups_as_a_list(frame, whole):
    import torch
    groups = torch.arange(frame.groups_total, dtype=torch.int32, device=frame.device)
    frame.render(SPP, counted=True, groups=groups)
    assert_same(frame, whole, counted=True)


def test_progressive_launches(rt, frame):
    frame.render(2, counted=True)
    frame.render(2, first_sample=2, counted=True, seeds_in=frame.seeds)
    assert_same(frame, rt.SmallptFrame(W, H).render(4, counters=True), counted=True)


def test_bad_mode_code_and_exception(rt, frame):
    assert frame.render(1, mode=0x400, check=False) == rt._lib.RT_ERR_INVALID
    with pytest.raises(rt.RTError):
        frame.render(1, mode=0x400)
    with pytest.raises(ValueError):
        frame.render(1, rows=(0, H), share=(0, 2))


def test_missing_entry_point_is_an_rterror(rt):
    """What share=, groups= and cost= raise on an older library without
    their entry points."""
    with pytest.raises(rt.RTError, match="not exported"):
        rt._lib.entry("spt_scene_render_no_such_async")


def test_graph_capture_replays_the_same_bits(frame, whole):
    """render under capture (torch.cuda.graph's side stream): it reads the
    current stream at the time of the call, allocates nothing and never
    synchronises."""
    import torch
    frame.render(SPP)                                  # (an uncaptured launch first, as the other graph tests do)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="relaxed"):
        frame.render(SPP)
    torch.cuda.synchronize()
    frame.reset(colors=-1.0, pixels=1, seeds=1)
    g.replay()
    assert_same(frame, whole, counted=False)
