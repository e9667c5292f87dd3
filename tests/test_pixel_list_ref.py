"""The pixel-list reference (tests/pixel_list_ref.py) against single ors_render
calls on a 24 x 16 Cornell frame, and the public surface the pixel lists add.
No GPU."""
import numpy as np
import pytest

import pixel_list_ref as plr

W, H, NMAX = 24, 16, 4


@pytest.fixture(scope="module", params=[0, 1], ids=["path", "direct"])
def snaps(request, oracle):
    S, n = oracle.cornell()
    cam = oracle.cornell_camera(W, H)
    return S, n, cam, request.param, plr.snapshots(S, n, cam, W, H, NMAX, request.param)


def _render(oracle, S, n, cam, dl, windows):
    """Fresh buffers, then one ors_render call per (row_begin, row_end, nsamples)."""
    col = np.zeros(3 * W * H, np.float32)
    seeds = oracle.seeds(W, H)
    px = np.zeros(W * H, np.uint32)
    for r0, r1, ns in windows:
        oracle.smallpt_render(S, n, cam, col, seeds, px, W, H, 0, ns, row_begin=r0, row_end=r1, dl=dl)
    return col, seeds, px


def test_snapshot_n_is_one_call_of_n_samples(oracle, snaps):
    S, n, cam, dl, sn = snaps
    assert sn["col"].shape == (NMAX + 1, 3 * W * H) and not sn["col"][0].any() and not sn["px"][0].any()
    assert (sn["seeds"][0] == oracle.seeds(W, H)).all()
    for k in range(1, NMAX + 1):
        col, seeds, px = _render(oracle, S, n, cam, dl, [(0, H, k)])
        assert (sn["col"][k].view(np.uint32) == col.view(np.uint32)).all(), k
        assert (sn["seeds"][k] == seeds).all() and (sn["px"][k] == px).all(), k
        assert sn["cnt"][k][3] == k * W * H
    assert (sn["seeds"][1] != sn["seeds"][2]).any() and sn["px"][NMAX].any()


def test_rows_with_different_counts_equal_expected(oracle, snaps):
    """Rows [0, 5) once, [5, 11) three times, [11, 14) not at all, [14, 16)
    four times, each window one ors_render call on the same buffers: every
    pixel is the snapshot of its own count -- pixels do not depend on each
    other in the oracle itself."""
    S, n, cam, dl, sn = snaps
    windows = [(0, 5, 1), (5, 11, 3), (14, 16, 4)]
    totals = np.zeros((H, W), np.int64)
    for r0, r1, ns in windows:
        totals[r0:r1] = ns
    col, seeds, px = _render(oracle, S, n, cam, dl, windows)
    ecol, eseeds, epx, edone = plr.expected(sn, totals)
    assert (ecol.view(np.uint32) == col.view(np.uint32)).all()
    assert (eseeds == seeds).all() and (epx == px).all()
    assert (edone.reshape(H, W)[::-1] == totals).all()
    # the rows a window skipped are the start's
    assert not epx.reshape(H, W)[11:14].any() and epx.reshape(H, W)[14:].any()


def test_expected_picks_single_pixels(snaps):
    """A scattered map: each pixel's colour, seeds and packed value come from
    the snapshot of its own total, at the slot and the index the frame uses."""
    sn = snaps[4]
    totals = np.random.default_rng(5).integers(0, NMAX + 1, (H, W))
    col, seeds, px, done = plr.expected(sn, totals)
    for (x, y) in [(0, 0), (W - 1, 0), (3, 7), (W - 1, H - 1), (11, 15)]:
        t, slot = totals[y, x], (H - y - 1) * W + x
        assert (col[3 * slot:3 * slot + 3].view(np.uint32) == sn["col"][t][3 * slot:3 * slot + 3].view(np.uint32)).all()
        assert (seeds[2 * slot:2 * slot + 2] == sn["seeds"][t][2 * slot:2 * slot + 2]).all()
        assert px[y * W + x] == sn["px"][t][y * W + x] and done[slot] == t


def test_the_pixel_list_surface_exists():
    import rtamd
    assert "spt_scene_render_pixels_async" in rtamd._lib.EXPORTS
    for name in ("render_pixels", "budget_list", "done"):
        assert hasattr(rtamd.SmallptDeviceFrame, name), name
