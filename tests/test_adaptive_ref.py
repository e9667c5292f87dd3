"""The adaptive-sampling reference (tests/adaptive_ref.py) against the oracle
on a 37 x 19 Cornell frame, eight samples, both modes: a sample's radiance
from a single-sample render, the colour fold restated in numpy float32, the m2
snapshots built with it, the numpy plan's properties, and the public surface
the feature adds.  No GPU."""
import numpy as np
import pytest

import adaptive_ref as ar
import pixel_list_ref as plr

W, H, NMAX = 37, 19, 8
PARAMS = (2, 8, 2, 0.4, 1e-3)                   # min, max, step, tol, floor: the closed loop of the GPU test


@pytest.fixture(scope="module", params=[0, 1], ids=["path", "direct"])
def snaps(request, oracle):
    S, n = oracle.cornell()
    return ar.snapshots(S, n, oracle.cornell_camera(W, H), W, H, NMAX, request.param)


def test_single_sample_renders_fold_into_the_oracles_colours(snaps):
    """The seeds advance as in the progressive frame (asserted inside
    ar.snapshots too), and (c * k1 + R) * k2 with k2 = 1 / (k1 + 1) over the
    single-sample radiances is the oracle's colour after every sample, bit
    for bit."""
    col = np.zeros(3 * W * H, np.float32)
    for k in range(NMAX):
        col = ar.fold(col, snaps["rad"][k], k)
        assert (col.view(np.uint32) == snaps["col"][k + 1].view(np.uint32)).all(), k
    assert snaps["rad"].any() and np.isfinite(snaps["rad"]).all()


def test_m2_snapshots_are_the_mean_of_squared_radiance(snaps):
    rad = snaps["rad"].reshape(NMAX, -1, 3).astype(np.float64)
    q = (rad ** 2).sum(axis=2)
    assert not snaps["m2"][0].any()
    r0 = snaps["rad"][0].reshape(-1, 3)
    q0 = (r0[:, 0] * r0[:, 0] + r0[:, 1] * r0[:, 1]) + r0[:, 2] * r0[:, 2]
    assert (snaps["m2"][1].view(np.uint32) == q0.view(np.uint32)).all()         # sample 0 stores q itself
    for k in range(1, NMAX + 1):
        want = q[:k].mean(axis=0)
        assert np.allclose(snaps["m2"][k], want, rtol=1e-5, atol=1e-30), k
        # the variance the plan takes from the planes is the samples' own (up to float cancellation)
        c = snaps["col"][k].reshape(-1, 3).astype(np.float64)
        var = snaps["m2"][k] - (c ** 2).sum(axis=1)
        assert np.allclose(var, rad[:k].var(axis=0).sum(axis=1), rtol=1e-3, atol=2e-6 * (want + 1)), k
    totals = np.random.default_rng(2).integers(0, NMAX + 1, (H, W))
    m2 = ar.expected_m2(snaps, totals)
    for (x, y) in [(0, 0), (W - 1, 0), (5, 11), (W - 1, H - 1)]:
        slot = (H - y - 1) * W + x
        assert m2[slot].view(np.uint32) == snaps["m2"][totals[y, x]][slot].view(np.uint32)


def _tile_order(w, h):
    y, x = np.mgrid[0:h, 0:w]
    p = (y * w + x).reshape(-1)
    return p[np.argsort(ar.tile_key(x.reshape(-1), y.reshape(-1), w), kind="stable")]


def test_plan_from_nothing_lists_every_pixel_in_tile_order(snaps):
    mn = PARAMS[0]
    lst, take, err, tot = ar.plan(snaps["col"][0], snaps["m2"][0], np.zeros(W * H, np.int32), W, H, PARAMS, W * H)
    assert (lst == _tile_order(W, H)).all() and (take == mn).all()
    assert np.isposinf(err).all() and tot == (W * H, mn * W * H)
    assert (lst[:8] == np.arange(8)).all() and lst[8] == W and lst[64] == 8      # a tile's rows, then the next tile


def test_plan_properties_on_an_uneven_frame(snaps):
    """Random totals in [0, max]: the list is a set in ascending key order,
    done + take <= max, below min the take is min - done, a converged or
    finished pixel is not listed; truncation keeps the first cap entries and
    the totals; the padding is -1 / 0."""
    mn, mx, step, tol, _ = PARAMS
    totals = np.random.default_rng(3).integers(0, NMAX + 1, (H, W))
    col, _, _, done = plr.expected(snaps, totals)
    m2 = ar.expected_m2(snaps, totals)
    lst, take, err, tot = ar.plan(col, m2, done, W, H, PARAMS, W * H)
    nl = tot[0]
    assert 0 < nl < W * H and (lst[nl:] == -1).all() and (take[nl:] == 0).all() and (lst[:nl] >= 0).all()
    p, t = lst[:nl], take[:nl]
    assert len(set(p)) == nl and tot[1] == t.sum() and (t > 0).all()
    assert (np.diff(ar.tile_key(p % W, p // W, W)) > 0).all()
    slot = (H - 1 - p // W) * W + p % W
    assert (done[slot] + t <= mx).all()
    low = done[slot] < mn
    assert low.any() and (t[low] == mn - done[slot][low]).all() and (t[~low] == np.minimum(step, mx - done[slot][~low])).all()
    assert (err[slot][~low] > tol).all() and np.isposinf(err[done < mn]).all()
    unlisted = np.ones(W * H, bool)
    unlisted[slot] = False
    assert ((done[unlisted] >= mx) | (err[unlisted] <= tol)).all() and (done[unlisted] >= mn).all()
    assert ((done >= mx) & (err > tol)).any() and ((done >= mn) & (done < mx) & (err <= tol)).any()
    for cap in (0, 1, nl - 1, nl, nl + 3):
        l2, t2, e2, tot2 = ar.plan(col, m2, done, W, H, PARAMS, cap)
        k = min(cap, nl)
        assert len(l2) == len(t2) == cap and (l2[:k] == p[:k]).all() and (t2[:k] == t[:k]).all()
        assert (l2[k:] == -1).all() and (t2[k:] == 0).all() and tot2 == tot and ar.same_floats(e2, err).all()


def test_plan_edge_values():
    """tol = 0 lists every pixel with any spread; tol = inf none past the
    bootstrap; zero colours over a zero floor and NaN planes are not listed;
    an infinite m2 is."""
    inf, nan = np.inf, np.nan
    col = np.array([[1, 1, 1], [1, 1, 1], [0, 0, 0], [nan, 0, 0], [1, 0, 0], [inf, 0, 0], [1, 1, 1]], np.float32)
    m2 = np.array([3.5, 3, 0, 1, inf, 1, nan], np.float32)
    done = np.full(7, 4, np.int32)
    lst, take, err, tot = ar.plan(col.reshape(-1), m2, done, 7, 1, (2, 8, 3, 0.0, 0.0), 7)
    assert (lst == [0, 4, -1, -1, -1, -1, -1]).all() and (take[:2] == 3).all() and tot == (2, 6)
    assert err[0] > 0 and err[1] == 0 and np.isnan(err[2]) and np.isnan(err[3]) and np.isposinf(err[4])
    assert err[5] == 0 and err[6] == 0
    lst, take, err, tot = ar.plan(col.reshape(-1), m2, done, 7, 1, (2, 8, 3, inf, 0.0), 7)
    assert (lst == -1).all() and tot == (0, 0)
    lst, take, _, tot = ar.plan(col.reshape(-1), m2, np.full(7, 7, np.int32), 7, 1, (2, 8, 3, 0.0, 0.0), 7)
    assert (take[:2] == 1).all() and tot == (2, 2)                              # step larger than max - n
    lst, take, _, tot = ar.plan(col.reshape(-1), m2, np.arange(7, dtype=np.int32), 7, 1, (5, 5, 3, 0.0, 0.0), 7)
    assert (take == [5, 4, 3, 2, 1, 0, 0]).all() and tot == (5, 15)              # max == min: the bootstrap only


def test_the_closed_loop_condition_holds_on_the_reference(snaps):
    """The GPU test's loop, simulated: after the bootstrap the passes list
    between 10 % and 90 % of the pixels until the last lists none, and every
    total of 2, 4, 6, 8 occurs."""
    totals, log = ar.refine(snaps, 5, PARAMS)
    shares = [l[0] / (W * H) for l in log]
    assert shares[0] == 1.0 and shares[-1] == 0.0 and all(0.1 < s < 0.9 for s in shares[1:-1]), shares
    assert sorted(np.unique(totals)) == [2, 4, 6, 8] and min((totals == t).sum() for t in (2, 4, 6, 8)) >= 24


def test_the_adaptive_surface_exists():
    import rtamd
    for name in ("spt_scene_render_pixels_stats_async", "spt_frame_plan_scratch_bytes", "spt_frame_plan_async"):
        assert name in rtamd._lib.EXPORTS, name
    for name in ("m2", "plan", "refine", "plan_totals", "error"):
        assert hasattr(rtamd.SmallptDeviceFrame, name), name
    import ctypes as C
    assert C.sizeof(rtamd._lib.PlanParams) == 20
