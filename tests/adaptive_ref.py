"""What the second-moment plane and the sample plan must hold, restated in
numpy float32 from the oracle as it is.  A plain helper module.

The oracle keeps a running mean and shows no sample on its own.  Sample k's
radiance of every pixel is one ors_render call (first_sample=0, nsamples=1)
into zeroed colours from a copy of the seeds after k samples: the fold of
sample number 0 stores the radiance itself.  Folding those radiances with
(c * k1 + R) * k2, k2 = 1 / (k1 + 1), gives the oracle's colours back bit for
bit (tests/test_adaptive_ref.py pins that), so the same fold of
q = (R.x * R.x + R.y * R.y) + R.z * R.z is the m2 the STATS kernels must write.

plan() restates spt_frame_plan_async (include/rt_hip.h)."""
import numpy as np

import oracle_lib
import pixel_list_ref as plr

F = np.float32


def fold(m, q, k):
    """One fold of sample number k into the running mean m (float32 arrays)."""
    if k == 0:
        return q.copy()
    k1 = F(k)
    k2 = F(1) / (k1 + F(1))
    return (m * k1 + q) * k2


def radiances(S, n, cam, w, h, snaps, dl=0):
    """float32 [nmax, 3 * w * h] in slot order: sample k's radiance of every
    pixel, and uint32 [nmax, 2 * w * h]: the seeds that render left (they must
    be snaps["seeds"][k + 1])."""
    rad, after = [], []
    for k in range(len(snaps["col"]) - 1):
        col = np.zeros(3 * w * h, np.float32)
        seeds = snaps["seeds"][k].copy()
        px = np.zeros(w * h, np.uint32)
        oracle_lib.smallpt_render(S, n, cam, col, seeds, px, w, h, 0, 1, dl=dl, nthreads=plr.THREADS)
        rad.append(col)
        after.append(seeds)
    return np.stack(rad), np.stack(after)


def snapshots(S, n, cam, w, h, nmax, dl=0, seed=1):
    """pixel_list_ref.snapshots plus "rad" float32 [nmax, 3 * w * h], the
    samples' radiances, and "m2" float32 [nmax + 1, w * h] in slot order: the
    running mean of |R|^2 after 0 .. nmax samples (snapshot 0: zeros)."""
    snaps = dict(plr.snapshots(S, n, cam, w, h, nmax, dl, seed))
    rad, after = radiances(S, n, cam, w, h, snaps, dl)
    assert (after == snaps["seeds"][1:]).all()
    m2 = [np.zeros(w * h, np.float32)]
    for k in range(nmax):
        r = rad[k].reshape(-1, 3)
        q = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        m2.append(fold(m2[-1], q, k))
    snaps["rad"], snaps["m2"] = rad, np.stack(m2)
    for v in (snaps["rad"], snaps["m2"]):
        v.setflags(write=False)
    return snaps


def expected_m2(snaps, totals):
    """m2 of a frame whose pixel (x, y) has had totals[y, x] samples, float32
    [w * h] in slot order."""
    by_slot = np.asarray(totals)[::-1].reshape(-1).astype(np.int64)
    return snaps["m2"][by_slot, np.arange(len(by_slot))]


def tile_key(x, y, w):
    """budget_list(order="tile")'s sort key."""
    return ((y >> 3) * ((w + 7) // 8) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)


def plan(col, m2, done, w, h, params, cap):
    """spt_frame_plan_async in numpy: (list int32 [cap], take int32 [cap],
    error float32 [w * h] at the slot, totals (listed, sum of takes)).  params
    = (min_samples, max_samples, step, tol, floor); col float32 [3 * w * h],
    m2 float32 and done int32 [w * h], all in slot order."""
    mn, mx, step, tol, floor = params
    c = np.asarray(col, np.float32).reshape(-1, 3)
    m2 = np.asarray(m2, np.float32)
    n = np.asarray(done).astype(np.int64)
    with np.errstate(all="ignore"):
        mean2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        var = m2 - mean2
        var = np.where(var > 0, var, F(0)).astype(np.float32)
        e = np.sqrt(var / (n.astype(np.float32) * (mean2 + F(floor)))).astype(np.float32)
        low = n < mn
        e = np.where(low, F(np.inf), e).astype(np.float32)
        more = (e > F(tol)) & (n < mx)
    take = np.where(low, mn - n, np.where(more, np.minimum(step, mx - n), 0))
    slot = np.arange(w * h)
    x, y = slot % w, h - 1 - slot // w
    listed = np.flatnonzero(take > 0)
    listed = listed[np.argsort(tile_key(x[listed], y[listed], w), kind="stable")]
    pix, tk = (y * w + x)[listed], take[listed]
    lst, tko = np.full(cap, -1, np.int32), np.zeros(cap, np.int32)
    k = min(cap, len(pix))
    lst[:k], tko[:k] = pix[:k], tk[:k]
    return lst, tko, e, (len(pix), int(tk.sum()))


def same_floats(a, b):
    """Equal as bit patterns, a NaN equal to any NaN (the expressions do not
    fix a NaN's sign or payload; x86 and gfx950 produce different ones)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def refine(snaps, passes, params):
    """frame.refine(passes, ...) simulated on the snapshots from the start
    state: the totals map [h, w] afterwards and, per pass, the plan's (listed,
    sum of takes)."""
    w, h = snaps["w"], snaps["h"]
    totals = np.zeros((h, w), np.int64)
    log = []
    for _ in range(passes):
        col, _, _, done = plr.expected(snaps, totals)
        lst, tk, _, tot = plan(col, expected_m2(snaps, totals), done, w, h, params, w * h)
        ok = lst >= 0
        np.add.at(totals.reshape(-1), lst[ok], tk[ok])
        log.append(tot)
    return totals, log
