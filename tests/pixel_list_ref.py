"""What a pixel list must leave in the frame, from the oracle as it is.  A
plain helper module.

A pixel owns its RNG words and its accumulator, so "pixel p after n samples"
is pixel p of ors_render(first_sample=0, nsamples=n), whatever the other
pixels were given.  snapshots() renders the whole frame one sample at a time
from the seed fill and keeps every buffer after 0 .. nmax samples;
expected() then picks each pixel from the snapshot of its own total.

tests/test_pixel_list_ref.py pins both against single ors_render calls."""
import os

import numpy as np

import oracle_lib

THREADS = max(1, min(8, os.cpu_count() or 1))


def snapshots(S, n, cam, w, h, nmax, dl=0, seed=1):
    """The frame after 0 .. nmax samples of every pixel: a dict of "col"
    float32 [nmax + 1, 3 * w * h] and "seeds" uint32 [nmax + 1, 2 * w * h] in
    slot order (h - y - 1) * w + x, "px" uint32 [nmax + 1, w * h] at y * w + x,
    and "cnt" uint64 [nmax + 1, 4], the oracle's counters summed up to there
    (Intersect calls, IntersectP calls, sphere tests, samples).  Snapshot 0 is
    the start: zero colours and pixels, the seed fill."""
    col = np.zeros(3 * w * h, np.float32)
    seeds = oracle_lib.seeds(w, h, seed)
    px = np.zeros(w * h, np.uint32)
    out = {"col": [col.copy()], "seeds": [seeds.copy()], "px": [px.copy()], "cnt": [np.zeros(4, np.uint64)]}
    for k in range(nmax):
        cnt = oracle_lib.smallpt_render(S, n, cam, col, seeds, px, w, h, k, 1, dl=dl, nthreads=THREADS)
        out["col"].append(col.copy())
        out["seeds"].append(seeds.copy())
        out["px"].append(px.copy())
        out["cnt"].append(out["cnt"][-1] + np.array(cnt, np.uint64))
    out = {k: np.stack(v) for k, v in out.items()}
    out["w"], out["h"] = w, h
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def expected(snaps, totals):
    """(col, seeds, px, done) of a frame whose pixel (x, y) has had
    totals[y, x] samples since the start (an integer map [h, w], every entry
    <= nmax): each pixel from the snapshot of its own total.  done is int32
    [w * h] in slot order, the totals themselves."""
    w, h = snaps["w"], snaps["h"]
    totals = np.asarray(totals)
    assert totals.shape == (h, w) and totals.min() >= 0 and totals.max() < len(snaps["col"])
    by_px = totals.reshape(-1).astype(np.int64)                  # at y * w + x
    by_slot = totals[::-1].reshape(-1).astype(np.int64)         # at (h - y - 1) * w + x
    slot = np.arange(w * h)
    col = snaps["col"].reshape(len(snaps["col"]), w * h, 3)[by_slot, slot].reshape(-1)
    seeds = snaps["seeds"].reshape(len(snaps["seeds"]), w * h, 2)[by_slot, slot].reshape(-1)
    px = snaps["px"][by_px, slot]
    return col, seeds, px, by_slot.astype(np.int32)
