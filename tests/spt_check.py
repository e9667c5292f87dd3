"""Shared plumbing of the smallpt GPU tests: the oracle's reference frame, a
per-module cache of such frames, and the one bit-exact comparison.

TEST INFRASTRUCTURE ONLY (imported like oracle_lib and scenes_layouts)."""
import json
import os

import numpy as np


def golden(key):
    """tests/golden/known_answers.json's smallpt entry `key`: hashes of the reference core's frame."""
    with open(os.path.join(os.path.dirname(__file__), "golden", "known_answers.json")) as f:
        return json.load(f)["smallpt"][key]


def oracle_frame(oracle, w, h, steps, mode=0, scene=None, cam=None, rows=None, nthreads=8):
    """The oracle's frame after the progressive passes `steps` (a list of pass
    sizes) from the initial state: read-only (colors float32, seeds uint32,
    pixels uint32, counters).  scene: (spheres, n), default Cornell; cam:
    default Cornell's at w x h; rows=(r0, r1): a row window of a zero frame
    (slots outside it keep 0 / the initial seeds)."""
    S, n = oracle.cornell() if scene is None else scene
    cam = oracle.cornell_camera(w, h) if cam is None else cam
    r0, r1 = rows or (0, h)
    col = np.zeros(3 * w * h, np.float32)
    seeds = oracle.seeds(w, h)
    px = np.zeros(w * h, np.uint32)
    cnt = [0, 0, 0, 0]
    first = 0
    for k in steps:
        c = oracle.smallpt_render(S, n, cam, col, seeds, px, w, h, first, k, row_begin=r0, row_end=r1, dl=mode,
                                  nthreads=nthreads)
        cnt = [a + b for a, b in zip(cnt, c)]
        first += k
    for a in (col, seeds, px):
        a.setflags(write=False)
    return col, seeds, px, tuple(cnt)


def frame_cache(oracle):
    """get(w, h, steps, mode=0, rows=None, name="cornell", make=None):
    oracle_frame, computed once per key.  A scene other than Cornell goes by
    a `name` of the caller's (part of the key) and `make`, called on a miss
    only, which returns ((spheres, n), camera)."""
    cache = {}

    def get(w, h, steps, mode=0, rows=None, name="cornell", make=None):
        key = (name, w, h, tuple(steps), mode, rows)
        if key not in cache:
            scene, cam = make() if make else (None, None)
            cache[key] = oracle_frame(oracle, w, h, steps, mode, scene, cam, rows)
        return cache[key]

    return get


def _fields(x):
    """(colors, seeds, pixels, counters or None) of a frame object or tuple."""
    if isinstance(x, tuple):
        col, seeds, px = x[:3]
        cnt = x[3] if len(x) > 3 else None
    elif hasattr(x, "host"):                       # SmallptDeviceFrame
        (col, seeds, px), cnt = x.host(), x.counters.tolist()
    else:                                          # SmallptFrame
        col, seeds, px, cnt = x.colors, x.seeds, x.pixels, x.counters
    return col, seeds, px, None if cnt is None else [int(v) for v in cnt]


def assert_same(got, ref, counted=None):
    """got == ref bit for bit.  Each is a SmallptFrame, a SmallptDeviceFrame
    or a (colors, seeds, pixels[, counters]) tuple.  Colours are compared as
    uint32 patterns (so an equal NaN passes and +0.0 against -0.0 fails),
    then seeds and pixels, then the counters where both sides have them --
    unless counted is False (an uncounted launch's frame); counted=True also
    fails where a side has none."""
    gcol, gseeds, gpx, gcnt = _fields(got)
    rcol, rseeds, rpx, rcnt = _fields(ref)
    assert gcol.shape == rcol.shape and gseeds.shape == rseeds.shape and gpx.shape == rpx.shape
    diff = gcol.view(np.uint32) != rcol.view(np.uint32)
    if diff.any():
        with np.errstate(invalid="ignore"):
            d = np.abs(gcol.astype(np.float64) - rcol.astype(np.float64))[diff]
        d = d[~np.isnan(d)]
        raise AssertionError("HDR not bit-exact (%d slots, max |d| %g)" % (diff.sum(), d.max() if d.size else np.nan))
    bad = gseeds.view(np.uint32) != rseeds.view(np.uint32)
    assert not bad.any(), "seeds differ (%d words)" % bad.sum()
    bad = gpx.view(np.uint32) != rpx.view(np.uint32)
    assert not bad.any(), "pixels differ (%d)" % bad.sum()
    if counted:
        assert gcnt is not None and rcnt is not None, "counted=True needs counters on both sides"
    if counted is not False and gcnt is not None and rcnt is not None:
        assert gcnt == rcnt, "counters differ: %s != %s" % (gcnt, rcnt)
