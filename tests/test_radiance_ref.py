"""The per-ray radiance reference (tests/radiance_ref.py) against the oracle's
whole frames, and the host helpers the radiance queries added
(rtamd.scenes.mwc_draw, camera_rays' jitter).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import radiance_ref as rr

W, H, SPP = 8, 6, 3


def _slots(w, h):
    """Pixel (x, y) of every colour / seed slot i = (h - y - 1) * w + x."""
    i = np.arange(w * h)
    return i % w, h - 1 - i // w


@pytest.mark.parametrize("dl", [0, 1], ids=["path", "direct"])
def test_per_ray_calls_reproduce_the_frame(oracle, dl):
    """Cornell 8 x 6, 3 samples: one 1 x 1 ors_render call per ray and sample,
    the jitter drawn in numpy, gives the whole-frame ors_render's colours and
    seeds bit for bit; and the rays handed to the device are camera_rays'."""
    import rtamd
    S, n = oracle.cornell()
    cam = oracle.cornell_camera(W, H)
    col = np.zeros(3 * W * H, np.float32)
    seeds = oracle.seeds(W, H)
    seeds0 = seeds.copy()
    px = np.zeros(W * H, np.uint32)
    whole = oracle.smallpt_render(S, n, cam, col, seeds, px, W, H, 0, SPP, dl=dl)
    x, y = _slots(W, H)
    c = np.zeros((W * H, 3), np.float32)
    s = seeds0.reshape(-1, 2).copy()
    total = np.zeros(4, np.uint64)
    for k in range(SPP):
        _, r1, r2 = rr.after_jitter(s)
        D, O = rr.camera_pairs(cam, W, H, r1, r2, x, y)
        rays = rr.launch_rays(D, O)
        want = rtamd.scenes.camera_rays(cam, W, H, x, y, r1, r2)
        assert (rays.view(np.uint32) == want.view(np.uint32)).all()
        c, s, cnt = rr.oracle_sample(S, n, D, O, s, c, k, dl)
        assert (cnt[:, 0] >= 1).all() and (cnt[:, 3] == 1).all()
        total += cnt.sum(axis=0)
    assert (c.reshape(-1).view(np.uint32) == col.view(np.uint32)).all()
    assert (s.reshape(-1) == seeds).all()
    assert list(total) == whole and whole[0] > 3 * W * H and (dl or whole[1] > 0)


def test_camera_rays_with_zero_jitter_is_the_pixel_centre():
    import rtamd
    cam = rtamd.scenes.cornell_camera(16, 12)
    z = np.zeros(16 * 12, np.float32)
    a = rtamd.scenes.camera_rays(cam, 16, 12)
    b = rtamd.scenes.camera_rays(cam, 16, 12, r1=z, r2=z)
    assert a.dtype == b.dtype == np.float32 and (a.view(np.uint32) == b.view(np.uint32)).all()
    x, y = np.array([3, 15, 0]), np.array([0, 11, 5])
    c = rtamd.scenes.camera_rays(cam, 16, 12, x, y, r1=z[:3], r2=z[:3])
    assert (c.view(np.uint32) == a[y * 16 + x].view(np.uint32)).all()
    # a jitter moves the ray
    d = rtamd.scenes.camera_rays(cam, 16, 12, r1=z + np.float32(0.25), r2=z)
    assert (d[:, 3:] != a[:, 3:]).any(axis=1).all()


def test_mwc_draw_is_get_random(oracle):
    import rtamd
    L = oracle.lib()
    rng = np.random.default_rng(5)
    s = rng.integers(0, 2 ** 32, (2000, 2), dtype=np.uint64).astype(np.uint32)
    s[:8] = [[0, 0], [1, 1], [2, 2], [0xffffffff, 0xffffffff], [65535, 65536], [0x80000000, 1], [2, 0xffff0000],
             [12345, 67890]]
    before = s.copy()
    v, s0, s1 = rtamd.scenes.mwc_draw(s[:, 0], s[:, 1])
    assert (s == before).all()                                  # the inputs are untouched
    assert v.dtype == np.float32 and s0.dtype == s1.dtype == np.uint32
    for k in range(len(s)):
        a, b = C.c_uint32(int(s[k, 0])), C.c_uint32(int(s[k, 1]))
        want = np.float32(L.ors_get_random(C.byref(a), C.byref(b)))
        assert (a.value, b.value) == (int(s0[k]), int(s1[k]))
        assert want.view(np.uint32) == v[k].view(np.uint32)
