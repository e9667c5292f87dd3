"""CPU pins of what tests/test_gpu_whitted_trace.py compares rtw_trace with:
the per-ray reference (tests/native/whitted_trace_ref.c), fed
rtamd.scenes.whitted_camera_rays and folded by rtamd.scenes.whitted_pack,
reproduces the oracle's frames (orw_render / orw_render_ocl) and all four
counters -- so the per-ray contract (one sub-sample of Engine_Render along the
ray as given) is the frame's, and the two numpy helpers restate the camera and
the pack exactly."""
import numpy as np
import pytest

import lit_scenes
import oracle_lib as O
import rtamd
import whitted_trace_ref as R
from rtamd import scenes


def _frame_from_rays(P, n, w, h, r0, r1, ocl):
    rays = scenes.whitted_camera_rays(w, h, r0, r1, ocl=ocl)
    assert rays.shape == (r1 - r0, w, 4 if ocl else 9, 6) and rays.dtype == np.float32
    col, t, ids, cnt, stale = R.trace(P, n, rays, ocl)
    px = scenes.whitted_pack(col.reshape(rays.shape[:3] + (3,)), ocl=ocl)
    assert px.dtype == np.uint32 and px.shape == (r1 - r0, w)
    return px, cnt, stale, (col, t, ids)


@pytest.mark.parametrize("w,h", [(32, 48), (64, 48)])
@pytest.mark.parametrize("ocl", [False, True], ids=["cpu", "ocl"])
def test_reference_scene_frames_and_counters(w, h, ocl):
    P, n = O.whitted_scene()
    if ocl:
        ref, rcnt = O.whitted_render_ocl(w, h, nthreads=R.NT)
    else:
        ref, rcnt = O.whitted_render(w, h, 20, h, nthreads=R.NT)
    px, cnt, _, _ = _frame_from_rays(P, n, w, h, 20, h, ocl)
    assert (px == ref[20:h]).all(), "%d pixels differ" % (px != ref[20:h]).sum()
    assert cnt == rcnt
    assert len(np.unique(px)) > 50                          # (not an empty frame)


@pytest.mark.parametrize("seed", [lit_scenes.WALLED_DEEP_SEED, lit_scenes.WALLED_SEEDS[0]])
@pytest.mark.parametrize("ocl", [False, True], ids=["cpu", "ocl"])
def test_walled_scenes_frames_and_counters(seed, ocl):
    P, n, w, h, rays, out, (ref, rcnt) = R.walled_set(seed, ocl)
    r0, r1 = R.window_rows(w, h, ocl)
    lit_scenes.check_lit(ref, (r0, r1))
    px = scenes.whitted_pack(out[0].reshape(rays.shape[:3] + (3,)), ocl=ocl)
    assert (px == ref[r0:r1]).all(), "%d pixels differ" % (px != ref[r0:r1]).sum()
    assert out[3] == rcnt


def test_both_stale_ray_kinds_are_covered():
    """A TIR node's refraction child runs along the refr_Ray variable as the
    earlier calls left it.  Earlier node's ray: the reference scene's 64 x 48
    set (16,128 rays), all 9 TIR nodes.  Caller's own ray: the same scene with
    m_RIndex = 0.5, all 1,323 TIR nodes.  (Both measured on the oracle.)"""
    P, n, rays, (col, t, ids, cnt, stale) = R.camera_set("ref", False)
    assert rays.reshape(-1, 6).shape[0] == 16128
    assert cnt == [37287, 149076, 1941804, 9]
    assert stale == [9, 0]
    ref, rcnt = O.whitted_render(64, 48, 20, 48, nthreads=R.NT)
    assert cnt == rcnt
    P, n, rays, (col, t, ids, cnt, stale) = R.camera_set("low", False)
    assert stale == [0, 1323] and cnt[3] == 1323
    ref, rcnt = O.whitted_render(64, 48, 20, 48, nthreads=R.NT, prims=P, n=n)
    assert cnt == rcnt
    px = scenes.whitted_pack(col.reshape(rays.shape[:3] + (3,)))
    assert (px == ref[20:48]).all()


def test_per_ray_outputs():
    """t and id are the root call's: 1e6 and -1 on a miss, else the distance
    and primitive; a colour channel is never -0.0."""
    P, n, rays, (col, t, ids, cnt, stale) = R.camera_set("ref", False)
    assert ((ids >= 0) & (ids < n)).all() and (t < 1e6).all()          # the reference scene is closed
    away = np.array([[0, 50, 0, 0, 1, 0]], np.float32)                 # above the ceiling plane, pointing up
    c, t1, i1, _, _ = R.trace(P, n, away)
    assert i1[0] == -1 and t1[0] == np.float32(1e6) and (R.bits(c) == 0).all()
    assert not (R.bits(col) == 0x80000000).any()


def test_pack_conversion_edges():
    """(int) of a NaN or an out-of-range value is INT_MIN; the clamp is from
    above only; CPU adds the channels, OpenCL ORs them."""
    f = np.float32
    c = np.zeros((5, 1, 3), f)
    c[0, 0] = (1.0, 0.5, 0.25)                 # 28 14 7 / 64 32 16
    c[1, 0] = (100.0, np.nan, 0.0)             # 255, INT_MIN, 0
    c[2, 0] = (-1.0, 0.0, 0.0)                 # -28 / -64
    c[3, 0] = (np.inf, -np.inf, 1e30)          # INT_MIN x 3
    c[4, 0] = (0.0, 0.0, -0.26)                # (int) truncates toward zero: -7 / -16
    M = 1 << 32
    lo = -(1 << 31)
    want_cpu = [(28 << 16) + (14 << 8) + 7, ((255 << 16) + ((lo << 8) % M)) % M, ((-28 << 16) % M),
                (((lo << 16) % M) + ((lo << 8) % M) + (lo % M)) % M, (-7) % M]
    want_ocl = [(64 << 16) | (32 << 8) | 16, (255 << 16) | ((lo << 8) % M), ((-64 << 16) % M),
                ((lo << 16) % M) | ((lo << 8) % M) | (lo % M), (-16) % M]
    assert [int(v) for v in scenes.whitted_pack(c)] == want_cpu
    assert [int(v) for v in scenes.whitted_pack(c, ocl=True)] == want_ocl
    # the ordered sum: (a + b) + c in float32, from 0
    s = np.array([[[1e8, 0, 0], [1.0, 0, 0], [-1e8, 0, 0]]], f)
    assert int(scenes.whitted_pack(s)[0]) == 0
    assert int(scenes.whitted_pack(s[:, ::-1])[0]) == 0 and int(scenes.whitted_pack(s[:, [0, 2, 1]])[0]) == 28 << 16


def test_camera_rays_rows_and_defaults():
    full = scenes.whitted_camera_rays(40, 120)                       # rows [20, 50)
    assert full.shape == (30, 40, 9, 6)
    part = scenes.whitted_camera_rays(40, 120, 31, 44)               # m_SY's recurrence still starts at row 20
    assert (R.bits(part) == R.bits(full[11:24])).all()
    assert scenes.whitted_camera_rays(40, 120, ocl=True).shape == (100, 40, 4, 6)
    with pytest.raises(ValueError):
        scenes.whitted_camera_rays(40, 120, 19, 30)


def test_python_surface():
    assert rtamd.RTW_TRACE_OCL == 0x1
    assert callable(rtamd.whitted_trace) and callable(rtamd.whitted_trace_async)
