"""CPU checks around the ray queries (spt_scene_query_async): the numpy
restatement the GPU tests compare with (tests/ray_query_ref.py) equals the
C++ full scan of tests/native/spt_bvh_check.cpp; non-finite rays miss under
it (the kernel's up-front rule); camera_rays; the header; argument errors
that need no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ray_query_ref as rq
import scenes_layouts as sl

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NATIVE = os.path.join(HERE, "native")


@pytest.fixture(scope="module")
def chk():
    subprocess.run(["make", "-s", "-C", NATIVE, "libspt_bvh_check.so"], check=True)
    L = C.CDLL(os.path.join(NATIVE, "libspt_bvh_check.so"))
    P = C.c_void_p
    L.spt_bvh_wide_check.restype = C.c_longlong
    L.spt_bvh_wide_check.argtypes = [P, C.c_int, P, P, C.c_longlong, P, P, P, P, P]
    return L


def test_restatement_equals_the_native_full_scan(chk):
    """cloud(3000), 2,000 mixed rays: nearest (bound 1e20f) and highest
    occluder (the set's tmax) equal spt_bvh_wide_check's t_scan / id_scan."""
    S, n = sl.cloud(sl.N_LEAF8)
    rays, tmax = rq.ray_set(S, n, sl.cloud_camera, 2000)
    nr = len(rays)
    tw, ts = np.zeros(nr, np.float32), np.zeros(nr, np.float32)
    iw, is_ = np.zeros(nr, np.int32), np.zeros(nr, np.int32)
    chk.spt_bvh_wide_check(C.addressof(S), n, rays.ctypes.data, None, nr, tw.ctypes.data, iw.ctypes.data,
                           ts.ctypes.data, is_.ctypes.data, None)
    t, ids = rq.scan(S, n, rays)["nearest"]
    assert (ids == is_).all(), np.flatnonzero(ids != is_)[:10]
    assert (t.view(np.uint32) == ts.view(np.uint32)).all()
    assert (ids >= 4).sum() > 200 and (ids < 0).sum() > 200
    chk.spt_bvh_wide_check(C.addressof(S), n, rays.ctypes.data, tmax.ctypes.data, nr, tw.ctypes.data, iw.ctypes.data,
                           ts.ctypes.data, is_.ctypes.data, None)
    ref = rq.scan(S, n, rays, tmax)
    assert (ref["occluder"] == is_).all(), np.flatnonzero(ref["occluder"] != is_)[:10]
    assert ((ref["any"] == 1) == (is_ >= 0)).all()
    assert (is_ >= 0).sum() > 200 and (is_ < 0).sum() > 200


def test_bound_semantics_of_the_restatement():
    """d < bound strictly; a miss returns the bound's bits (NaN payload too);
    ties go to the highest index."""
    S, n = sl.coincident()
    o = np.array([[1.0, 0.0, 5.0]], np.float32)
    ray = np.concatenate([o, [[0.0, 0.0, -1.0]]], axis=1).astype(np.float32)
    t, i = rq.scan(S, n, ray)["nearest"]
    assert i[0] == sl.COINCIDENT_DUPES[-1] and t[0] == np.float32(4.0)
    for b, hit in ((t[0], False), (np.nextafter(t[0], np.float32(9)), True)):
        tt, ii = rq.scan(S, n, ray, np.array([b], np.float32))["nearest"]
        assert (ii[0] >= 0) == hit and (hit or tt.view(np.uint32)[0] == np.float32(b).view(np.uint32))
    nan = np.array([0x7fc12345], np.uint32).view(np.float32)
    tt, ii = rq.scan(S, n, ray, nan)["nearest"]
    assert ii[0] == -1 and tt.view(np.uint32)[0] == 0x7fc12345


def test_non_finite_rays_miss_under_the_restatement():
    """20,000 rays with one to three non-finite components over a 400-sphere
    cloud: no sphere is accepted at the bounds 1e20, 3e38 and +inf -- what the
    kernel's up-front classification returns without walking."""
    S, n = sl.cloud(400)
    rays = rq.non_finite_rays(S, n, 20000)
    for bound in (1e20, 3e38, np.inf):
        ref = rq.scan(S, n, rays, np.full(len(rays), bound, np.float32))
        assert (ref["nearest"][1] == -1).all() and (ref["occluder"] == -1).all() and (ref["any"] == 0).all()
        assert (ref["nearest"][0] == np.float32(bound)).all()


def test_camera_rays_cornell_centre_pixel():
    """The centre pixel of the Cornell view first hits the back wall (sphere
    2, whose surface is the plane z = 0 there) about 205.6 away; rows are
    numbered as pixels are; selected pixels equal the full grid's rows."""
    import rtamd
    S, n = rtamd.scenes.cornell()
    w, h = 64, 48
    cam = rtamd.scenes.cornell_camera(w, h)
    rays = rtamd.scenes.camera_rays(cam, w, h)
    assert rays.dtype == np.float32 and rays.shape == (w * h, 6) and rays.flags.c_contiguous
    assert np.abs(np.linalg.norm(rays[:, 3:].astype(np.float64), axis=1) - 1).max() < 2e-7
    t, ids = rq.scan(S, n, rays)["nearest"]
    c = (h // 2) * w + w // 2
    assert ids[c] == 2 and abs(float(t[c]) - 205.69) < 0.05
    assert abs(float(rays[c, 2]) + float(t[c]) * float(rays[c, 5])) < 0.05          # the hit lies on z = 0
    # x grows with the column, y with the row (cam.x, cam.y), as GenerateCameraRay's kcx / kcy
    assert rays[c + 1, 3] > rays[c, 3] and rays[c + w, 4] > rays[c, 4]
    assert (ids >= 0).all()                                                        # a closed room
    sel = rtamd.scenes.camera_rays(cam, w, h, [5, w // 2], [7, h // 2])
    assert (sel.view(np.uint32) == rays[[7 * w + 5, c]].view(np.uint32)).all()


def test_header_declares_the_query_surface():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "smallpt, ray queries" in src
    for name, val in (("SPT_QUERY_NEAREST", 0), ("SPT_QUERY_ANY", 1), ("SPT_QUERY_OCCLUDER", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src), name
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+spt_scene_query_async\(const spt_scene \*scene, const float \*d_rays, "
                     r"const float \*d_tmax, size_t nrays,\s*int kind, float \*d_t, int \*d_id, void \*stream\);", code)
    import rtamd
    assert "spt_scene_query_async" in rtamd._lib.EXPORTS
    assert (rtamd.SPT_QUERY_NEAREST, rtamd.SPT_QUERY_ANY, rtamd.SPT_QUERY_OCCLUDER) == (0, 1, 2)
    assert rtamd.SmallptScene.QUERY_KINDS == {"nearest": 0, "any": 1, "occluder": 2}


def test_null_scene_is_invalid_without_a_device():
    """The argument checks come before anything touches a device."""
    import rtamd
    q = rtamd.lib().spt_scene_query_async
    buf = (C.c_float * 6)()
    out = (C.c_int * 1)()
    for kind in (0, 1, 2, 7):
        assert q(None, C.addressof(buf), C.addressof(buf), 1, kind, None, C.addressof(out), None) == -1
    assert b"spt_scene_query_async" in rtamd.lib().rt_last_error()
