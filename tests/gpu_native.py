"""ctypes drivers for tests/native/libgpu_math_check.so and libgpu_prims_check.so
(test infrastructure)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")

# (name, fn id, lo, hi) float-bit ranges: the hot path's input domains.
DOMAINS = [
    ("powf_y20", 0, 0x00000000, 0x40000000),     # raytracer.cpp:165, dot in (0, 2]
    ("powf_y20_above2", 0, 0x40000001, 0x7f800000),   # the same with a non-unit normal: any dot > 0, +inf too
    ("powf_gamma", 1, 0x00000000, 0x3f800000),   # vec.h:62, [0, 1]
    ("powf_gamma_negzero", 1, 0x80000000, 0x80000000),
    ("expf_all", 2, 0x00000000, 0xffffffff),     # raytracer.cpp:487-489
    ("sinf", 3, 0x00000000, 0x41000000),         # geomfunc.h:66,262, [0, 8]
    ("cosf", 4, 0x00000000, 0x41000000),         # geomfunc.h:65,261
    ("sincosf_sin", 5, 0x00000000, 0x41000000),  # branch-free pair used by smallpt.hip
    ("sincosf_cos", 6, 0x00000000, 0x41000000),
    ("sincosf_sin_neg", 5, 0x80000000, 0xc1000000),
    ("sincosf_cos_neg", 6, 0x80000000, 0xc1000000),
    ("sqrt_rn_pos", 7, 0x00000000, 0x7fffffff),  # rt_common.h sqrt_rn: every non-negative float, NaNs
    ("sqrt_rn_neg", 7, 0x80000000, 0xffffffff),  # every negative float (NaN results, -0)
    # rt_common.h short forms: sqrt_nr / rcp_nr on their stated ranges, and the
    # guarded sqrt_exact / inv_len (uniform fallback) on every float
    ("sqrt_nr_range", 11, 0x0f800000, 0x7f7fffff),   # [2^-96, FLT_MAX]
    ("rcp_nr_range", 10, 0x00800000, 0x7c7fffff),    # [2^-126, 2^126)
    ("rcp_nr_range_neg", 10, 0x80800000, 0xfc7fffff),
    ("sqrt_exact_all", 8, 0x00000000, 0xffffffff),
    ("inv_len_all", 9, 0x00000000, 0xffffffff),
]


def lib():
    path = os.path.join(HERE, "libgpu_math_check.so")
    if not os.path.exists(path):
        subprocess.run(["make", "-s", "-C", HERE, "libgpu_math_check.so"], check=True)
    L = C.CDLL(path)
    L.gmc_run.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.gmc_run_pow20.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.gmc_run_cvt.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.gmc_run_spec20.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_int] + [C.c_void_p] * 7
    return L


# ------------------------------------------------------------------ rt_prims.h
MAXP = 64
# prims::PrimLists (rt_prims.h), field for field
IMAGE = np.dtype([("sph", "<f4", (MAXP, 4)), ("pln", "<f4", (MAXP, 4)), ("sph_id", "<i4", MAXP),
                  ("pln_id", "<i4", MAXP), ("osph", "<f4", (MAXP, 4)), ("opln", "<f4", (MAXP, 4)),
                  ("osph_pos", "<i4", MAXP), ("opln_pos", "<i4", MAXP), ("n", "<i4"), ("ns", "<i4"),
                  ("np", "<i4"), ("nos", "<i4"), ("nop", "<i4"), ("nlights", "<i4"), ("nnonlight", "<i4"),
                  ("pad_", "<i4")])

_prims_lib = None


def prims_lib():
    """tests/native/libgpu_prims_check.so: rt_prims.h's loops over the caller's
    scene and rays (gpu_prims_check.hip)."""
    global _prims_lib
    if _prims_lib is None:
        path = os.path.join(HERE, "libgpu_prims_check.so")
        if not os.path.exists(path):
            subprocess.run(["make", "-s", "-C", HERE, "libgpu_prims_check.so"], check=True)
        L = C.CDLL(path)
        vp = C.c_void_p
        L.gpc_build.argtypes = [vp] * 9
        L.gpc_nearest.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
        L.gpc_occluder.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
        L.gpc_len_inv.argtypes = [vp, C.c_int, vp]
        assert L.gpc_image_bytes() == IMAGE.itemsize
        _prims_lib = L
    return _prims_lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d)" % (what, rc))


def prims_build(valid, is_sphere, is_plane, is_light, is_occluder, sph, pln):
    """fill_lists on the device over MAXP lanes: (image, a 0-d array of dtype
    IMAGE; rank int32[MAXP], the per-lane light rank)."""
    L = prims_lib()
    flags = [np.ascontiguousarray(a, dtype=np.int32) for a in (valid, is_sphere, is_plane, is_light, is_occluder)]
    geo = [np.ascontiguousarray(a, dtype=np.float32) for a in (sph, pln)]
    assert all(a.shape == (MAXP,) for a in flags) and all(a.shape == (MAXP, 4) for a in geo)
    image = np.zeros((), IMAGE)
    rank = np.zeros(MAXP, np.int32)
    _check(L.gpc_build(*[a.ctypes.data for a in flags + geo], image.ctypes.data, rank.ctypes.data), "gpc_build")
    return image, rank


def _rays(rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    assert rays.ndim == 2 and rays.shape[1] == 6
    return rays


def prims_nearest(image, rays, R, traits, shift=0):
    """nearest_n<R, traits> ("whitted" / "queue"), ray i in lane i and, for
    R = 2, ray (i + shift) % n beside it: (dist bits uint32, prim int32,
    result int32), each of shape [R, n] -- row s is the lanes' slot s."""
    rays = _rays(rays)
    n = len(rays)
    out = np.zeros((R, n, 3), np.uint32)
    _check(prims_lib().gpc_nearest(image.ctypes.data, rays.ctypes.data, n, R, {"whitted": 0, "queue": 1}[traits],
                                   shift, out.ctypes.data), "gpc_nearest")
    return out[:, :, 0].copy(), out[:, :, 1].astype(np.int32), out[:, :, 2].astype(np.int32)


def prims_occluder(image, rays, lens, count):
    """first_occluder<count> entered with 0x7fffffff: int32[n]."""
    rays = _rays(rays)
    lens = np.ascontiguousarray(lens, dtype=np.float32)
    assert lens.shape == (len(rays),)
    out = np.zeros(len(rays), np.int32)
    _check(prims_lib().gpc_occluder(image.ctypes.data, rays.ctypes.data, lens.ctypes.data, len(rays), int(bool(count)),
                                    out.ctypes.data), "gpc_occluder")
    return out


def prims_len_inv(d2):
    """light_len_inv: (len bits, inv bits), uint32[n] each."""
    d2 = np.ascontiguousarray(d2, dtype=np.float32)
    out = np.zeros((len(d2), 2), np.uint32)
    _check(prims_lib().gpc_len_inv(d2.ctypes.data, len(d2), out.ctypes.data), "gpc_len_inv")
    return out[:, 0].copy(), out[:, 1].copy()


def pow20_check(lo=0x00000001, hi=0x40800000):
    """rtm::pow_d(x, 20.0) on the device vs the host glibc pow for every float
    x with bits in [lo, hi] (default: (0, 4]); (count, mismatches, first bad)."""
    L = lib()
    bad, first = C.c_uint64(), C.c_uint32()
    rc = L.gmc_run_pow20(lo, hi, C.byref(bad), C.byref(first))
    if rc != 0:
        raise RuntimeError("gmc_run_pow20 failed (%d)" % rc)
    return hi - lo + 1, bad.value, hex(first.value)


def cvt_check(lo=0x00000000, hi=0xffffffff):
    """rt::cvt_i32_x86 on the device vs the host's (int)f (cvttss2si) for every
    float with bits in [lo, hi], as integers; (count, mismatches, first bad)."""
    bad, first = C.c_uint64(), C.c_uint32()
    rc = lib().gmc_run_cvt(lo, hi, C.byref(bad), C.byref(first))
    if rc != 0:
        raise RuntimeError("gmc_run_cvt failed (%d)" % rc)
    return hi - lo + 1, bad.value, hex(first.value)


def spec20_check(pspec_bits, lo=0x00000001, hi=0x40000000):
    """rt::queue::spec20<false> vs spec20<true> on the device for every float dp
    with bits in [lo, hi] (default: (0, 2]) and each pspec (float32 bit
    patterns).  Per pspec bits: a dict of `wrong` (certified but different:
    count, inputs), `uncertified` (count, inputs), `uncertified_hi` (the count
    at or above 0x3c000000) and `host_uncertified` (count, inputs: the same
    certificate run on the host).  Input lists hold at most spec20 cap
    entries: all of them, ascending, while the count is within the cap; past
    it the host's are the smallest and the device's any."""
    L = lib()
    cap, n = L.gmc_spec20_cap(), len(pspec_bits)
    ps = np.array(pspec_bits, np.uint32).view(np.float32)
    wrong, unc, unc_hi, hunc = (np.zeros(n, np.uint64) for _ in range(4))
    wl, ul, hl = (np.zeros((n, cap), np.uint32) for _ in range(3))
    rc = L.gmc_run_spec20(lo, hi, ps.ctypes.data, n, wrong.ctypes.data, unc.ctypes.data, unc_hi.ctypes.data,
                          wl.ctypes.data, ul.ctypes.data, hunc.ctypes.data, hl.ctypes.data)
    if rc != 0:
        raise RuntimeError("gmc_run_spec20 failed (%d)" % rc)
    return {int(b): {"wrong": (int(wrong[j]), wl[j, :min(int(wrong[j]), cap)].tolist()),
                     "uncertified": (int(unc[j]), ul[j, :min(int(unc[j]), cap)].tolist()),
                     "uncertified_hi": int(unc_hi[j]),
                     "host_uncertified": (int(hunc[j]), hl[j, :min(int(hunc[j]), cap)].tolist())}
            for j, b in enumerate(pspec_bits)}


def math_check(domains=DOMAINS):
    L = lib()
    out = {}
    for name, fn, lo, hi in domains:
        bad, first = C.c_uint64(), C.c_uint32()
        rc = L.gmc_run(fn, lo, hi, C.byref(bad), C.byref(first))
        if rc != 0:
            raise RuntimeError("gmc_run failed (%d) on %s" % (rc, name))
        out[name] = (hi - lo + 1, bad.value, hex(first.value))
    return out
