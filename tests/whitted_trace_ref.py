"""The reference for rtw_trace: tests/native/whitted_trace_ref.c (the oracle's
own engine_raytrace under the reference's tree loop, one sub-sample per
caller ray), built on demand with the oracle Makefile's CFLAGS, and the ray
sets the CPU pins and the GPU tests share.

TEST INFRASTRUCTURE ONLY (imported like oracle_lib and lit_scenes)."""
import ctypes as C
import functools
import os
import re
import shlex
import subprocess

import numpy as np

import oracle_lib as O
import rtamd

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "whitted_trace_ref.c")
LIB = os.path.join(HERE, "native", "libwhitted_trace_ref.so")
NT = min(16, os.cpu_count() or 1)
_lib = None


def _oracle_cflags():
    text = open(os.path.join(O.ORACLE_DIR, "Makefile")).read()
    return shlex.split(re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1))


def lib():
    global _lib
    if _lib is None:
        deps = (SRC, os.path.join(O.ORACLE_DIR, "whitted_oracle.c"), os.path.join(O.ORACLE_DIR, "oracle.h"))
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            tmp = "%s.%d.tmp" % (LIB, os.getpid())
            subprocess.run(["gcc"] + _oracle_cflags() + ["-shared", "-o", tmp, SRC, "-lm"], check=True)
            os.replace(tmp, LIB)
        L = C.CDLL(LIB)
        L.wtr_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.wtr_trace.restype = None
        _lib = L
    return _lib


def trace(prims, n, rays, ocl=False):
    """(colours float32 [n, 3], t float32 [n], id int32 [n], counters [4],
    stale [earlier node's ray, caller's own ray]) of rays float32 [..., 6]."""
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    nr = rays.shape[0]
    col, t, ids = np.empty((nr, 3), np.float32), np.empty(nr, np.float32), np.empty(nr, np.int32)
    cnt, stale = (C.c_uint64 * 4)(), (C.c_uint64 * 2)()
    lib().wtr_trace(C.addressof(prims), n, rays.ctypes.data, nr, int(ocl), col.ctypes.data, t.ctypes.data,
                    ids.ctypes.data, cnt, stale, NT)
    return col, t, ids, list(cnt), list(stale)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_floats(ref, got):
    """Bit-equal, except that where the reference holds a NaN any NaN will do."""
    ref, got = np.asarray(ref, np.float32), np.asarray(got, np.float32)
    return ref.shape == got.shape and bool(np.all((bits(ref) == bits(got)) | (np.isnan(ref) & np.isnan(got))))


def low_index_scene():
    """The reference scene with m_RIndex = 0.5 on every refractive sphere:
    entering one is already a total internal reflection for most rays, so the
    stale refraction ray is the caller's own."""
    P, n = O.whitted_scene()
    for p in P[:n]:
        if p.m_Refr > 0:
            p.m_RIndex = 0.5
    return P, n


@functools.lru_cache(maxsize=None)
def camera_set(name, ocl):
    """The two 64 x 48 camera-ray sets, rows [20, 48): "ref" the reference
    scene, "low" low_index_scene.  (P, n, rays [28, 64, nsub, 6], reference
    outputs of trace()), computed once, arrays read-only."""
    P, n = O.whitted_scene() if name == "ref" else low_index_scene()
    rays = rtamd.scenes.whitted_camera_rays(64, 48, 20, 48, ocl=ocl)
    out = trace(P, n, rays, ocl)
    for a in (rays,) + out[:3]:
        a.setflags(write=False)
    return P, n, rays, out


def window_rows(w, h, ocl):
    return (20, min(530, h)) if ocl else (20, h - 70)


@functools.lru_cache(maxsize=None)
def walled_set(seed, ocl):
    """lit_scenes.walled_oracle(seed) through its window's camera rays:
    (P, n, w, h, rays, reference outputs, the oracle's (frame, counters))."""
    import lit_scenes
    P, n, w, h, cpu, oc = lit_scenes.walled_oracle(seed)
    r0, r1 = window_rows(w, h, ocl)
    rays = rtamd.scenes.whitted_camera_rays(w, h, r0, r1, ocl=ocl)
    out = trace(P, n, rays, ocl)
    for a in (rays,) + out[:3]:
        a.setflags(write=False)
    return P, n, w, h, rays, out, (oc if ocl else cpu)
