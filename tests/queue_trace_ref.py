"""The reference for rtq_trace: tests/native/queue_trace_ref.c (the oracle's own
q_raytrace under q_pixel's push and drain loop, driven by the caller's chains
of rays), built on demand with the oracle Makefile's CFLAGS, and the ray sets
the CPU pins and the GPU tests share.

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
SRC = os.path.join(HERE, "native", "queue_trace_ref.c")
LIB = os.path.join(HERE, "native", "libqueue_trace_ref.so")
NT = min(16, os.cpu_count() or 1)
F = np.float32
FAR = F(1e7)                      # d_t of a miss (raytracer_non_OpenCL.c:181)
_lib = None


def _oracle_cflags():
    text = open(os.path.join(O.ORACLE_DIR, "Makefile")).read()
    return shlex.split(re.search(r"^CFLAGS\s*=\s*(.*)$", text, re.M).group(1))


def lib():
    global _lib
    if _lib is None:
        deps = (SRC, os.path.join(O.ORACLE_DIR, "queue_oracle.c"), os.path.join(O.ORACLE_DIR, "oracle.h"))
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            tmp = "%s.%d.tmp" % (LIB, os.getpid())
            subprocess.run(["gcc"] + _oracle_cflags() + ["-shared", "-o", tmp, SRC, "-lm"], check=True)
            os.replace(tmp, LIB)
        L = C.CDLL(LIB)
        L.qtr_trace.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int]
        L.qtr_trace.restype = None
        _lib = L
    return _lib


def trace(prims, n, rays, group=1):
    """(colours float32 [nrays / group, 3], t float32 [nrays], id int32
    [nrays], counters [4]) of rays float32 [..., 6] in chains of `group`."""
    rays = np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)
    nr = rays.shape[0]
    assert 1 <= group <= 64 and nr % group == 0
    col, t, ids = np.empty((nr // group, 3), F), np.empty(nr, F), np.empty(nr, np.int32)
    cnt = (C.c_uint64 * 4)()
    lib().qtr_trace(C.addressof(prims), n, rays.ctypes.data, nr, group, col.ctypes.data, t.ctypes.data,
                    ids.ctypes.data, cnt, NT)
    return col, t, ids, list(cnt)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def same_floats(ref, got):
    """Bit-equal, except that where the reference holds a NaN any NaN will do."""
    ref, got = np.asarray(ref, F), np.asarray(got, F)
    return ref.shape == got.shape and bool(np.all((bits(ref) == bits(got)) | (np.isnan(ref) & np.isnan(got))))


def _frozen(rays, out):
    for a in (rays,) + out[:3]:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def camera_set(name, group):
    """The two camera-ray sets: "ref" the reference scene at 64 x 48, "deep"
    lit_scenes.queue_lit(QUEUE_EXACT_SEED) at 96 x 72 (the camera inside a
    glass sphere).  (P, n, w, h, rays [h, w, 9, 6], trace(rays, group)),
    computed once, arrays read-only."""
    import lit_scenes
    if name == "ref":
        (P, n), (w, h) = O.queue_scene(), (64, 48)
    else:
        P, n, _, _ = lit_scenes.queue_lit(lit_scenes.QUEUE_EXACT_SEED)
        w, h = lit_scenes.QUEUE_W, lit_scenes.QUEUE_H
    rays = rtamd.scenes.queue_camera_rays(w, h)
    return P, n, w, h, rays, _frozen(rays, trace(P, n, rays, group))


@functools.lru_cache(maxsize=None)
def case_set(case):
    """degenerate_prims.queue_case(case) through its camera rays at group 9:
    (P, n, w, h, rays, trace(), the oracle's frame, its counters)."""
    import degenerate_prims as D
    P, n, w, h, frame, cnt = D.queue_case(case)
    rays = rtamd.scenes.queue_camera_rays(w, h)
    return P, n, w, h, rays, _frozen(rays, trace(P, n, rays, 9)), frame, cnt


def frame_words(frame):
    """The oracle's uint8 [h, w, 4] frame as queue_pack's uint32 [h, w]."""
    return np.ascontiguousarray(frame).view(np.uint32)[..., 0]


MISS = (0.0, 100.0, 0.0, 0.0, 1.0, 0.0)          # above the reference scene's ceiling, pointing up


def arbitrary_rays(count=4096, seed=11):
    """Rays no camera makes: origins uniform in x [-7, 7], y [-5, 6],
    z [-7, 35], directions normal x a length in [0.1, 4] (not normalised)."""
    rng = np.random.default_rng(seed)
    o = rng.uniform((-7, -5, -7), (7, 6, 35), (count, 3))
    d = rng.standard_normal((count, 3))
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.1, 4.0, (count, 1))
    return np.concatenate([o, d], axis=1).astype(F)


def explicit_rows(P, n):
    """Rays that miss everything; rays starting inside each glass sphere; a
    root hit on each sphere light (from two units in front of it); zero-length
    directions; NaN and +-inf in every component of origin and direction."""
    rows = [MISS, (0, 100, 0, 0.3, 2.0, 0.1), (1000, 0, 0, 1, 0, 0)]
    for p in P[:n]:
        if p.type == 1 and not p.is_light and p.m_refr > 0:
            c = (p.center.x, p.center.y, p.center.z)
            rows += [c + (0.0, 0.0, 1.0), c + (0.6, -0.5, 0.2), (c[0] + 0.3 * p.radius, c[1], c[2], -1.0, 0.2, 0.1)]
        if p.type == 1 and p.is_light:
            c = (p.center.x, p.center.y, p.center.z)
            rows += [(c[0], c[1], c[2] - 2.0, 0.0, 0.0, 1.0), (c[0], c[1] - 2.0, c[2], 0.0, 0.5, 0.0)]
    rows += [(0, 0.25, -7, 0, 0, 0), (0, -3.4, 23, 0, 0, 0), (0, 0.25, -7, 0.0, -0.0, 0.0)]
    base = np.array([0.5, 0.25, -7.0, 0.05, -0.1, 1.0])
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            r = base.copy()
            r[k] = v
            rows.append(tuple(r))
    return np.array(rows, F)
