"""Shared plumbing of the refit tests (tests/test_refit.py on the CPU,
tests/test_gpu_scene_update.py on the GPU): the native check
(tests/native/spt_refit_check.cpp, built here with one g++ call into a
temporary directory), the nine scenes, the five edits and the ray families.

TEST INFRASTRUCTURE ONLY (imported like oracle_lib and scenes_layouts)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import rtamd
import scenes_layouts as sl

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "spt_refit_check.cpp")
CSRC = os.path.join(os.path.dirname(HERE), "se-195-project-ray-tracer_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-pthread"]
SECTIONS = ("nodes", "geo", "ids", "wide", "maxid")

_lib = None


def native():
    """The check as a shared library (built once per process)."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="spt_refit_check_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libspt_refit_check.so")
        subprocess.run(["g++"] + FLAGS + ["-shared", "-fPIC", "-I" + CSRC, SRC, "-o", so], check=True)
        L = C.CDLL(so)
        P, LL = C.c_void_p, C.c_longlong
        L.rfc_create.restype = P
        L.rfc_create.argtypes = [P, C.c_int, C.c_int]
        L.rfc_destroy.argtypes = [P]
        L.rfc_sizes.argtypes = [P, P]
        L.rfc_sections.argtypes = [P, P]
        L.rfc_refit.argtypes = [P, P]
        L.rfc_check.restype = LL
        L.rfc_check.argtypes = [P, P, C.c_int]
        L.rfc_walk.restype = LL
        L.rfc_walk.argtypes = [P, P, P, LL, P, P]
        _lib = L
    return _lib


def split_sections(raw, sizes):
    """The five sections of a concatenated byte buffer, as spt_scene_read_hierarchy returns them."""
    out, o = {}, 0
    kinds = (np.float32, np.float32, np.int32, np.uint32, np.uint32)
    shapes = ((-1, 4), (-1, 4), (-1,), (-1, 28), (-1, 8))
    for name, nbytes, kind, shape in zip(SECTIONS, sizes, kinds, shapes):
        out[name] = raw[o:o + nbytes].view(kind).reshape(shape)
        o += nbytes
    return out


class Host:
    """One scene's sections on the host: built as spt_scene_create builds
    them (wide=False: RT_SPT_WIDE=0), refitted by spt_refit.h's refit_host."""

    def __init__(self, S, n, wide=True):
        self.L = native()
        self.n = n
        self.h = self.L.rfc_create(C.addressof(S), n, int(wide))
        assert self.h, "build_meta failed"
        out = (C.c_longlong * 12)()
        self.L.rfc_sizes(self.h, out)
        self.sizes = list(out[:5])
        (self.nodes, self.nb, self.na, self.wnodes, self.wdepth, self.leaf_max, self.meta_bytes) = out[5:12]

    def sections(self):
        raw = np.zeros(sum(self.sizes), np.uint8)
        self.L.rfc_sections(self.h, raw.ctypes.data)
        return split_sections(raw, self.sizes)

    def refit(self, S):
        self.L.rfc_refit(self.h, C.addressof(S))
        return self

    def check(self):
        """Violations of containment (0 expected) and the first one's text."""
        msg = C.create_string_buffer(256)
        return self.L.rfc_check(self.h, msg, 256), msg.value.decode()

    def walk(self, rays, maxt=None):
        """(mismatches of the walks against the full scan, the scan's t, its id)."""
        nr = len(rays)
        ts, ids = np.zeros(nr, np.float32), np.zeros(nr, np.int32)
        bad = self.L.rfc_walk(self.h, rays.ctypes.data, None if maxt is None else maxt.ctypes.data, nr,
                              ts.ctypes.data, ids.ctypes.data)
        return bad, ts, ids

    def close(self):
        if self.h:
            self.L.rfc_destroy(self.h)
            self.h = None


# ---- scenes -----------------------------------------------------------------
SCENES = {
    "n256": sl.n256,
    "no_always": sl.no_always,
    "many_always": lambda: sl.many_always()[0],
    "coincident": sl.coincident,
    "cloud3000": lambda: sl.cloud(sl.N_LEAF8),
    "cloud30000": lambda: sl.cloud(sl.N_LEAF12),
    "cloud43000": lambda: sl.cloud(sl.N_LEAF16),
    "cloud56000": lambda: sl.cloud(sl.N_NOWIDE),
    "degenerate": sl.degenerate_base,       # the cloud the degenerate kinds of scenes_layouts.py edit
}
LEAF = {"n256": 8, "no_always": 8, "many_always": 8, "coincident": 8, "cloud3000": 8, "cloud30000": 12,
        "cloud43000": 16, "cloud56000": 0, "degenerate": 8}


def raw_rows(S, n):
    """A copy of the spheres as float32 [n, 11] (refl as raw bits)."""
    return sl.rows_of(S, n).copy()


def from_raw(rows):
    """A Sphere array from raw_rows' form."""
    rows = np.ascontiguousarray(rows, np.float32)
    arr = (rtamd.Sphere * len(rows))()
    C.memmove(arr, rows.ctypes.data, rows.nbytes)
    return arr


# ---- edits ------------------------------------------------------------------
EDITS = (1, 2, 3, 4, 5)


def edit(k, rows, ids, nb):
    """Edit k of the scene `rows` (raw_rows' form), whose hierarchy order is
    `ids` (the first nb in the tree, the rest always spheres): a new array.
    Only radii and centres change."""
    rows = rows.copy()
    n = len(rows)
    tree, always = ids[:nb], ids[nb:]
    cen = rows[tree, 1:4].astype(np.float64)
    half = float(((cen.max(0) - cen.min(0)) / 2).max())
    med = np.float32(np.median(rows[:, 0]))
    rng = np.random.default_rng([20, k])
    if k == 1:          # 10 % moved by up to the half extent, radii x 2^U(-1, 1)
        pick = rng.choice(n, max(1, n // 10), replace=False)
        rows[pick, 1:4] += rng.uniform(-half, half, (len(pick), 3)).astype(np.float32)
        rows[pick, 0] *= (2.0 ** rng.uniform(-1, 1, len(pick))).astype(np.float32)
    elif k == 2:        # one sphere 10^3 x the extent away: the exponents grow
        rows[tree[len(tree) // 2], 1:4] += np.float32(1e3 * 2 * max(half, 1.0))
    elif k == 3:        # every radius x 2^-6: the exponents shrink
        rows[:, 0] *= np.float32(2.0 ** -6)
    elif k == 4:        # a tree sphere past 64 x the median, the first always sphere down to it
        rows[tree[len(tree) // 3], 0] = np.float32(100.0) * med
        if len(always):
            rows[always[0], 0] = med
    elif k == 5:        # every tree sphere on one point with one radius
        rows[tree, 1:4] = cen.mean(0).astype(np.float32)
        rows[tree, 0] = med
    return rows


# ---- rays (the families of tests/test_bvh_wide.py) ----------------------------
def rays(rng, centres, origin, nr, spread):
    o = centres[rng.integers(0, len(centres), nr)] + rng.normal(0, spread, (nr, 3))
    o[: nr // 8] = origin
    d = rng.normal(0, 1, (nr, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d[: nr // 16, 1] = 0.0                          # axis-parallel components (the 1e-30 clamp)
    d[: nr // 16] /= np.linalg.norm(d[: nr // 16], axis=1, keepdims=True)
    return np.ascontiguousarray(np.concatenate([o, d], 1).astype(np.float32))
