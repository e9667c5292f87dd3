"""Shared plumbing of the regroup tests (tests/test_regroup.py on the CPU,
tests/test_gpu_regroup.py on the GPU): the native check
(tests/native/spt_regroup_check.cpp, built here with one g++ call into a
temporary directory) behind refit_check.Host's interface, a direct
recomputation of the 8-wide highest-index table, and the permuted scene.

TEST INFRASTRUCTURE ONLY (imported like refit_check and scenes_layouts)."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import refit_check as rc

SRC = os.path.join(rc.HERE, "native", "spt_regroup_check.cpp")

_lib = None


def native():
    """The check as a shared library (built once per process)."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="spt_regroup_check_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        so = os.path.join(d, "libspt_regroup_check.so")
        subprocess.run(["g++"] + rc.FLAGS + ["-shared", "-fPIC", "-I" + rc.CSRC, SRC, "-o", so], check=True)
        L = C.CDLL(so)
        P, LL = C.c_void_p, C.c_longlong
        L.rgc_create.restype = P
        L.rgc_create.argtypes = [P, C.c_int, C.c_int]
        L.rgc_destroy.argtypes = [P]
        L.rgc_state.restype = P
        L.rgc_state.argtypes = [P]
        L.rgc_regroup.argtypes = [P, P]
        L.rgc_area.restype = C.c_double
        L.rgc_area.argtypes = [P]
        L.rgc_plan.argtypes = [P, C.c_int, P]
        # spt_refit_check.cpp's entry points, over rgc_state's pointer
        L.rfc_sizes.argtypes = [P, P]
        L.rfc_sections.argtypes = [P, P]
        L.rfc_refit.argtypes = [P, P]
        L.rfc_check.restype = LL
        L.rfc_check.argtypes = [P, P, C.c_int]
        L.rfc_walk.restype = LL
        L.rfc_walk.argtypes = [P, P, P, LL, P, P]
        _lib = L
    return _lib


class Host(rc.Host):
    """refit_check.Host plus regroup_host (spt_regroup.h), the summed surface
    area of the binary nodes' boxes and the launch plan's counts."""

    def __init__(self, S, n, wide=True):
        self.L = native()
        self.n = n
        self.g = self.L.rgc_create(C.addressof(S), n, int(wide))
        assert self.g, "build_meta failed"
        self.h = self.L.rgc_state(self.g)
        out = (C.c_longlong * 12)()
        self.L.rfc_sizes(self.h, out)
        self.sizes = list(out[:5])
        (self.nodes, self.nb, self.na, self.wnodes, self.wdepth, self.leaf_max, self.meta_bytes) = out[5:12]

    def regroup(self, S):
        self.L.rgc_regroup(self.g, C.addressof(S))
        return self

    def area(self):
        return float(self.L.rgc_area(self.g))

    def plan(self, sub_max=-1):
        """(levels of the tree, levels sorted by global passes, subtree roots of
        the LDS tier) with that tier given subtrees of at most sub_max entries
        (default: the library's own size)."""
        out = (C.c_longlong * 3)()
        self.L.rgc_plan(self.g, sub_max, out)
        return tuple(out)

    def close(self):
        if self.g:
            self.L.rgc_destroy(self.g)
            self.g = self.h = None


def maxid_direct(sec):
    """The 8-wide highest-index table recomputed from the child words and ids
    alone: a leaf child's word holds its entry range, a wide child's highest
    index is the highest of its own slots (children follow their parent)."""
    wide, ids = sec["wide"], sec["ids"]
    out = np.zeros((len(wide), 8), np.uint32)
    valid = [[s for s in range(8) if (int(w[3]) >> (24 + s)) & 1] for w in wide]
    for w in range(len(wide) - 1, -1, -1):
        for s in valid[w]:
            cw = int(wide[w, 8 + s].view(np.int32))
            if cw < 0:
                first, count = (~cw) & 0xffffff, (~cw) >> 24
                out[w, s] = ids[first:first + count].max()
            else:
                out[w, s] = out[cw, valid[cw]].max()
    return out


def first_difference(got, want):
    """"" if two dicts of sections are equal word for word, else a line that names the first differing word."""
    for k in rc.SECTIONS:
        a, b = got[k].view(np.uint32).ravel(), want[k].view(np.uint32).ravel()
        if a.shape != b.shape:
            return "%s: %d words against %d" % (k, a.size, b.size)
        if (a != b).any():
            i = int(np.argmax(a != b))
            return "%s: %d words differ, first word %d: %#x against %#x" % (k, int((a != b).sum()), i, a[i], b[i])
    return ""


def permuted(rows, ids, nb, seed=5):
    """`rows` with (radius, centre) permuted among the tree spheres ids[:nb]
    (a fixed seed); the always spheres stay.  Returns (rows, perm) with
    new[tree[j]] = old[tree[perm[j]]]."""
    rows = rows.copy()
    tree = ids[:nb]
    perm = np.random.default_rng(seed).permutation(nb)
    rows[tree, 0:4] = rows[tree[perm], 0:4]
    return rows, perm
