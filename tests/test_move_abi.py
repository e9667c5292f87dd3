"""The device-memory move's surface (no GPU compute here): the four entry
points are declared in include/rt_hip.h with the prototypes the issue gives,
exported by the built library, bound by rtamd._lib, and SmallptScene has the
methods that wrap them."""
import ctypes as C
import os
import subprocess

import test_abi

MOVE = ("spt_scene_move_prepare", "spt_scene_move_async", "spt_scene_move_info", "spt_scene_read_spheres")

# A declaration that differs from the header's in any parameter or in the
# return type is a compile error (conflicting types) in C.
PROTOTYPES = """
#include "rt_hip.h"
int spt_scene_move_prepare(spt_scene *scene, void *stream);
int spt_scene_move_async(spt_scene *scene, const float *d_geom, unsigned first, unsigned count, void *stream);
int spt_scene_move_info(const spt_scene *scene, uint64_t *out, int nout);
int spt_scene_read_spheres(const spt_scene *scene, rt_sphere *out, unsigned cap);
int (*const taken[])(void) = {(int (*)(void))spt_scene_move_prepare, (int (*)(void))spt_scene_move_async,
                              (int (*)(void))spt_scene_move_info, (int (*)(void))spt_scene_read_spheres};
int words[SPT_MOVE_INFO_WORDS == 3 ? 1 : -1];
"""


def test_header_declares_the_move_entry_points(tmp_path):
    names = test_abi.declared()
    for n in MOVE:
        assert n in names, n
    src = tmp_path / "move_protos.c"
    src.write_text(PROTOTYPES)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I" + os.path.join(test_abi.ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "move_protos.o")], check=True)


def test_library_exports_and_binds_them():
    import rtamd
    L = rtamd.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", rtamd._lib.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines()}
    vp, u, i = C.c_void_p, C.c_uint, C.c_int
    want = {"spt_scene_move_prepare": [vp, vp], "spt_scene_move_async": [vp, vp, u, u, vp],
            "spt_scene_move_info": [vp, vp, i], "spt_scene_read_spheres": [vp, vp, u]}
    for n in MOVE:
        assert n in exported and n in rtamd._lib.EXPORTS, n
        fn = rtamd._lib.entry(n)
        assert fn is getattr(L, n) or fn.argtypes == getattr(L, n).argtypes
        assert list(fn.argtypes) == want[n] and fn.restype is C.c_int, n


def test_smallpt_scene_has_the_methods():
    import rtamd
    for m in ("move", "move_prepare", "move_info", "spheres"):
        assert callable(getattr(rtamd.SmallptScene, m, None)), m
    assert rtamd.SmallptScene.MOVE_INFO == ("moves", "captured", "refits")
