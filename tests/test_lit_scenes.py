"""CPU only.  Two things the GPU parity tests stand on:

1. The lit random scenes (tests/lit_scenes.py) meet their conditions for
   every listed seed -- evaluated on the oracle's frames.
2. The oracle equals the reference's own code on whole frames, bit for bit:
   oracle/whitted_oracle.c against Engine_Render (raytracer.cpp compiled
   unmodified) and against raytrace_kernel (openCLcode.cl compiled as host
   C++; built-ins as glibc sqrtf / expf / powf), oracle/smallpt_oracle.c
   against the reference's radiance core, oracle/queue_oracle.c against
   raytracer_non_OpenCL.c -- on the lit scenes, on the older occlusion-heavy
   random scenes and on the hand-made edge scenes.  These skip where
   oracle/_ref is not built (no reference tree at build time).  The reference
   exposes no work counters: those stay pinned by the probe figures
   (tests/test_oracle.py).
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import lit_scenes as L
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "known_answers.json")))


# ---------------------------------------------------------------- conditions
@pytest.mark.parametrize("seed", L.WALLED_SEEDS)
def test_walled_scene_is_lit(seed):
    P, n, w, h, (cpu, _), (ocl, _) = L.walled_oracle(seed)
    wc, wo = L.whitted_windows(w, h)
    assert 60 <= w < 200 and 130 <= h < 180 and wc[1] - wc[0] >= 40
    assert 1 <= n <= 64
    L.check_lit(cpu, wc[:2])
    L.check_lit(ocl, wo[:2])
    # the rows outside the window stay untouched
    assert (cpu[:20] == 0).all() and (cpu[h - 70:] == 0).all() and (ocl[:20] == 0).all()


def test_walled_set_has_tir_and_deep_trees_and_every_feature():
    have = {}
    for sem in (0, 1):
        tir, rpp = [], []
        for seed in L.WALLED_SEEDS:
            P, n, w, h, *frames = L.walled_oracle(seed)
            cnt = frames[sem][1]
            tir.append(cnt[3] > 0)
            rpp.append(L.rays_per_primary(cnt, w, L.whitted_windows(w, h)[sem]))
            for k, v in L.walled_features(P, n).items():
                have[k] = have.get(k, False) or v
        assert 3 * sum(tir) >= len(tir), tir
        assert max(rpp) > 3.0, rpp
    assert all(have.values()) and set(have) == {"full", "plane_light", "mirror_plane", "nested_in_glass"}, have
    assert len(L.WALLED_SEEDS) >= 8 and L.WALLED_DEEP_SEED in L.WALLED_SEEDS
    P, n, w, h, (_, cnt), _ = L.walled_oracle(L.WALLED_DEEP_SEED)
    assert L.rays_per_primary(cnt, w, L.whitted_windows(w, h)[0]) > 3.0


def test_walled_walls_keep_everything_on_the_normal_side():
    """The placement rule itself: N.p + D > 0 at the camera and at every point
    of every sphere, for every wall of every listed scene."""
    for seed in L.WALLED_SEEDS:
        P, n, _, _ = L.whitted_walled(seed)
        for q in P[:n]:
            if q.type != L.PLANE:
                continue
            N = np.array([q.plane_N.x, q.plane_N.y, q.plane_N.z], np.float64)
            assert 0.29 <= np.linalg.norm(N) <= 1.51
            assert N @ L.CAMERA + q.plane_D > 0.4
            for s in P[:n]:
                if s.type == L.SPHERE:
                    c = np.array([s.m_Centre.x, s.m_Centre.y, s.m_Centre.z], np.float64)
                    assert N @ c - np.linalg.norm(N) * s.m_Radius + q.plane_D > 0.4, seed


@pytest.mark.parametrize("seed", L.QUEUE_SEEDS)
def test_queue_scene_is_lit(seed):
    P, n, frame, cnt = L.queue_lit(seed)
    assert frame.shape == (L.QUEUE_H, L.QUEUE_W, 4) and 1 <= n <= 64
    assert cnt[3] == 0                     # no undefined behaviour in the reference
    L.check_lit(frame)


def test_queue_set_keeps_the_hard_cases():
    have = {}
    for seed in L.QUEUE_SEEDS:
        P, n, _, _ = L.queue_lit(seed)
        for k, v in L.queue_features(P, n).items():
            have[k] = have.get(k, False) or v
    assert have == {"camera_inside": True, "extra_planes": True, "glass": True}
    assert len(L.QUEUE_SEEDS) >= 8


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", L.ROOM_SEEDS)
def test_room_scene_is_lit(seed, mode):
    S, n, cam, w, h, steps, ref = L.room_oracle(seed, mode)
    assert 24 <= w < 90 and 16 <= h < 70 and 9 <= n <= 38 and len(steps) == 2
    L.check_lit(ref[2])
    assert np.isfinite(ref[0]).all()


def test_room_set_covers_all_materials():
    assert len(L.ROOM_SEEDS) >= 6
    for seed in L.ROOM_SEEDS:
        S, n = L.smallpt_room(seed)[:2]
        assert sum(1 for s in S[:n] if s.rad == np.float32(1e4)) == 6
        assert 1 <= sum(1 for s in S[:n] if s.e.x > 0) <= 3
    refl = {s.refl for seed in L.ROOM_SEEDS for s in L.smallpt_room(seed)[0]}
    assert refl == {L.DIFF, L.SPEC, L.REFR}
    assert any(s.refl == L.SPEC and s.rad == np.float32(1e4) for seed in L.ROOM_SEEDS for s in L.smallpt_room(seed)[0])


# ---------------------------------------------------------------- Whitted: oracle == reference build
def _need_ref_whitted():
    libs = O.ref_libs()
    if libs is None or not (hasattr(libs[0], "ref_whitted_render") and hasattr(libs[0], "ref_whitted_render_ocl")):
        pytest.skip("oracle/_ref not built (no reference tree at build time)")


@functools.lru_cache(maxsize=None)
def _ref_scene_frame(w, h):
    f = O.ref_whitted_render(w, h)
    f.setflags(write=False)
    return f


def _same(ref, got, what):
    bad = np.argwhere(ref != got)
    assert bad.size == 0, "%s: %d pixels differ, first at %s (reference %x, oracle %x)" % (
        what, len(bad), bad[0].tolist(), ref[tuple(bad[0])], got[tuple(bad[0])])


def _pin_both(P, n, w, h, what, cpu=None, ocl=None):
    cpu = O.whitted_render(w, h, nthreads=L.NT, prims=P, n=n)[0] if cpu is None else cpu
    ocl = O.whitted_render_ocl(w, h, nthreads=L.NT, prims=P, n=n)[0] if ocl is None else ocl
    _same(O.ref_whitted_render(w, h, P, n), cpu, what + " (Engine_Render)")
    _same(O.ref_whitted_render_ocl(w, h, P, n), ocl, what + " (raytrace_kernel)")


@pytest.mark.parametrize("w,h", [(640, 480), (97, 131), (33, 91)])
def test_whitted_oracle_is_the_reference_engine_reference_scene(w, h):
    _need_ref_whitted()
    _same(_ref_scene_frame(w, h), O.whitted_render(w, h, nthreads=L.NT)[0], "%dx%d (Engine_Render)" % (w, h))
    _same(O.ref_whitted_render_ocl(w, h), O.whitted_render_ocl(w, h, nthreads=L.NT)[0],
          "%dx%d (raytrace_kernel)" % (w, h))


def test_reference_engine_probe_pixel_and_layout():
    """The build is the probed program: pixel (400, 300) of 640x480 is the
    probe's, rows outside [20, h - 70) are not written, and both translation
    units see the 96-byte Primitive."""
    _need_ref_whitted()
    W = O.ref_libs()[0]
    assert W.ref_sizeof_primitive() == 96 and W.ref_ocl_sizeof_primitive() == 96
    f = _ref_scene_frame(640, 480)
    assert int(f[300, 400]) == GOLD["survey"]["whitted_pixel_400_300"]["640x480"] == 0xccaaaa
    assert (f[:20] == 0).all() and (f[410:] == 0).all() and (f[20:410] != 0).any()


@pytest.mark.parametrize("key", ["640x480", "800x600"])
def test_whitted_goldens_are_the_reference_engines_frames(key):
    """The committed golden hashes are generated from the oracle
    (tests/golden/make_golden.py); here they are checked against the frame
    the reference's own Engine_Render writes."""
    _need_ref_whitted()
    w, h = map(int, key.split("x"))
    assert O.fnv1a64(_ref_scene_frame(w, h)) == GOLD["whitted"][key]["xrgb"]


@pytest.mark.parametrize("seed", L.WALLED_SEEDS)
def test_whitted_oracle_is_the_reference_engine_walled(seed):
    _need_ref_whitted()
    P, n, w, h, (cpu, _), (ocl, _) = L.walled_oracle(seed)
    _pin_both(P, n, w, h, "walled seed %d" % seed, cpu, ocl)


@pytest.mark.parametrize("seed", [21, 22, 23, 24, 25, 26, 27])
def test_whitted_oracle_is_the_reference_engine_unconstrained(seed):
    _need_ref_whitted()
    P, n, w, h = L.whitted_unconstrained(seed)
    _pin_both(P, n, w, h, "unconstrained seed %d" % seed)


def test_whitted_oracle_is_the_reference_engine_edge_scenes():
    _need_ref_whitted()
    for name, P, n, w, h in L.whitted_edge_scenes():
        _pin_both(P, n, w, h, name)


# ---------------------------------------------------------------- smallpt: oracle == reference core
def _pin_smallpt(scene, mode):
    libs = O.ref_libs()
    if libs is None:
        pytest.skip("oracle/_ref not built (no reference tree at build time)")
    S, n, cam, w, h, steps = scene
    assert len(steps) == 2
    col, seeds, px, _ = L.oracle_frame(O, w, h, list(steps), mode=mode, scene=(S, n), cam=cam, nthreads=L.NT)
    c2 = np.zeros(3 * w * h, np.float32)
    s2 = O.seeds(w, h)
    p2 = np.zeros(w * h, np.uint32)
    first = 0
    for k in steps:
        libs[1].ref_smallpt_render(C.cast(S, C.POINTER(O.Sphere)), n, C.cast(C.pointer(cam), C.POINTER(O.Camera)),
                                   c2.ctypes.data, s2.ctypes.data, p2.ctypes.data, w, h, 0, h, first, k, mode)
        first += k
    assert (col.view(np.uint32) == c2.view(np.uint32)).all()
    assert (seeds == s2).all() and (px == p2).all()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", L.ROOM_SEEDS)
def test_smallpt_oracle_is_the_reference_core_rooms(seed, mode):
    _pin_smallpt(L.smallpt_room(seed), mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("seed", [11, 12, 13, 14, 15, 16])
def test_smallpt_oracle_is_the_reference_core_unconstrained(seed, mode):
    _pin_smallpt(L.smallpt_unconstrained(seed), mode)


# ---------------------------------------------------------------- queue tracer: oracle == reference build
@pytest.mark.parametrize("seed", L.QUEUE_SEEDS)
def test_queue_oracle_is_the_reference_build_lit_scenes(seed):
    Q = O.ref_queue_lib()
    if Q is None:
        pytest.skip("oracle/_ref not built (no reference tree at build time)")
    P, n, frame, _ = L.queue_lit(seed)
    assert (O.ref_queue_render(Q, L.QUEUE_W, L.QUEUE_H, P, n) == frame).all()
