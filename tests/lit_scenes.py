"""Random scenes whose frames carry colour, shared by the CPU pins of the
oracle and the GPU parity tests of the three tracers.

The older random-scene tests draw unconstrained scenes; most of those come out
black or one flat value (random planes cut every point off from every light),
so only the work counters tell a right kernel from a wrong one there.  The
generators below place the geometry so that light reaches the camera, and the
seed lists hold only seeds whose frames meet CONDITIONS -- evaluated on the
reference side (the oracle's frame), never on the GPU's:

  * at least MIN_LIT of the rendered window is non-black,
  * at least MIN_DISTINCT distinct pixel values,
  * per Whitted set: TIR events in at least a third of the scenes, and one
    scene above 3 traced rays per primary ray.

tests/test_lit_scenes.py asserts them for every listed seed; each GPU test
asserts them again on the oracle's frame before it compares (check_lit), so
an empty scene never passes silently.

TEST INFRASTRUCTURE ONLY (imported like oracle_lib and scenes_layouts)."""
import functools
import os

import numpy as np

import oracle_lib as O
import rtamd
from rtamd.scenes import DIFF, PLANE, REFR, SPEC, SPHERE, _prim, _sphere
from spt_check import oracle_frame

MIN_LIT = 0.25
MIN_DISTINCT = 100
NT = min(16, os.cpu_count() or 1)
CAMERA = np.array([0.0, 0.25, -7.0])        # the Whitted and the queue tracer's eye

# Seeds that meet the conditions (chosen on the CPU with the oracle; the
# reference builds give the same frames, tests/test_lit_scenes.py).
WALLED_SEEDS = (100, 101, 102, 104, 105, 106, 107, 108, 109, 110, 111, 113)   # (103: 16 % lit under OpenCL semantics)
WALLED_DEEP_SEED = 107                       # the deepest trees of the set: 9.4 traced rays per primary ray
QUEUE_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9)
QUEUE_EXACT_SEED = 3                         # the camera inside a glass sphere
QUEUE_POOL_SEED = 1                          # 511,547 rays in 6,912 trees
ROOM_SEEDS = (200, 201, 202, 203, 204, 205, 206, 207)


def lit_stats(frame, window=None):
    """(fraction of non-black pixels, distinct pixel values) of the rows
    `window` = (r0, r1) of a frame: uint32 [h, w], uint8 [h, w, 4] (the queue
    tracer's) or a flat uint32 array (smallpt's pixels; then no window)."""
    a = np.ascontiguousarray(frame)
    if a.dtype == np.uint8:
        a = a.view(np.uint32)[..., 0]
    if window is not None:
        a = a[window[0]:window[1]]
    return float((a != 0).mean()), int(np.unique(a).size)


def check_lit(frame, window=None):
    """Asserts the per-scene conditions on a reference-side frame."""
    lit, distinct = lit_stats(frame, window)
    assert lit >= MIN_LIT, "only %.1f %% of the window is non-black" % (100 * lit)
    assert distinct >= MIN_DISTINCT, "only %d distinct pixel values" % distinct
    return lit, distinct


# ---------------------------------------------------------------- Whitted
def whitted_walled(seed):
    """(prims, n, w, h): 1-4 small sphere lights high in the scene, 3-39
    spheres in front of the camera (mirrors, glass of index 1.0-2.6, diffuse,
    specular: the material mix of test_random_scenes_vs_oracle) and 1-6
    planes placed as walls.  A wall has a random normal N, |N| in [0.3, 1.5],
    and D = margin - min(N.c - |N| r) over the camera and every sphere (c, r),
    margin in [0.5, 6]: the camera, every sphere and every light lie on the
    side N points to (N.p + D >= margin there), the reference scene's own
    convention, so no wall hides a light from what it lights.  Some scenes
    fill all 64 primitive slots, flag a wall as a light, make walls mirrors or
    put a sphere inside a glass one.  Primitive order is shuffled."""
    rng = np.random.default_rng(seed)
    full = seed % 6 == 5                                   # MAXP primitives
    nlights = int(rng.integers(1, 5))
    nplanes = int(rng.integers(1, 7))
    nspheres = 64 - nlights - nplanes if full else int(rng.integers(3, 40))
    nested = rng.random() < 0.4
    plane_light = rng.random() < 0.25
    glassy = float(rng.uniform(0.25, 0.6))                 # this scene's share of glass and of mirrors
    rows = []                                              # _prim's arguments after the Primitive
    balls = [(CAMERA, 0.0)]
    for _ in range(nlights):
        c = (rng.uniform(-6, 6), rng.uniform(5, 9), rng.uniform(2, 30))
        g = float(rng.uniform(0.6, 1.0))
        rows.append((SPHERE, *c, 0.35, g, g, g, 0.0, 0.0, 0.0, float(rng.uniform(0, 1)), 1.8, True))
        balls.append((np.array(c), 0.35))
    for i in range(nspheres):
        if nested and i == 1:                              # inside sphere 0, which is then glass
            c0, r0 = balls[nlights + 1]
            r = float(r0 * rng.uniform(0.3, 0.5))
            c = tuple(c0 + rng.uniform(-0.3, 0.3, 3) * r0)
        else:
            r = float(rng.uniform(0.3, 3.0))
            c = (rng.uniform(-8, 8), rng.uniform(-6, 4.5), rng.uniform(8, 40))
        refl = float(rng.uniform(0.1, 1.9)) if rng.random() < glassy else 0.0
        refr = float(rng.uniform(0.3, 1.5)) if rng.random() < glassy or (nested and i == 0) else 0.0
        rows.append((SPHERE, *c, r, *rng.uniform(0.05, 1.8, 3), refl, refr, float(rng.uniform(1.0, 2.6)),
                     float(rng.uniform(0, 1.2)), float(rng.uniform(0, 1.8)), False))
        balls.append((np.array(c), r))
    for i in range(nplanes):
        nrm = rng.standard_normal(3)
        nrm *= rng.uniform(0.3, 1.5) / np.linalg.norm(nrm)
        ln = float(np.linalg.norm(nrm))
        d = float(rng.uniform(0.5, 6.0)) - min(float(nrm @ c) - ln * r for c, r in balls)
        rows.append((PLANE, *nrm, d, *rng.uniform(0.05, 2.5, 3),
                     float(rng.uniform(0.1, 0.9)) if rng.random() < 0.35 else 0.0, 0.0, 1.0,
                     float(rng.uniform(0.2, 1.2)), float(rng.uniform(0, 1.5)), plane_light and i == 0))
    order = rng.permutation(len(rows))
    P = (rtamd.Primitive * len(rows))()
    for k, j in enumerate(order):
        _prim(P[k], *rows[j])
    w, h = int(rng.integers(60, 200)), int(rng.integers(130, 180))
    return P, len(rows), w, h


def walled_features(P, n):
    """What whitted_walled put into a scene, read back from the primitives:
    a dict of booleans."""
    sph = [p for p in P[:n] if p.type == SPHERE]

    def inside(a, b):                                      # sphere a wholly inside sphere b
        d = np.linalg.norm([a.m_Centre.x - b.m_Centre.x, a.m_Centre.y - b.m_Centre.y, a.m_Centre.z - b.m_Centre.z])
        return a is not b and d + a.m_Radius < b.m_Radius
    return {"full": n == 64,
            "plane_light": any(p.type == PLANE and p.m_Light for p in P[:n]),
            "mirror_plane": any(p.type == PLANE and p.m_Refl > 0 and not p.m_Light for p in P[:n]),
            "nested_in_glass": any(inside(a, b) and b.m_Refr > 0 and not b.m_Light for a in sph for b in sph)}


@functools.lru_cache(maxsize=None)
def walled_oracle(seed):
    """whitted_walled(seed) and the oracle's two frames of it, computed once:
    (P, n, w, h, (frame, counters), (frame_ocl, counters_ocl)), frames
    read-only."""
    P, n, w, h = whitted_walled(seed)
    cpu = O.whitted_render(w, h, nthreads=NT, prims=P, n=n)
    ocl = O.whitted_render_ocl(w, h, nthreads=NT, prims=P, n=n)
    cpu[0].setflags(write=False)
    ocl[0].setflags(write=False)
    return P, n, w, h, cpu, ocl


def whitted_windows(w, h):
    """The rows Engine_Render and raytrace_kernel write, and their primary
    rays per pixel: ((r0, r1, 9), (r0, r1, 4))."""
    return (20, h - 70, 9), (20, min(530, h), 4)


def rays_per_primary(counters, w, window):
    r0, r1, spp = window
    return counters[0] / float(w * (r1 - r0) * spp)


def whitted_unconstrained(seed):
    """(prims, n, w, h) of test_gpu_whitted.test_random_scenes_vs_oracle's
    seed (21-27), draw for draw: the occlusion-heavy scenes, mostly black.
    Restated here so the CPU pins can run the reference build on them; that
    GPU test keeps its own copy."""
    rng = np.random.default_rng(seed)
    n = 64 if seed == 27 else int(rng.integers(4, 48))
    P = (rtamd.Primitive * n)()
    for i in range(n):
        light = i < 2 or rng.random() < 0.08
        if rng.random() < 0.75:
            c = (rng.uniform(-8, 8), rng.uniform(-6, 7), rng.uniform(8, 40))
            _prim(P[i], SPHERE, *c, float(rng.uniform(0.2, 4.0)), *rng.uniform(0.05, 1.8, 3),
                  float(rng.choice([0.0, 0.0, rng.uniform(0.1, 1.9)])),
                  float(rng.choice([0.0, 0.0, rng.uniform(0.3, 1.5)])),
                  float(rng.uniform(1.0, 2.6)), float(rng.uniform(0, 1.2)), float(rng.uniform(0, 1.8)), light)
        else:
            nrm = rng.standard_normal(3)
            _prim(P[i], PLANE, *nrm, float(rng.uniform(2, 12)), *rng.uniform(0.05, 2.5, 3),
                  float(rng.choice([0.0, rng.uniform(0.1, 0.9)])), 0.0, 1.0,
                  float(rng.uniform(0, 1.2)), float(rng.uniform(0, 1.5)), light and rng.random() < 0.3)
    w, h = int(rng.integers(60, 200)), int(rng.integers(100, 160))
    return P, n, w, h


def whitted_edge_scenes():
    """[(name, prims, n, w, h)]: the small hand-made scenes of
    test_gpu_whitted (both single-primitive scenes; the reference scene plus
    a sphere of infinite radius and one of radius 1e-15)."""
    out = []
    for light in (False, True):
        P = (rtamd.Primitive * 1)()
        _prim(P[0], SPHERE, 0.5, 0.0, 12.0, 2.0, 0.7, 0.6, 0.5, 0.4, 0.0, 1.0, 0.8, 0.6, light)
        out.append(("single_light" if light else "single", P, 1, 96, 128))
    S, n = rtamd.scenes.whitted_scene()
    P = (rtamd.Primitive * (n + 2))()
    for i in range(n):
        P[i] = S[i]
    _prim(P[n], SPHERE, 1.0, -2.0, 25.0, float("inf"), 0.5, 0.5, 0.5, 0.0, 0.0, 1.0, 1.0, 0.0, False)
    _prim(P[n + 1], SPHERE, -1.0, 1.0, 20.0, 1e-15, 0.5, 0.5, 0.5, 0.3, 0.0, 1.0, 1.0, 0.5, False)
    out.append(("inf_and_tiny_radius", P, n + 2, 200, 150))
    return out


# ---------------------------------------------------------------- queue tracer
QUEUE_W, QUEUE_H = 96, 72


@functools.lru_cache(maxsize=None)
def queue_lit(seed, w=QUEUE_W, h=QUEUE_H):
    """(prims, n, frame, counters): test_oracle_queue.random_scene's closed
    room (oracle_lib.queue_random_scene: random spheres, some around the
    camera, extra random planes) from that function's own stream for `seed`,
    re-drawn until the oracle counts no undefined behaviour in a w x h frame
    AND the frame meets the conditions (where random_scene's own draw is lit,
    this is that scene).
    The oracle's frame and counters come along, read-only."""
    rng = np.random.default_rng(1000 + seed)                # test_oracle_queue.random_scene's stream
    while True:
        P, n = O.queue_random_scene(rng, nspheres=int(rng.integers(2, 40)), nlights=int(rng.integers(1, 5)),
                                    nplanes_extra=int(rng.integers(0, 3)))
        frame, cnt = O.queue_render(w, h, P, n, nthreads=NT)
        lit, distinct = lit_stats(frame)
        if cnt[3] == 0 and lit >= MIN_LIT and distinct >= MIN_DISTINCT:
            frame.setflags(write=False)
            return P, n, frame, cnt


def queue_features(P, n):
    eye = [p for p in P[:n] if p.type == 1 and not p.is_light and
           np.linalg.norm([p.center.x - CAMERA[0], p.center.y - CAMERA[1], p.center.z - CAMERA[2]]) < p.radius]
    return {"camera_inside": bool(eye), "extra_planes": sum(p.type == 0 for p in P[:n]) > 6,
            "glass": any(p.type == 1 and p.m_refr > 0 for p in P[:n])}


# ---------------------------------------------------------------- smallpt
def smallpt_room(seed):
    """(spheres, n, camera, w, h, steps): Cornell's six wall spheres with
    random colours (some walls mirrors), 1-3 emitters and 2-29 diffuse /
    mirror / glass spheres inside the room, in shuffled order; the camera
    inside the room looks at a random interior point.  Frame sizes and the
    two progressive pass sizes as in
    test_gpu_smallpt.test_random_scenes_vs_oracle; the tests run every room
    under both estimators."""
    rng = np.random.default_rng(seed)
    walls, _ = rtamd.scenes.cornell()
    rows = []
    for s in walls[:6]:
        rows.append((s.rad, (s.p.x, s.p.y, s.p.z), (0.0, 0.0, 0.0), tuple(rng.uniform(0.2, 0.9, 3)),
                     SPEC if rng.random() < 0.25 else DIFF))
    lo, hi = np.array([1.0, 0.0, 0.0]), np.array([99.0, 81.6, 170.0])   # the room in front of the camera
    for _ in range(int(rng.integers(1, 4))):
        r = float(rng.uniform(3, 8))
        c = rng.uniform(lo + r, hi - r)
        c[1] = rng.uniform(45, 81.6 - r)                                # emitters in the upper half
        rows.append((r, tuple(c), tuple(rng.uniform(4, 15, 3)), (0.0, 0.0, 0.0), DIFF))
    for _ in range(int(rng.integers(2, 30))):
        r = float(rng.uniform(2, 14))
        rows.append((r, tuple(rng.uniform(lo + r, hi - r)), (0.0, 0.0, 0.0), tuple(rng.uniform(0.1, 0.95, 3)),
                     int(rng.choice([DIFF, DIFF, SPEC, REFR]))))
    order = rng.permutation(len(rows))
    S = (rtamd.Sphere * len(rows))()
    for k, j in enumerate(order):
        _sphere(S[k], *rows[j])
    w, h = int(rng.integers(24, 90)), int(rng.integers(16, 70))
    cam = rtamd.Camera()
    cam.orig = rtamd.Vec3(*map(float, rng.uniform([10, 10, 175], [90, 70, 260])))
    cam.target = rtamd.Vec3(*map(float, rng.uniform([20, 10, 20], [80, 70, 120])))
    rtamd.scenes.update_camera(cam, w, h)
    steps = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
    return S, len(rows), cam, w, h, steps


def smallpt_unconstrained(seed):
    """(spheres, n, camera, w, h, steps) of
    test_gpu_smallpt.test_random_scenes_vs_oracle's seed (11-16), draw for
    draw (that test runs estimator seed % 2); restated here for the CPU pins,
    that GPU test keeps its own copy."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(3, 40))
    S = (rtamd.Sphere * n)()
    for i in range(n):
        big = rng.random() < 0.2
        rad = float(10 ** rng.uniform(2, 4)) if big else float(10 ** rng.uniform(-1.5, 1.2))
        c = rng.uniform(-60, 60, 3)
        if big:
            ax = int(rng.integers(0, 3))
            c[ax] = np.sign(rng.standard_normal()) * (rad + rng.uniform(20, 80))
        light = rng.random() < 0.15 or i == 0
        e = tuple(rng.uniform(1, 15, 3)) if light else (0.0, 0.0, 0.0)
        refl = int(rng.choice([0, 0, 0, 1, 2]))
        _sphere(S[i], rad, tuple(c), e, tuple(rng.uniform(0.1, 0.95, 3)), refl)
    w, h = int(rng.integers(24, 90)), int(rng.integers(16, 70))
    cam = rtamd.Camera()
    cam.orig = rtamd.Vec3(*map(float, rng.uniform(-20, 20, 3)))
    cam.target = rtamd.Vec3(*map(float, rng.uniform(-20, 20, 3)))
    rtamd.scenes.update_camera(cam, w, h)
    steps = (int(rng.integers(1, 4)), int(rng.integers(1, 4)))
    return S, n, cam, w, h, steps


@functools.lru_cache(maxsize=None)
def room_oracle(seed, mode):
    """smallpt_room(seed) and the oracle's frame after its passes under
    estimator `mode` (spt_check.oracle_frame: colours, seeds, pixels,
    counters), computed once: (spheres, n, camera, w, h, steps, frame)."""
    S, n, cam, w, h, steps = smallpt_room(seed)
    ref = oracle_frame(O, w, h, list(steps), mode=mode, scene=(S, n), cam=cam, nthreads=NT)
    return S, n, cam, w, h, steps, ref
