"""Reference for rtp_query_async (include/rt_hip.h "level-pass tracers, ray
queries"): the public contract on top of tests/prims_ref.py's loops over the
oracle's per-primitive intersects -- the miss values made the same for both
tracers, the d_tmax filter on the nearest hit, and the shadow loop's position
in the occluder order mapped back to a primitive index.  Pinned on the CPU by
tests/test_prims_query_ref.py (the filter equals the oracle's loop started at
the bound), used by tests/test_gpu_prims_query.py.  TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C

import numpy as np

import prims_ref as R

F = np.float32
KINDS = ("nearest", "shadow", "occluder")
FAR = {t: R.TRAITS[t][0] for t in R.TRAITS}


def scene_of(prims, n, tracer):
    """prims_ref.Scene of a Primitive (tracer "whitted") or QPrimitive
    ("queue") array, by each tracer's own rules: Whitted SPHERE 1 / PLANE 2,
    light m_Light > 0, occluder m_Light == 0 (raytracer.cpp:100); queue tracer
    PLANE 0 / SPHERE 1, light is_light, occluder !is_light
    (raytracer_non_OpenCL.c:232)."""
    out = []
    for i in range(n):
        q = prims[i]
        if tracer == "whitted":
            kind = {1: "s", 2: "p"}.get(q.type, "o")
            geo = ((q.m_Centre.x, q.m_Centre.y, q.m_Centre.z, q.m_SqRadius) if kind == "s" else
                   (q.plane_N.x, q.plane_N.y, q.plane_N.z, q.plane_D) if kind == "p" else (0.0, 0.0, 0.0, 0.0))
            out.append((kind, geo, q.m_Light > 0, q.m_Light == 0))
        else:
            kind = {0: "p", 1: "s"}.get(q.type, "o")
            geo = ((q.center.x, q.center.y, q.center.z, q.sq_radius) if kind == "s" else
                   (q.normal.x, q.normal.y, q.normal.z, q.depth) if kind == "p" else (0.0, 0.0, 0.0, 0.0))
            out.append((kind, geo, bool(q.is_light), not q.is_light))
    return R.Scene(out)


def rays_of(rays):
    return np.ascontiguousarray(rays, dtype=F).reshape(-1, 6)


def query(scene, rays, tracer, kind, tmax=None):
    """rtp_query_async's answer.  "nearest": (t float32, id int32, result
    int32); "shadow" / "occluder": id int32."""
    rays = rays_of(rays)
    far, result0, miss = R.TRAITS[tracer]
    if kind == "nearest":
        dist, prim, result = R.nearest(scene, rays, tracer)
        hit = prim != miss
        if tmax is not None:
            with np.errstate(invalid="ignore"):
                hit &= dist < np.asarray(tmax, F)          # strictly; NaN accepts nothing
        return (np.where(hit, dist, far).astype(F), np.where(hit, prim, -1).astype(np.int32),
                np.where(hit, result, 0).astype(np.int32))
    first = R.first_occluder(scene, rays, np.asarray(tmax, F), tracer)
    found = first != R.NONE
    if kind == "shadow":
        return found.astype(np.int32)
    assert kind == "occluder"
    ids = np.append(np.flatnonzero(scene.occluder), -1)   # position -> primitive index
    return np.where(found, ids[np.where(found, first, -1)], -1).astype(np.int32)


def loop_from(scene, rays, bounds, tracer):
    """The oracle's nearest-hit loop STARTED AT bounds[i] instead of far:
    d.value = B, then orw_ / orq_primitive_intersect in index order.  (dist,
    prim or -1, result or 0) -- what query(..., "nearest", tmax=B) claims to
    equal for B <= far."""
    P, f = scene.prims(tracer), R._intersect(tracer)
    P = [P[s] for s in range(scene.n)]
    rays, base = R._rays(rays)
    bounds = np.asarray(bounds, F)
    n = len(rays)
    dist, prim, result = np.empty(n, F), np.full(n, -1, np.int32), np.zeros(n, np.int32)
    d = C.c_float()
    for i in range(n):
        d.value = bounds[i]
        for s in range(scene.n):
            res = f(P[s], base + 24 * i, d)
            if res:
                prim[i], result[i] = s, res
        dist[i] = d.value
    return dist, prim, result


# ------------------------------------------------------------------ inputs
def directions(rng, m):
    v = rng.normal(size=(m, 3)).astype(F)
    return v * (F(1) / np.sqrt((v * v).sum(1, dtype=F)))[:, None]


def fan(origin, m, rng):
    """m rays from one origin."""
    return np.concatenate([np.tile(np.asarray(origin, F), (m, 1)), directions(rng, m)], 1)


def random_rays(rng, m, lo, hi):
    return np.concatenate([rng.uniform(lo, hi, (m, 3)).astype(F), directions(rng, m)], 1)


def sphere_centres(scene):
    return [tuple(scene.geo[i][:3]) for i in range(scene.n) if scene.kind[i] == "s"]


def ray_set(scene, m, seed):
    """Rays that miss (escapes), fans from a camera-like point and from inside
    every sphere (result -1), and random rays through the scene's box: m rays
    (more when m is too small for a few of each)."""
    rng = np.random.default_rng(seed)
    cs = sphere_centres(scene)
    per = max(4, m // (4 * max(len(cs), 1)))
    parts = [escapes(), fan((0.0, 0.25, -7.0), m // 4, rng)] + [fan(c, per, rng) for c in cs]
    parts.append(random_rays(rng, max(m - sum(len(p) for p in parts), 8), (-9, -6, -8), (9, 8, 30)))
    return np.concatenate(parts).astype(F)


def escapes():
    """Misses even in a closed room: along each axis, a ray leaving from 1000
    out (parallel to four walls, moving away from the other two) and a ray
    coming in from 3e7 out (whatever it meets is beyond both tracers' far)."""
    out = []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            e = np.zeros(3, F)
            e[axis] = sign
            out.append(np.concatenate([e * F(1000), e]))
            out.append(np.concatenate([e * F(3e7), -e]))
    return np.array(out, F)


def shadow_lengths(scene, rays, tracer, seed):
    """Lengths around the true occluder distances: for a ray whose nearest
    occluder is at c, one of c itself, the floats beside it, a fraction and a
    multiple of it; else a random length."""
    rng = np.random.default_rng(seed)
    occ = R.Scene([(scene.kind[i], tuple(scene.geo[i]), False, True) if scene.occluder[i] else R.other(light=True)
                   for i in range(scene.n)])
    dist, prim, _ = R.nearest(occ, rays, tracer)
    n = len(dist)
    choice = rng.integers(0, 6, n)
    lens = rng.uniform(0.5, 40.0, n).astype(F)
    hit = prim != R.TRAITS[tracer][2]
    with np.errstate(all="ignore"):
        alt = [dist, np.nextafter(dist, F(np.inf)), np.nextafter(dist, F(-np.inf)), dist * F(0.5), dist * F(3)]
    for k, a in enumerate(alt):
        m = hit & (choice == k)
        lens[m] = a[m]
    return lens


def big_scene(tracer, seed=64):
    """64 random primitives: spheres, planes, lights of both kinds and, for
    Whitted, a few that are neither light nor occluder."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(R.MAXP):
        light = rng.random() < 0.15
        occluder = None if tracer == "queue" or light or rng.random() < 0.9 else False
        if rng.random() < 0.6:
            out.append(R.sphere(rng.uniform(-9, 9, 3), rng.uniform(0.1, 9.0), light=light, occluder=occluder))
        else:
            v = rng.normal(size=3)
            out.append(R.plane(v / np.linalg.norm(v), rng.uniform(-10, 10), light=light, occluder=occluder))
    return R.Scene(out)
