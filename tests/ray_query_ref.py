"""Expected values of the ray queries (spt_scene_query_async) and the rays the
tests and tools/ray_query_time.py send.  A plain helper module.

The expected values are a numpy float32 restatement of the reference's
SphereIntersect, Intersect and IntersectP (smallptgpu-v1.6/geomfunc.h:32-110):
one float32 operation per numpy call, in the reference's order, so nothing is
fused; chunked over spheres so a 56,000-sphere scene needs no large array.
Results are compared with the device's as bits (t) and integers (id)."""
import numpy as np

import rtamd
import scenes_layouts as sl

f32 = np.float32
EPS = f32(0.01)                 # geom.h:29
INF = f32(np.inf)
KINDS = ("nearest", "any", "occluder")


def geometry(S, n):
    """(centres float32 [n, 3], radii float32 [n]) of a Sphere array."""
    rows = sl.rows_of(S, n)
    return np.ascontiguousarray(rows[:, 1:4]), np.ascontiguousarray(rows[:, 0])


def distances(p, rad, rays):
    """SphereIntersect (geomfunc.h:32-59) of every ray with every sphere of the
    chunk: float32 [rays, spheres], 0 where the reference returns 0."""
    with np.errstate(all="ignore"):
        o, d = rays[:, None, 0:3], rays[:, None, 3:6]
        opx = p[None, :, 0] - o[..., 0]                     # vsub(op, s->p, r->o)
        opy = p[None, :, 1] - o[..., 1]
        opz = p[None, :, 2] - o[..., 2]
        b = opx * d[..., 0]                                 # vdot(op, r->d)
        b = b + opy * d[..., 1]
        b = b + opz * d[..., 2]
        oo = opx * opx                                      # vdot(op, op)
        oo = oo + opy * opy
        oo = oo + opz * opz
        det = b * b
        det = det - oo
        det = det + (rad * rad)[None, :]
        neg = det < 0
        sd = np.sqrt(det)                                   # correctly rounded
        t1 = b - sd
        t2 = b + sd
        dist = np.where(t1 > EPS, t1, np.where(t2 > EPS, t2, f32(0)))
        dist = np.where(neg, f32(0), dist)
    assert dist.dtype == f32
    return dist


def scan(S, n, rays, tmax=None, chunk=512):
    """All three kinds in one pass over the spheres: {"nearest": (t, id),
    "any": id, "occluder": id}.  tmax None: the bound 1e20f of Intersect."""
    p, rad = geometry(S, n)
    rays = np.ascontiguousarray(rays, dtype=f32)
    nr = len(rays)
    bound = np.full(nr, f32(1e20), f32) if tmax is None else np.ascontiguousarray(tmax, dtype=f32)
    best = np.full(nr, INF, f32)
    best_id = np.full(nr, -1, np.int32)
    high = np.full(nr, -1, np.int32)
    rows = np.arange(nr)
    for lo in range(0, n, chunk):
        dist = distances(p[lo:lo + chunk], rad[lo:lo + chunk], rays)
        with np.errstate(invalid="ignore"):
            acc = (dist != 0) & (dist < bound[:, None])         # d != 0.f && d < *t (or maxt)
        cs = dist.shape[1]
        dm = np.where(acc, dist, INF)
        last = cs - 1 - np.argmin(dm[:, ::-1], axis=1)          # the minimum's highest index in the chunk
        m = dm[rows, last]
        some = acc.any(axis=1)
        take = some & (m <= best)                               # later chunks hold higher indices: ties go to them
        best = np.where(take, m, best)
        best_id = np.where(take, lo + last, best_id).astype(np.int32)
        top = cs - 1 - np.argmax(acc[:, ::-1], axis=1)
        high = np.where(some, lo + top, high).astype(np.int32)
    hit = best_id >= 0
    t = np.where(hit, best.view(np.uint32), bound.view(np.uint32)).astype(np.uint32).view(f32)
    return {"nearest": (t, best_id), "any": (high >= 0).astype(np.int32), "occluder": high}


# ---- rays
def _unit(rng, k):
    d = rng.normal(0, 1, (k, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def scene_box(p, rad):
    """The box of the scene's ordinary spheres (walls and grounds left out)."""
    small = rad < 100 * np.median(rad)
    if not small.any():
        small[:] = True
    lo = (p[small] - rad[small, None]).min(axis=0).astype(np.float64)
    hi = (p[small] + rad[small, None]).max(axis=0).astype(np.float64)
    return lo, hi


def random_rays(S, n, count, seed=1):
    """`count` rays with origins uniform in the scene's box and uniform unit
    directions (normalised in double, rounded to float32): float32 [count, 6]."""
    p, rad = geometry(S, n)
    lo, hi = scene_box(p, rad)
    rng = np.random.default_rng([seed, 100])
    return np.concatenate([rng.uniform(lo, hi, (count, 3)), _unit(rng, count)], axis=1).astype(f32)


def ray_set(S, n, cam, count, seed=1, aim=()):
    """(rays float32 [count, 6], tmax float32 [count]): the mix the GPU tests
    send -- camera rays, random rays, light-directed rays with tmax = distance
    - EPS, origins exactly on sphere surfaces, the constructed det == 0
    tangent, axis-aligned directions, |d| = 2 and |d|^2 = 1 + 2^-10, d = 0 from
    inside a sphere, tmax in {-1, 0, EPS, +inf, NaN}, non-finite rays, and rays
    aimed at the centres in `aim`.  count >= 1024."""
    assert count >= 1024
    p, rad = geometry(S, n)
    rows = sl.rows_of(S, n)
    lo, hi = scene_box(p, rad)
    ext = float((hi - lo).max())
    rng = np.random.default_rng([seed, n])
    p64, r64 = p.astype(np.float64), rad.astype(np.float64)
    small = np.flatnonzero(rad < 100 * np.median(rad))
    rays, tmax = [], []

    def add(o, d, tm):
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        rays.append(np.concatenate([o, d], axis=1).astype(f32))
        tmax.append(np.broadcast_to(np.asarray(tm, f32), (len(o),)).astype(f32))

    def origins(k):
        return rng.uniform(lo, hi, (k, 3))

    # camera rays: a 16 x 8 grid of pixel centres
    cr = rtamd.scenes.camera_rays(cam(16, 8), 16, 8)
    add(cr[:, :3], cr[:, 3:], f32(1e20))
    # towards the lights, tmax = distance - EPS (the path tracer's shadow rays, roughly)
    lights = np.flatnonzero((rows[:, 4] != 0) | (rows[:, 6] != 0))
    k = count // 8
    o = origins(k)
    li = lights[rng.integers(0, len(lights), k)]
    v = p64[li] - o
    dist = np.linalg.norm(v, axis=1)
    add(o, v / dist[:, None], dist.astype(f32) - EPS)
    # origins exactly on (the float32 rounding of) sphere surfaces
    k = count // 8
    si = small[rng.integers(0, len(small), k)]
    add(p64[si] + r64[si, None] * _unit(rng, k), _unit(rng, k), rng.uniform(0.05 * ext, ext, k))
    # det == 0: op = (r, 0, 0), d = (0, +-1, 0) or (0, 0, 1); b = 0 and det = -r*r + r*r
    k = 48
    si = small[rng.integers(0, len(small), 4 * k)]
    ox = (p[si, 0] - rad[si]).astype(f32)
    si = si[(p[si, 0] - ox) == rad[si]][:k]                   # op.x is the radius exactly
    o = p64[si].copy()
    o[:, 0] = (p[si, 0] - rad[si]).astype(f32)
    d = np.zeros((len(si), 3))
    d[np.arange(len(si)), 1 + (np.arange(len(si)) % 2)] = np.where(np.arange(len(si)) % 3 == 0, -1.0, 1.0)
    add(o, d, f32(1e20))
    # axis-aligned directions, and directions with one zero component
    k = count // 16
    d = np.zeros((k, 3))
    d[np.arange(k), rng.integers(0, 3, k)] = rng.choice([-1.0, 1.0], k)
    add(origins(k), d, np.where(rng.random(k) < 0.5, f32(1e20), rng.uniform(0.05 * ext, ext, k)))
    d = _unit(rng, k)
    d[np.arange(k), rng.integers(0, 3, k)] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    add(origins(k), d, f32(1e20))
    # unnormalised: |d| = 2 (exact doubling of a float32 unit vector), |d|^2 = 1 + 2^-10
    k = count // 16
    add(origins(k), 2.0 * _unit(rng, k).astype(f32), rng.uniform(0.05 * ext, ext, k))
    add(origins(k), np.sqrt(1.0 + 2.0 ** -10) * _unit(rng, k), f32(1e20))
    # d = 0 from inside a sphere: b = 0, det = r*r - |op|^2 > 0, the far root is sqrt(det)
    k = 32
    si = small[rng.integers(0, len(small), k)]
    add(p64[si] + 0.3 * r64[si, None] * _unit(rng, k), np.zeros((k, 3)), f32(1e20))
    # bounds that accept nothing, or everything
    for tm in (-1.0, 0.0, float(EPS), np.inf, np.nan):
        add(origins(16), _unit(rng, 16), f32(tm))
    # non-finite rays
    k = 64
    o, d = origins(k), _unit(rng, k)
    od = np.concatenate([o, d], axis=1)
    od[np.arange(k), rng.integers(0, 6, k)] = rng.choice([np.inf, -np.inf, np.nan], k)
    od[: k // 4, 3] = rng.choice([np.inf, np.nan], k // 4)
    add(od[:, :3], od[:, 3:], f32(1e20))
    # aimed at given centres from outside
    for c in aim:
        k = count // 8
        o = np.asarray(c, np.float64) + rng.uniform(2.0, 6.0, (k, 1)) * _unit(rng, k)
        v = np.asarray(c, np.float64) + rng.normal(0, 0.2, (k, 3)) - o
        add(o, v / np.linalg.norm(v, axis=1, keepdims=True), f32(1e20))
    # the rest: random rays, half of them with a finite reach
    have = sum(len(r) for r in rays)
    assert have <= count, (have, count)
    k = count - have
    rr = random_rays(S, n, k, seed)
    add(rr[:, :3], rr[:, 3:], np.where(rng.random(k) < 0.5, f32(1e20), rng.uniform(0.02 * ext, ext, k)))
    rays, tmax = np.concatenate(rays), np.concatenate(tmax)
    assert rays.shape == (count, 6) and tmax.shape == (count,)
    return np.ascontiguousarray(rays), np.ascontiguousarray(tmax)


def non_finite_rays(S, n, count, seed=1):
    """`count` rays, each with one to three components replaced by +inf, -inf
    or NaN (the others: random_rays)."""
    rays = random_rays(S, n, count, seed).copy()
    rng = np.random.default_rng([seed, 200])
    for _ in range(3):
        on = rng.random(count) < (1.0 if _ == 0 else 0.3)
        col = rng.integers(0, 6, count)
        val = rng.choice(np.array([np.inf, -np.inf, np.nan], f32), count)
        rays[np.flatnonzero(on), col[on]] = val[on]
    assert (~np.isfinite(rays)).any(axis=1).all()
    return rays
