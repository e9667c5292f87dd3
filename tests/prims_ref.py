"""Reference for rt_prims.h's loops (nearest_n, first_occluder, light_len_inv,
fill_lists), built on the oracle's own per-primitive intersects
(orw_primitive_intersect, orq_primitive_intersect): the references' loops in
index order, nothing else.  Pinned on the CPU by tests/test_prims_ref.py, used
by tests/test_gpu_prims.py.  TEST INFRASTRUCTURE ONLY.
"""
import ctypes as C

import numpy as np

import oracle_lib as O

MAXP = 64
NONE = 0x7fffffff

# (far, result0, miss): whitted.hip / queue.hip NearestTraits, i.e.
# whitted_oracle.c:155-161 and queue_oracle.c:101-106.
TRAITS = {
    "whitted": (np.float32(1000000.0), 0, 0x7fffffff),
    "queue": (np.float32(10000000.0), 1, -1),
}


def sphere(c, sq_radius, light=False, occluder=None):
    return ("s", (c[0], c[1], c[2], sq_radius), light, (not light) if occluder is None else occluder)


def plane(N, D, light=False, occluder=None):
    return ("p", (N[0], N[1], N[2], D), light, (not light) if occluder is None else occluder)


def other(light=False, occluder=None):
    """Neither sphere nor plane (Whitted's BOX): counted in n, in no list."""
    return ("o", (0.0, 0.0, 0.0, 0.0), light, (not light) if occluder is None else occluder)


class Scene:
    """<= 64 primitives: kind 's' / 'p' / 'o', geometry (centre.xyz, squared
    radius | normal.xyz, D), light flag, occluder flag.  A primitive that is
    neither light nor occluder is Whitted's m_Light < 0; the queue tracer has
    none (its occluders are its non-lights)."""

    def __init__(self, prims):
        assert 1 <= len(prims) <= MAXP
        self.n = len(prims)
        self.kind = [p[0] for p in prims]
        self.geo = np.array([p[1] for p in prims], dtype=np.float32).reshape(self.n, 4)
        self.light = np.array([bool(p[2]) for p in prims])
        self.occluder = np.array([bool(p[3]) for p in prims])
        assert not (self.light & self.occluder).any()
        self._prims = {}

    def flags(self):
        """The harness' MAXP-long inputs: valid, is_sphere, is_plane, is_light,
        is_occluder (int32), sphere geometry, plane geometry (float32 x 4)."""
        def pad(a):
            out = np.zeros(MAXP, np.int32)
            out[:self.n] = a
            return out
        geo = np.zeros((MAXP, 4), np.float32)
        geo[:self.n] = self.geo
        k = np.array(self.kind)
        return (pad(1), pad(k == "s"), pad(k == "p"), pad(self.light), pad(self.occluder), geo, geo.copy())

    def prims(self, traits):
        """The oracle's primitive array for this scene."""
        if traits in self._prims:
            return self._prims[traits]
        if traits == "whitted":
            P = (O.Primitive * MAXP)()
            for i in range(self.n):
                x, y, z, w = (float(v) for v in self.geo[i])
                p = P[i]
                p.type = {"s": 1, "p": 2, "o": 3}[self.kind[i]]
                p.m_Light = 1 if self.light[i] else (0 if self.occluder[i] else -1)
                if self.kind[i] == "s":
                    p.m_Centre, p.m_SqRadius = O.V3(x, y, z), w
                elif self.kind[i] == "p":
                    p.plane_N, p.plane_D = O.V3(x, y, z), w
        else:
            assert (self.light != self.occluder).all(), "the queue tracer's occluders are its non-lights"
            P = (O.QPrimitive * MAXP)()
            for i in range(self.n):
                x, y, z, w = (float(v) for v in self.geo[i])
                p = P[i]
                p.type = {"p": 0, "s": 1, "o": 2}[self.kind[i]]
                p.is_light = 1 if self.light[i] else 0
                if self.kind[i] == "s":
                    p.center, p.sq_radius = O.F4(x, y, z, 0.0), w
                elif self.kind[i] == "p":
                    p.normal, p.depth = O.F4(x, y, z, 0.0), w
        self._prims[traits] = P
        return P


def _intersect(traits):
    L = O.lib()
    return L.orw_primitive_intersect if traits == "whitted" else L.orq_primitive_intersect


def _rays(rays):
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    return rays, rays.ctypes.data


def candidate(scene, s, ray, traits):
    """Primitive s alone against one ray, with no distance to beat: (the
    intersect's return, its distance or +inf)."""
    ray, base = _rays(ray)
    d = C.c_float(np.inf)
    res = _intersect(traits)(scene.prims(traits)[s], base, d)
    return res, np.float32(d.value)


def nearest(scene, rays, traits):
    """The references' nearest-hit loop: (dist float32[n], prim int32[n],
    result int32[n]); prim = the traits' miss and result = result0 on a miss."""
    far, result0, miss = TRAITS[traits]
    P, f = scene.prims(traits), _intersect(traits)
    P = [P[s] for s in range(scene.n)]
    rays, base = _rays(rays)
    n = len(rays)
    dist, prim, result = np.empty(n, np.float32), np.empty(n, np.int32), np.empty(n, np.int32)
    d = C.c_float()
    for i in range(n):
        d.value = far
        p, r = miss, result0
        ray = base + 24 * i
        for s in range(scene.n):
            res = f(P[s], ray, d)
            if res:
                p, r = s, res
        dist[i], prim[i], result[i] = d.value, p, r
    return dist, prim, result


def first_occluder(scene, rays, lens, traits):
    """The references' shadow loop: the position, in the occluder (non-light)
    order, of the first occluder nearer than lens[i]; 0x7fffffff when none."""
    P, f = scene.prims(traits), _intersect(traits)
    rays, base = _rays(rays)
    lens = np.asarray(lens, dtype=np.float32)
    occ = [P[s] for s in range(scene.n) if scene.occluder[s]]
    out = np.full(len(rays), NONE, np.int32)
    d = C.c_float()
    for i in range(len(rays)):
        ray = base + 24 * i
        for pos, p in enumerate(occ):
            d.value = lens[i]
            if f(p, ray, d):
                out[i] = pos
                break
    return out


def light_len_inv(d2):
    """sqrtf(d2) and 1.0f / it, in float32."""
    d2 = np.asarray(d2, dtype=np.float32)
    with np.errstate(all="ignore"):
        length = np.sqrt(d2)
        inv = np.float32(1.0) / length
    return length, inv


def lists(scene):
    """fill_lists' result, constructed plainly: a dict of the PrimLists
    fields (lists cut to their counts) and the per-primitive light rank."""
    k = np.array(scene.kind)
    sph, pln = np.flatnonzero(k == "s"), np.flatnonzero(k == "p")
    occ_rank = np.cumsum(scene.occluder) - scene.occluder       # occluders before this one
    osph = np.array([i for i in sph if scene.occluder[i]], dtype=np.int64)
    opln = np.array([i for i in pln if scene.occluder[i]], dtype=np.int64)
    rank = np.zeros(MAXP, np.int32)
    rank[:scene.n] = np.cumsum(scene.light) - scene.light
    rank[scene.n:] = scene.light.sum()
    return {
        "sph": scene.geo[sph], "pln": scene.geo[pln], "sph_id": sph.astype(np.int32), "pln_id": pln.astype(np.int32),
        "osph": scene.geo[osph], "opln": scene.geo[opln],
        "osph_pos": occ_rank[osph].astype(np.int32), "opln_pos": occ_rank[opln].astype(np.int32),
        "n": scene.n, "ns": len(sph), "np": len(pln), "nos": len(osph), "nop": len(opln),
        "nlights": int(scene.light.sum()), "nnonlight": int(scene.occluder.sum()),
    }, rank
