"""GPU parity of the level-pass tracers' ray queries (rtp_query_async,
csrc/prims_query.hip) through the public surface (rtamd.PrimScene and the
C entry point), bit for bit against tests/prims_query_ref.py (the references'
loops over the oracle's per-primitive intersects): both tracers' reference
scenes and synthetic ones, the three kinds, NEAREST with one and with two rays
per lane, batch sizes around the wave and chunk sizes with the grid capped,
guard words, the edges tests/test_gpu_prims.py found or guards (far, ties,
discriminants outside sqrt_nr's range beside ordinary lanes and lanes past
nrays, plane edges, NaN / inf), bounds, a set followed by a query on one
stream, and a captured graph."""
import contextlib
import functools
import os

import numpy as np
import pytest

import prims_query_ref as Q
import prims_ref as R
import test_gpu_prims as TP      # its case builders (far_case, TIES, room, ...), not its checks

pytestmark = pytest.mark.gpu
F = np.float32
TRACERS = ["whitted", "queue"]
INF, NAN = F(np.inf), F(np.nan)
GUARD = 8                        # words past the end of every output
FILL_F, FILL_I = -777.25, -777
KIND_ID = {"nearest": 0, "shadow": 1, "occluder": 2}


@contextlib.contextmanager
def env(**kv):
    """RT_PRIMS_QUERY_BLOCKS / RT_PRIMS_QUERY_RAYS, both read at the call."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared references are read-only)


def prim_bytes(P, n):
    """The first n primitives of a ctypes array as a uint8 device tensor."""
    import ctypes as C
    size = C.sizeof(P._type_)
    return dev(np.frombuffer(P, dtype=np.uint8, count=size * n).copy())


def prepared(rt, scene, tracer, prims=None):
    return rt.PrimScene(scene.prims(tracer) if prims is None else prims, scene.n, tracer=tracer)


def gpu(rt, ps, rays, kind, tmax=None, want=(True, True, True)):
    """One rtp_query_async through the C entry point with every output the
    kind does not write, or that `want` leaves out, still passed where the
    contract lets it be (t and result for the shadow kinds) or withheld
    (NEAREST): returns (t bits, id, result) as numpy, None where not written.
    Asserts the guard words and the unwritten outputs are untouched."""
    import torch
    rays = Q.rays_of(rays)
    n = len(rays)
    d_rays = dev(rays)
    d_tmax = None if tmax is None else dev(np.asarray(tmax, F))
    t = torch.full((n + GUARD,), FILL_F, dtype=torch.float32, device="cuda")
    ids = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device="cuda")
    res = torch.full((n + GUARD,), FILL_I, dtype=torch.int32, device="cuda")
    nearest = kind == "nearest"
    give = [x.data_ptr() if (w or not nearest) else None for x, w in zip((t, ids, res), want)]
    rt.check(rt.entry("rtp_query_async")(ps.handle, d_rays.data_ptr(), None if d_tmax is None else d_tmax.data_ptr(), n,
                                         KIND_ID[kind], give[0], give[1], give[2],
                                         torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    t, ids, res = t.cpu().numpy(), ids.cpu().numpy(), res.cpu().numpy()
    assert (t[n:] == F(FILL_F)).all() and (ids[n:] == FILL_I).all() and (res[n:] == FILL_I).all(), "guard words"
    written = want if nearest else (False, True, False)
    for a, w, fill in ((t, written[0], F(FILL_F)), (ids, written[1], FILL_I), (res, written[2], FILL_I)):
        assert w or (a == fill).all(), "an output the call must not write was written"
    return (t[:n].view(np.uint32) if written[0] else None, ids[:n] if written[1] else None,
            res[:n] if written[2] else None)


def agree(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r, reference %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def check_nearest(rt, ps, scene, tracer, rays, tmax=None, ref=None, lanes=(1, 2)):
    """NEAREST with one and with two rays per lane against the reference;
    returns the answer (t float32, id, result)."""
    ref = Q.query(scene, rays, tracer, "nearest", tmax=tmax) if ref is None else ref
    for k in lanes:
        with env(RT_PRIMS_QUERY_RAYS=k):
            t, ids, res = gpu(rt, ps, rays, "nearest", tmax)
        tag = "%s nearest, %d per lane: " % (tracer, k)
        agree(tag + "id", ids, ref[1])
        agree(tag + "t bits", t, ref[0].view(np.uint32))
        agree(tag + "result", res, ref[2])
    return ref


def check_shadow(rt, ps, scene, tracer, rays, lens, ref=None):
    """OCCLUDER against the reference's break position, SHADOW against
    "found one", and SHADOW == (OCCLUDER != -1) on every ray."""
    ref = Q.query(scene, rays, tracer, "occluder", tmax=lens) if ref is None else ref
    occ = gpu(rt, ps, rays, "occluder", lens)[1]
    sh = gpu(rt, ps, rays, "shadow", lens)[1]
    agree(tracer + " occluder", occ, ref)
    agree(tracer + " shadow", sh, (ref != -1).astype(np.int32))
    agree(tracer + " shadow vs occluder", sh == 1, occ != -1)
    return occ


def check_all(rt, scene, tracer, rays, lens, prims=None):
    ps = prepared(rt, scene, tracer, prims)
    try:
        near = check_nearest(rt, ps, scene, tracer, rays)
        occ = check_shadow(rt, ps, scene, tracer, rays, lens)
    finally:
        ps.close()
    return near, occ


# ------------------------------------------------------------------ the reference scenes
@functools.lru_cache(maxsize=None)
def reference(tracer):
    """The tracer's reference scene as the product hands it out, 4096 + 17
    rays (fans, from inside every sphere, random, escaping), shadow lengths
    around the true occluder distances, and the three kinds' answers."""
    import rtamd
    P, n = rtamd.scenes.whitted_scene() if tracer == "whitted" else rtamd.scenes.queue_scene()
    scene = Q.scene_of(P, n, tracer)
    rays = Q.ray_set(scene, 4096 + 17, 2026)[:4096 + 17]
    assert len(rays) == 4096 + 17
    lens = Q.shadow_lengths(scene, rays, tracer, 16)
    near = Q.query(scene, rays, tracer, "nearest")
    occ = Q.query(scene, rays, tracer, "occluder", tmax=lens)
    assert (near[2] == -1).sum() > 100 and (near[1] == -1).any() and (occ == -1).sum() > 100 and (occ != -1).sum() > 100
    for a in (rays, lens, occ) + near:
        a.setflags(write=False)
    return P, n, scene, rays, lens, near, occ


@pytest.mark.parametrize("tracer", TRACERS)
def test_reference_scene(rt, tracer):
    """The three kinds on the tracer's own 17 primitives (the array the frames
    are rendered from), and NEAREST under random bounds around the hits."""
    P, n, scene, rays, lens, near, occ = reference(tracer)
    ps = rt.PrimScene(P, n, tracer=tracer)
    try:
        check_nearest(rt, ps, scene, tracer, rays, ref=near)
        check_shadow(rt, ps, scene, tracer, rays, lens, ref=occ)
        rng = np.random.default_rng(4)
        bounds = (near[0] * rng.uniform(0.5, 1.5, len(rays)).astype(F)).astype(F)
        got = check_nearest(rt, ps, scene, tracer, rays, tmax=bounds)
        assert 0 < (got[1] >= 0).sum() < (near[1] >= 0).sum()
    finally:
        ps.close()


# ------------------------------------------------------------------ batch edges
@pytest.mark.parametrize("blocks", [None, 1, 2])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 4096 + 17])
def test_batch_edges(rt, n, blocks):
    """Sizes around the wave (64 rays) and the two-per-lane chunk (128), a
    partial last chunk, and with the grid capped to 1 and 2 blocks several
    chunks per wave; the guard words past every output stay (gpu())."""
    for tracer in TRACERS:
        P, m, scene, rays, lens, near, occ = reference(tracer)
        ps = rt.PrimScene(P, m, tracer=tracer)
        try:
            with env(RT_PRIMS_QUERY_BLOCKS=blocks):
                check_nearest(rt, ps, scene, tracer, rays[:n], ref=tuple(a[:n] for a in near))
                check_shadow(rt, ps, scene, tracer, rays[:n], lens[:n], ref=occ[:n])
        finally:
            ps.close()


@pytest.mark.parametrize("tracer", TRACERS)
def test_outputs_not_requested_are_not_written(rt, tracer):
    """NEAREST with every subset of its three outputs (the others withheld
    and, inside gpu(), checked untouched); the shadow kinds with d_t and
    d_result passed all the same: they write d_id alone."""
    P, n, scene, rays, lens, near, occ = reference(tracer)
    rays, lens = rays[:200], lens[:200]
    ps = rt.PrimScene(P, n, tracer=tracer)
    try:
        for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False),
                     (False, True, True), (True, False, True)):
            for k in (1, 2):
                with env(RT_PRIMS_QUERY_RAYS=k):
                    got = gpu(rt, ps, rays, "nearest", want=want)
                for g, w, ref in zip(got, want, (near[0][:200].view(np.uint32), near[1][:200], near[2][:200])):
                    assert (g is None) == (not w)
                    if w:
                        agree("subset %r" % (want,), g, ref)
        check_shadow(rt, ps, scene, tracer, rays, lens, ref=occ[:200])
    finally:
        ps.close()


# ------------------------------------------------------------------ scene shapes
def shape(name, tracer):
    rng = np.random.default_rng(len(name))

    def geo():
        return rng.uniform(-9, 9, 3), rng.uniform(0.5, 9)

    def pgeo():
        v = rng.normal(size=3)
        return v / np.linalg.norm(v), rng.uniform(-9, 9)
    if name == "one sphere":
        return [R.sphere((0, 0, 6), 4.0)]
    if name == "one plane":
        return [R.plane((0, 0, -1), 8.0)]
    if name == "64 primitives":
        return None
    if name == "only spheres":
        return [R.sphere(*geo(), light=i % 5 == 0) for i in range(23)]
    if name == "only planes":
        return [R.plane(*pgeo(), light=i % 5 == 0) for i in range(9)]
    if name == "only lights":
        return [R.sphere(*geo(), light=True) if i % 2 else R.plane(*pgeo(), light=True) for i in range(12)]
    if name == "neither sphere nor plane":        # Whitted type 3 (BOX), queue type 2: in n, in no list
        return [(R.other(light=i % 4 == 1), R.sphere(*geo()), R.plane(*pgeo()))[i % 3] for i in range(20)]
    assert name == "neither light nor occluder" and tracer == "whitted"     # m_Light < 0
    return [(R.sphere(*geo(), light=i % 3 == 0, occluder=i % 3 == 1) if i % 2 else
             R.plane(*pgeo(), light=i % 3 == 0, occluder=i % 3 == 1)) for i in range(24)]


SHAPES = [(n, t) for n in ("one sphere", "one plane", "64 primitives", "only spheres", "only planes", "only lights",
                           "neither sphere nor plane") for t in TRACERS] + [("neither light nor occluder", "whitted")]


@pytest.mark.parametrize("name,tracer", SHAPES)
def test_scene_shapes(rt, name, tracer):
    prims = shape(name, tracer)
    scene = Q.big_scene(tracer) if prims is None else R.Scene(prims)
    assert scene.n == (64 if prims is None else len(prims))
    rays = Q.ray_set(scene, 600, 9)
    lens = Q.shadow_lengths(scene, rays, tracer, 2)
    near, occ = check_all(rt, scene, tracer, rays, lens)
    if name == "only lights":                      # no occluders at all
        assert (occ == -1).all() and (near[1] >= 0).any()
        inf = np.full(len(rays), INF, F)
        ps = prepared(rt, scene, tracer)
        try:
            assert (check_shadow(rt, ps, scene, tracer, rays, inf) == -1).all()
        finally:
            ps.close()
    else:
        assert (near[1] >= 0).any() and (occ != -1).any()
    if name == "neither light nor occluder":
        hit = near[1][near[1] >= 0]
        assert (~scene.light[hit] & ~scene.occluder[hit]).any()           # still nearest hits
        assert scene.occluder[occ[occ >= 0]].all()


# ------------------------------------------------------------------ far, ties
@pytest.mark.parametrize("kind", ["plane", "sphere"])
@pytest.mark.parametrize("tracer", TRACERS)
def test_far_boundary(rt, tracer, kind):
    """A first candidate exactly at far is a miss (strict '<'), one float
    below it a hit; alone, and before or after a nearer or a farther
    primitive (tests/test_gpu_prims.py test_far_boundary, through the public
    call).  A miss is id -1, t = far, result 0 for both tracers."""
    far = Q.FAR[tracer]
    others = [None, R.plane((0, 0, 1), -5.0), R.sphere((0, 0, 7), 4.0), R.sphere((0, 0, F(4) * far), 4.0)]
    for t in (TP.down(far), far, TP.up(far)):
        case = TP.far_case(kind, t)
        res, cand = R.candidate(R.Scene([case]), 0, TP.Z, tracer)
        assert res == 1 and cand == t, (kind, t, res, cand)          # the construction, in float32
        for other in others:
            for prims in ([case],) if other is None else ([other, case], [case, other]):
                scene = R.Scene(prims)
                ps = prepared(rt, scene, tracer)
                try:
                    ref = check_nearest(rt, ps, scene, tracer, [TP.Z] * 3)
                finally:
                    ps.close()
                k = prims.index(case)
                nearer = other is not None and R.candidate(scene, 1 - k, TP.Z, tracer)[1] < far
                if nearer:
                    assert ref[1][0] == 1 - k
                elif t < far:
                    assert (ref[1][0], ref[0][0], ref[2][0]) == (k, t, 1)
                else:
                    assert (ref[1][0], ref[0][0], ref[2][0]) == (-1, far, 0)


@pytest.mark.parametrize("name", sorted(TP.TIES))
@pytest.mark.parametrize("tracer", TRACERS)
def test_ties(rt, tracer, name):
    """Equal distances: the lowest index, with that primitive's result -- in
    the lean loops and, with a sphere of infinite radius in the scene, in the
    exact redo."""
    prims, ray, winner, dist, result = TP.TIES[name]
    for scene_prims, shift in ((prims, 0), (prims + [TP.BIG], 0), ([TP.BIG] + prims, 1)):
        scene = R.Scene(scene_prims)
        ps = prepared(rt, scene, tracer)
        try:
            t, ids, res = check_nearest(rt, ps, scene, tracer, [ray] * 5)
        finally:
            ps.close()
        assert (ids == winner + shift).all() and (t == F(dist)).all() and (res == result).all(), (t, ids, res)


# ------------------------------------------------------------------ sqrt_nr's range in mixed, partial waves
@pytest.mark.parametrize("tracer", TRACERS)
def test_redo_beside_ordinary_lanes_and_lanes_past_nrays(rt, tracer):
    """test_gpu_prims.py's room: a lane whose discriminant is outside
    sqrt_nr's range (2^-100, +inf) redoes its wave exactly.  One such lane per
    wave, and every second lane, beside ordinary lanes -- in batches that end
    inside a wave (and inside a two-per-lane chunk), so lanes past nrays sit
    in the redone wave too.  The ordinary lanes' answers are those of the
    batch without any such lane."""
    scene, rays, lens, odd, refs = TP.room()
    ps = prepared(rt, scene, tracer)
    try:
        for n in (64 * 3 + 17, 128 * 2 + 64 + 5):
            base = None
            for mode in TP.MODES:
                m = TP.replaced(n, mode)
                batch = np.where(m[:, None], odd[:n], rays[:n])
                near = check_nearest(rt, ps, scene, tracer, batch)
                occ = check_shadow(rt, ps, scene, tracer, batch, lens[:n])
                if mode == "alone":
                    base = (near, occ)
                    continue
                assert (near[1][m & (np.arange(n) % 4 < 2)] == 17).all()          # the 2^-100 sphere, hit at 2^-50
                for a, b in zip(base[0], near):
                    agree("ordinary lanes, %s vs alone" % mode, b[~m], a[~m])
                agree("ordinary lanes' occluders, %s vs alone" % mode, occ[~m], base[1][~m])
    finally:
        ps.close()


@pytest.mark.parametrize("tracer", TRACERS)
def test_small_discriminants(rt, tracer):
    """A ray from a sphere's centre has det == sq_radius exactly: every
    positive finite one hits from inside (result -1) at sqrtf(det), down to
    the subnormals; 0, inf and NaN miss.  Alone (a batch of one: 63 lanes past
    nrays) and all in one wave."""
    far = Q.FAR[tracer]
    centres = [(F(3 * i - 20), F(0.5 * i), F(2 + i)) for i in range(len(TP.SQ))]
    rays = np.array([[c[0], c[1], c[2], 0.6, 0.0, 0.8] for c in centres], F)
    for i, sq in enumerate(TP.SQ):
        scene = R.Scene([R.sphere(centres[i], sq)])
        ps = prepared(rt, scene, tracer)
        try:
            t, ids, res = check_nearest(rt, ps, scene, tracer, rays[i:i + 1])
            occ = check_shadow(rt, ps, scene, tracer, rays[i:i + 1], [INF])
        finally:
            ps.close()
        positive = bool(np.isfinite(F(sq)) and F(sq) > 0)
        hit = positive and np.sqrt(F(sq)) < far
        assert (ids[0], res[0]) == ((0, -1) if hit else (-1, 0)), (sq, ids, res)
        assert t[0] == (np.sqrt(F(sq)) if hit else far)
        assert occ[0] == (0 if positive else -1), (sq, occ)          # (no far in the shadow loop)
    finite = [i for i, sq in enumerate(TP.SQ) if sq != np.inf]
    scene = R.Scene([R.sphere(centres[i], TP.SQ[i]) for i in finite])
    check_all(rt, scene, tracer, rays[finite], np.full(len(finite), INF, F))


# ------------------------------------------------------------------ plane edges, NaN, inf
@pytest.mark.parametrize("tracer", TRACERS)
def test_plane_edges_and_non_finite_rays(rt, tracer):
    """d == +-0 (parallel), t == +-0, t < 0, t == +inf, and NaN / inf anywhere
    in a ray: the reference's own outcome for those floats."""
    scene = R.Scene([R.plane((0, 0, 1), -4.0), R.plane((0.6, 0, 0.8), -1e30), R.sphere((0, 3, 9), 4.0),
                     R.plane((0, 1, 0), 5.0)])
    rays = np.array([
        [0, 0, 0, 1, 0, 0], [0, 0, 0, -1, -1, -0.0], [0, 0, 4, 0, 0, 1], [0, 0, 4, 0, 0, -1], [0, 0, 9, 0, 0, 1],
        [0, 0, 0, 0, 0, 1e-30], [0, 0, 0, 0, 0, 1], [0, -5, 0, 0, 1, 0],
        [NAN, 0, 0, 0, 0, 1], [0, NAN, 0, 0, 0, 1], [0, 0, NAN, 0, 0, 1],
        [0, 0, 0, NAN, 0, 1], [0, 0, 0, 0, NAN, 1], [0, 0, 0, 0, 0, NAN],
        [INF, 0, 0, 0, 0, 1], [0, 0, -INF, 0, 0, 1], [0, 0, 0, INF, 0, 1], [0, 0, 0, 0, 0, INF],
        [0, 0, 0, 0, 0, -INF], [0, 0, 0, INF, INF, INF], [INF, INF, INF, INF, INF, INF], [NAN] * 6,
    ], F)
    ps = prepared(rt, scene, tracer)
    try:
        with np.errstate(all="ignore"):
            t, ids, res = check_nearest(rt, ps, scene, tracer, rays)
            assert (ids[6], t[6], res[6]) == (0, 4.0, 1) and ids[0] != 0 and ids[1] != 0
            assert (ids[-1], t[-1], res[-1]) == (-1, Q.FAR[tracer], 0)
            for length in (INF, F(3e38), F(5.0), F(0.0), NAN):
                check_shadow(rt, ps, scene, tracer, rays, np.full(len(rays), length, F))
    finally:
        ps.close()


# ------------------------------------------------------------------ bounds
@pytest.mark.parametrize("tracer", TRACERS)
def test_bounds(rt, tracer):
    """tmax at the hit distance is a miss, one float above it a hit, +inf
    leaves far in force, NaN, 0 and negative miss; a shadow length exactly at
    the occluder's distance is not occluded."""
    P, n, scene, rays, lens, near, occ = reference(tracer)
    rays, t0, id0 = rays[:1024], near[0][:1024], near[1][:1024]
    hit = id0 >= 0
    far = Q.FAR[tracer]
    ps = rt.PrimScene(P, n, tracer=tracer)
    try:
        t, ids, res = check_nearest(rt, ps, scene, tracer, rays, tmax=t0)
        assert (ids == -1).all() and (t == far).all() and (res == 0).all()
        t, ids, res = check_nearest(rt, ps, scene, tracer, rays, tmax=np.nextafter(t0, INF))
        agree("one float above: id", ids, id0)
        agree("one float above: t", t.view(np.uint32), t0.view(np.uint32))
        t, ids, res = check_nearest(rt, ps, scene, tracer, rays, tmax=np.full(1024, INF, F))
        agree("+inf: id", ids, id0)
        assert (~hit).any() and (t[~hit] == far).all()
        for b in (NAN, F(0), F(-0.0), F(-5), -INF):
            t, ids, res = check_nearest(rt, ps, scene, tracer, rays, tmax=np.full(1024, b, F))
            assert (ids == -1).all() and (t == far).all() and (res == 0).all(), b
        # shadow lengths at, just above and just below the nearest occluder's distance
        only = R.Scene([(scene.kind[i], tuple(scene.geo[i]), False, True) if scene.occluder[i] else R.other(light=True)
                        for i in range(scene.n)])
        d, p, _ = R.nearest(only, rays, tracer)
        has = p != R.TRAITS[tracer][2]
        assert has.sum() > 500
        at = check_shadow(rt, ps, scene, tracer, rays[has], d[has])
        above = check_shadow(rt, ps, scene, tracer, rays[has], np.nextafter(d[has], INF))
        assert (at == -1).all() and (above != -1).all()
    finally:
        ps.close()


# ------------------------------------------------------------------ set, then query
@pytest.mark.parametrize("tracer", TRACERS)
def test_set_then_query_on_one_stream(rt, tracer):
    """set_async and the three kinds enqueued back to back on a side stream,
    one synchronise at the end: the queries see the new primitives -- first
    another 17, then 64 with another light / occluder make-up, then 3."""
    import torch
    P, n, scene, rays, lens, near, occ = reference(tracer)
    rays, lens = rays[:1000], lens[:1000]
    d_rays, d_lens = dev(rays), dev(lens)
    big = Q.big_scene(tracer, seed=5)
    small = R.Scene([R.sphere((0, 0, 6), 4.0, light=True), R.plane((0, 0, -1), 20.0), R.sphere((1, 0, 9), 9.0)])
    moved = Q.scene_of(P, n, tracer)
    moved.geo[:, 3] *= F(1.25)
    assert big.occluder.sum() != scene.occluder.sum() and big.n == 64
    ps = rt.PrimScene(P, n, tracer=tracer)
    s = torch.cuda.Stream()
    try:
        for new in (moved, big, small):
            d_prims = prim_bytes(new.prims(tracer), new.n)
            outs = {k: tuple(torch.full((1000,), FILL_I, dtype=dt, device="cuda")
                             for dt in (torch.float32, torch.int32, torch.int32)) for k in Q.KINDS}
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                ps.set(d_prims, new.n)
                for k in Q.KINDS:
                    ps.query(d_rays, None if k == "nearest" else d_lens, kind=k, out=outs[k])
            s.synchronize()
            assert ps.n == new.n
            ref = Q.query(new, rays, tracer, "nearest")
            agree("after set: t", outs["nearest"][0].cpu().numpy().view(np.uint32), ref[0].view(np.uint32))
            agree("after set: id", outs["nearest"][1].cpu().numpy(), ref[1])
            agree("after set: result", outs["nearest"][2].cpu().numpy(), ref[2])
            rocc = Q.query(new, rays, tracer, "occluder", tmax=lens)
            agree("after set: occluder", outs["occluder"][1].cpu().numpy(), rocc)
            agree("after set: shadow", outs["shadow"][1].cpu().numpy(), (rocc != -1).astype(np.int32))
            assert (ref[1] != near[1][:1000]).any(), "the set must change some answers"
    finally:
        ps.close()


# ------------------------------------------------------------------ graph capture
@pytest.mark.parametrize("tracer", TRACERS)
def test_captured_queries_replay_and_follow_a_set(rt, tracer):
    """Three queries of different kinds captured into one graph: two replays
    give the same (right) results; after a set_async the next replay follows
    the new scene."""
    import torch
    P, n, scene, rays, lens, near, occ = reference(tracer)
    count = 1500
    rays, lens = rays[:count], lens[:count]
    d_rays, d_lens = dev(rays), dev(lens)
    t = torch.zeros(count, dtype=torch.float32, device="cuda")
    ids = torch.zeros(count, dtype=torch.int32, device="cuda")
    res = torch.zeros(count, dtype=torch.int32, device="cuda")
    sh = torch.zeros(count, dtype=torch.int32, device="cuda")
    oc = torch.zeros(count, dtype=torch.int32, device="cuda")
    ps = rt.PrimScene(P, n, tracer=tracer)
    try:
        ps.query(d_rays, kind="nearest", out=(t, ids, res))          # (code objects loaded before the capture)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ps.query(d_rays, kind="nearest", out=(t, ids, res))
            ps.query(d_rays, d_lens, kind="shadow", out=(None, sh, None))
            ps.query(d_rays, d_lens, kind="occluder", out=(None, oc, None))

        def replay(sc):
            for x in (t, ids, res, sh, oc):
                x.fill_(-7)
            g.replay()
            torch.cuda.synchronize()
            ref = Q.query(sc, rays, tracer, "nearest")
            rocc = Q.query(sc, rays, tracer, "occluder", tmax=lens)
            agree("replay: t", t.cpu().numpy().view(np.uint32), ref[0].view(np.uint32))
            agree("replay: id", ids.cpu().numpy(), ref[1])
            agree("replay: result", res.cpu().numpy(), ref[2])
            agree("replay: occluder", oc.cpu().numpy(), rocc)
            agree("replay: shadow", sh.cpu().numpy(), (rocc != -1).astype(np.int32))
            return ref[1].copy()
        first = replay(scene)
        replay(scene)
        big = Q.big_scene(tracer, seed=8)
        d_prims = prim_bytes(big.prims(tracer), big.n)
        ps.set(d_prims, big.n)
        assert (replay(big) != first).any()
        del g
    finally:
        ps.close()


# ------------------------------------------------------------------ arguments, with a device
@pytest.mark.parametrize("tracer", TRACERS)
def test_argument_errors_with_a_scene(rt, tracer):
    import torch
    P, n, scene, rays, lens, near, occ = reference(tracer)
    ps = rt.PrimScene(P, n, tracer=tracer)
    try:
        d_rays, d_lens = dev(rays[:64]), dev(lens[:64])
        ids = torch.full((64,), FILL_I, dtype=torch.int32, device="cuda")
        q = rt.entry("rtp_query_async")
        st = torch.cuda.current_stream().cuda_stream
        bad = rt._lib.RT_ERR_INVALID
        assert q(ps.handle, d_rays.data_ptr(), None, 64, 5, None, ids.data_ptr(), None, st) == bad
        assert q(ps.handle, d_rays.data_ptr(), None, 64, 0, None, None, None, st) == bad
        assert q(ps.handle, d_rays.data_ptr(), None, 64, 1, None, ids.data_ptr(), None, st) == bad
        assert q(ps.handle, d_rays.data_ptr(), d_lens.data_ptr(), 64, 2, None, None, None, st) == bad
        assert q(ps.handle, None, None, 64, 0, None, ids.data_ptr(), None, st) == bad
        assert q(ps.handle, d_rays.data_ptr(), None, 2 ** 31, 0, None, ids.data_ptr(), None, st) == bad
        assert q(ps.handle, d_rays.data_ptr(), None, 0, 0, None, ids.data_ptr(), None, st) == 0      # nothing to do
        other = "rtq_prims_set_async" if tracer == "whitted" else "rtw_prims_set_async"
        d_prims = prim_bytes(scene.prims(tracer), n)
        assert rt.entry(other)(ps.handle, d_prims.data_ptr(), n, st) == bad
        assert b"other tracer" in rt.lib().rt_last_error()
        for m in (0, 65):
            with pytest.raises(rt.RTError):
                ps.set(d_prims.data_ptr(), m)                       # (a raw device address)
        assert ps.n == n
        with pytest.raises(ValueError):
            ps.set(d_prims[:95], 1)
        with pytest.raises(ValueError):
            ps.query(d_rays, kind="shadow")
        with pytest.raises(ValueError):
            ps.query(d_rays, kind="any")
        with pytest.raises(ValueError):
            ps.query(d_rays.cpu())
        torch.cuda.synchronize()
        assert (ids.cpu().numpy() == FILL_I).all()                  # nothing was launched
        assert ps.query(d_rays[:0])[1].numel() == 0
        check_nearest(rt, ps, scene, tracer, rays[:64], ref=tuple(a[:64] for a in near))   # the scene is intact
    finally:
        ps.close()
