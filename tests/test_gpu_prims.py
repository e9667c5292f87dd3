"""GPU check of rt_prims.h's loops on their own (tests/native/gpu_prims_check.hip):
nearest_n<1> and <2> with the Whitted and the queue tracer's traits,
first_occluder<true> and <false>, light_len_inv and fill_lists, against the
references' own loops over the oracle's per-primitive intersect
(tests/prims_ref.py, pinned by tests/test_prims_ref.py), at the edges where the
code branches: the far distance, discriminants outside sqrt_nr's range (alone
and beside ordinary lanes), distance ties, parallel planes, shadow lengths
equal to a candidate.  Everything is bit for bit."""
import functools

import numpy as np
import pytest

import gpu_native as G
import prims_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
TRAITS = ["whitted", "queue"]
NONE = R.NONE
INF, NAN = F(np.inf), F(np.nan)
Z = [0, 0, 0, 0, 0, 1]              # from the origin along z


def up(x):
    return np.nextafter(F(x), INF)


def down(x):
    return np.nextafter(F(x), -INF)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def bits1(x):
    return int(np.array(x, F).view(np.uint32))


def agree(what, got, want):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%s: %d of %d differ, first at %d: got %r, reference %r" % (
        what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]])


def build(scene):
    return G.prims_build(*scene.flags())[0]


def check_nearest(scene, rays, traits, ref=None, image=None):
    """nearest_n<1> and nearest_n<2> (the second ray of a lane: the next ray of
    the batch, and the one half a batch on) against the reference; returns
    the <1> answer."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    n = len(rays)
    image = build(scene) if image is None else image
    ref = R.nearest(scene, rays, traits) if ref is None else ref
    one = None
    for Rn, shift in ((1, 0), (2, 1), (2, max(1, n // 2))):
        d, p, r = G.prims_nearest(image, rays, Rn, traits, shift)
        for s in range(Rn):
            idx = (np.arange(n) + s * shift) % n
            tag = "%s nearest_n<%d> shift %d slot %d " % (traits, Rn, shift, s)
            agree(tag + "prim", p[s], ref[1][idx])
            agree(tag + "dist bits", d[s], bits(ref[0])[idx])
            agree(tag + "result", r[s], ref[2][idx])
        if Rn == 1:
            one = (d[0], p[0], r[0])
    return one


def check_occluder(scene, rays, lens, traits, ref=None, image=None):
    """first_occluder<true>: the position.  first_occluder<false>: occluded or
    not only -- it stops as soon as every lane of the wave has found some
    occluder, so the position it leaves is not the first one's."""
    rays = np.asarray(rays, F).reshape(-1, 6)
    lens = np.asarray(lens, F)
    image = build(scene) if image is None else image
    ref = R.first_occluder(scene, rays, lens, traits) if ref is None else ref
    counted = G.prims_occluder(image, rays, lens, True)
    agree(traits + " first_occluder<true> position", counted, ref)
    agree(traits + " first_occluder<false> occluded", G.prims_occluder(image, rays, lens, False) != NONE, ref != NONE)
    return counted


def check_len_inv(d2):
    """Bit for bit, but any NaN for a NaN (d2 is a sum of squares: a NaN there
    only propagates, and its payload is not the references' to define)."""
    d2 = np.asarray(d2, F)
    length, inv = R.light_len_inv(d2)
    gl, gi = G.prims_len_inv(d2)
    for what, got, want in (("len", gl, length), ("inv", gi, inv)):
        nan = np.isnan(want)
        agree("light_len_inv %s is NaN" % what, np.isnan(got.view(F)), nan)
        agree("light_len_inv %s bits" % what, got[~nan], bits(want)[~nan])
    return gl, gi


# ------------------------------------------------------------------ far boundary
def far_case(kind, t):
    """A primitive whose candidate along Z is exactly t."""
    if kind == "plane":
        return R.plane((0, 0, 1), -t)
    return R.sphere((0, 0, F(t) + F(2)), 4.0)


@pytest.mark.parametrize("kind", ["plane", "sphere"])
@pytest.mark.parametrize("traits", TRAITS)
def test_far_boundary(traits, kind):
    """A first candidate exactly at the far distance is no hit (the
    references test dist < far strictly: whitted_oracle.c:93-105,
    queue_oracle.c:51,70-71), one float below it is, one above is not; alone,
    and with a nearer or a farther sphere or plane before or after it.

    While nearest_n kept "no hit yet" as prim = T::miss (its tie clause,
    T::miss >= 0 || prim >= 0, is constant-true for Whitted's 0x7fffffff, and
    any id is below that), the MI355X failed the two Whitted cases of this
    test at their first comparison after the one-float-below case: the
    primitive alone, exactly at far, nearest_n<1> returned prim 0 where the
    reference misses (0x7fffffff), for the plane and for the sphere (the test
    stops there, so the later contexts were not reached).  Both queue cases
    passed.  (profiles/r15/gpu_prims_before_fix.log)"""
    far = R.TRAITS[traits][0]
    others = [None, R.plane((0, 0, 1), -5.0), R.sphere((0, 0, 7), 4.0), R.plane((0, 0, 1), -(F(4) * far)),
              R.sphere((0, 0, F(4) * far), 4.0)]
    for t in (down(far), far, up(far)):
        case = far_case(kind, t)
        res, cand = R.candidate(R.Scene([case]), 0, Z, traits)
        assert res == 1 and cand == t, (kind, t, res, cand)          # the construction, in float32
        for other in others:
            for prims in ([case],) if other is None else ([other, case], [case, other]):
                scene = R.Scene(prims)
                ref = R.nearest(scene, [Z], traits)
                k = prims.index(case)
                nearer = other is not None and R.candidate(scene, 1 - k, Z, traits)[1] < far
                # beside a nearer primitive that one; else the case exactly when t < far
                want = 1 - k if nearer else (k if t < far else R.TRAITS[traits][2])
                assert ref[1][0] == want, (kind, t, ref)
                check_nearest(scene, [Z] * 3, traits, ref=tuple(np.repeat(a, 3) for a in ref))


# ------------------------------------------------------------------ small discriminants
SQ = [2.0 ** -95, 2.0 ** -96, 2.0 ** -97, 2.0 ** -102, 2.0 ** -103, 2.0 ** -126, 2.0 ** -127, 2.0 ** -140,
      2.0 ** -149, float(np.finfo(F).max), np.inf, np.nan, 0.0, -0.0]


@pytest.mark.parametrize("traits", TRAITS)
def test_small_discriminants(traits):
    """A ray from a sphere's centre has det == sq_radius exactly (v = 0, b = -0).
    Below 2^-96 (down to the subnormals) the lean loop's sqrt_nr is out of
    range and the loop is redone exactly; the reference hits, INPRIM at
    sqrtf(det), for every positive finite det.  sq_radius = +-0 gives
    det = +0 (a det of -0 cannot come out of b * b - v.v + sq_radius for
    sq_radius >= 0: b * b is never -0), a miss."""
    far, result0, miss = R.TRAITS[traits]
    centres = [(F(3 * i - 20), F(0.5 * i), F(2 + i)) for i in range(len(SQ))]
    rays = np.array([[c[0], c[1], c[2], 0.6, 0.0, 0.8] for c in centres], F)
    everything = R.Scene([R.sphere(c, sq) for c, sq in zip(centres, SQ)])
    finite = [i for i, sq in enumerate(SQ) if sq != np.inf]     # (the infinite one puts every ray out of range)
    mixed = R.Scene([R.sphere(centres[i], SQ[i]) for i in finite])
    for i, sq in enumerate(SQ):
        alone = R.Scene([R.sphere(centres[i], sq)])
        res, cand = R.candidate(alone, 0, rays[i], traits)
        positive = np.isfinite(F(sq)) and F(sq) > 0
        assert (res, cand) == ((-1, np.sqrt(F(sq))) if positive else (0, INF)), (sq, res, cand)
        d, p, r = check_nearest(alone, rays[i:i + 1], traits)
        hit = positive and np.sqrt(F(sq)) < far
        assert (p[0], r[0]) == ((0, -1) if hit else (miss, result0)), (sq, p, r)
        assert d[0] == bits1(np.sqrt(F(sq)) if hit else far), (sq, d)
        first = check_occluder(alone, rays[i:i + 1], [INF], traits)
        assert first[0] == (0 if positive else NONE), (sq, first)
    # all of them in one scene, a ray from each centre in one wave: each lane's
    # own sphere is out of range or not, the other spheres are ordinary for it
    for scene, batch in ((everything, rays), (mixed, rays[finite])):
        check_nearest(scene, batch, traits)
        check_occluder(scene, batch, np.full(len(batch), INF, F), traits)
        check_occluder(scene, batch, np.full(len(batch), 1e-30, F), traits)


# ------------------------------------------------------------------ mixed waves
TINY_C = (F(1.5), F(-2.25), F(0.75))


@functools.lru_cache(maxsize=None)
def room():
    """A random 40-primitive scene (spheres, planes, lights of both kinds)
    with one more sphere of squared radius 2^-100 at TINY_C, ordinary rays into
    it with shadow lengths, their reference answers, and the out-of-range rays:
    from TINY_C (det = 2^-100 for that sphere: below sqrt_nr's range, a hit
    at 2^-50) and with a direction of length 1e20 (det = +inf)."""
    rng = np.random.default_rng(20260)
    prims = []
    for i in range(40):
        light = rng.random() < 0.15
        if rng.random() < 0.6:
            prims.append(R.sphere(rng.uniform(-10, 10, 3), rng.uniform(0.1, 9.0), light=light))
        else:
            v = rng.normal(size=3)
            prims.append(R.plane(v / np.linalg.norm(v), rng.uniform(-10, 10), light=light))
    prims.insert(17, R.sphere(TINY_C, 2.0 ** -100))
    scene = R.Scene(prims)
    n = 1024 + 17

    def directions(m):
        v = rng.normal(size=(m, 3)).astype(F)
        return v * (F(1) / np.sqrt((v * v).sum(1, dtype=F)))[:, None]
    rays = np.concatenate([rng.uniform(-10, 10, (n, 3)).astype(F), directions(n)], 1)
    lens = rng.uniform(0.5, 30, n).astype(F)
    odd = np.concatenate([np.tile(np.array(TINY_C, F), (n, 1)), directions(n)], 1)
    huge = np.arange(n) % 4 >= 2
    odd[huge, :3] = rays[huge, :3]
    odd[huge, 3:] *= F(1e20)
    refs = {t: (R.nearest(scene, rays, t), R.first_occluder(scene, rays, lens, t),
                R.nearest(scene, odd, t), R.first_occluder(scene, odd, lens, t)) for t in TRAITS}
    return scene, rays, lens, odd, refs


def replaced(n, mode):
    """The lanes given an out-of-range input: none, one per wave of 64 (its
    place moving from wave to wave), or every second one."""
    idx = np.arange(n)
    if mode == "alone":
        return np.zeros(n, bool)
    if mode == "one":
        return idx % 64 == (7 * (idx // 64) + 3) % 64
    return idx % 2 == 1


MODES = ["alone", "one", "half"]


@pytest.mark.parametrize("traits", TRAITS)
def test_redo_in_mixed_waves(traits):
    """The whole-wave redo (a lane's det outside [2^-96, inf)) leaves the
    other lanes' answers what they were: the same ordinary rays alone, with
    one lane per wave out of range, and with every second one."""
    scene, rays, lens, odd, refs = room()
    near_ref, occ_ref, near_odd, occ_odd = refs[traits]
    # the out-of-range rays are what they are meant to be
    res, cand = R.candidate(scene, 17, odd[0], traits)
    assert res == -1 and cand == F(2.0 ** -50)
    tiny = np.arange(len(odd)) % 4 < 2
    assert (near_odd[1][tiny] == 17).all() and (near_odd[0][tiny] == F(2.0 ** -50)).all()
    image = build(scene)
    near, occ = {}, {}
    for mode in MODES:
        m = replaced(len(rays), mode)
        batch = np.where(m[:, None], odd, rays)
        nref = tuple(np.where(m, o, a) for a, o in zip(near_ref, near_odd))
        oref = np.where(m, occ_odd, occ_ref)
        near[mode] = check_nearest(scene, batch, traits, ref=nref, image=image)
        occ[mode] = check_occluder(scene, batch, lens, traits, ref=oref, image=image)
    for mode in MODES[1:]:
        keep = ~replaced(len(rays), mode)
        for a, b in zip(near["alone"], near[mode]):
            agree("ordinary lanes, %s vs alone" % mode, b[keep], a[keep])
        agree("ordinary lanes' occluders, %s vs alone" % mode, occ[mode][keep], occ["alone"][keep])


def test_len_inv_in_mixed_waves():
    rng = np.random.default_rng(5)
    n = 1024 + 17
    d2 = (rng.uniform(0.05, 40, n).astype(F)) ** 2
    odd = np.resize(np.array([2.0 ** -97, 2.0 ** -120, 2.0 ** -140, 2.0 ** -149, 0.0, np.inf, np.nan, 2.0 ** 127],
                             F), n)
    out = {}
    for mode in MODES:
        m = replaced(n, mode)
        out[mode] = check_len_inv(np.where(m, odd, d2))
    for mode in MODES[1:]:
        keep = ~replaced(n, mode)
        for a, b in zip(out["alone"], out[mode]):
            agree("ordinary lanes, %s vs alone" % mode, b[keep], a[keep])


# ------------------------------------------------------------------ ties
BIG = ("s", (0.0, 0.0, 0.0, float("inf")), False, True)     # det = +inf for every ray: forces the redo, never hit

TIES = {
    # name: (primitives, ray, winner, dist, result)
    "two spheres": ([R.sphere((0, 0, 10), 4.0)] * 2, Z, 0, 8.0, 1),
    "three spheres": ([R.sphere((0, 0, 10), 4.0)] * 3, Z, 0, 8.0, 1),
    "plane below sphere": ([R.plane((0, 0, -1), 8.0), R.sphere((0, 0, 10), 4.0)], Z, 0, 8.0, 1),
    "plane above sphere": ([R.sphere((0, 0, 10), 4.0), R.plane((0, 0, -1), 8.0)], Z, 0, 8.0, 1),
    "two planes": ([R.plane((0, 0, -1), 8.0)] * 2, Z, 0, 8.0, 1),
    "plane sphere sphere": ([R.plane((0, 0, -1), 8.0)] + [R.sphere((0, 0, 10), 4.0)] * 2, Z, 0, 8.0, 1),
    "sphere plane plane": ([R.sphere((0, 0, 10), 4.0)] + [R.plane((0, 0, -1), 8.0)] * 2, Z, 0, 8.0, 1),
    "sphere plane sphere": ([R.sphere((0, 0, 10), 4.0), R.plane((0, 0, -1), 8.0), R.sphere((0, 0, 10), 4.0)],
                            Z, 0, 8.0, 1),
    # from a sphere's centre: its exit (INPRIM, result -1) and a plane, both at 2
    "inside sphere then plane": ([R.sphere((0, 0, 6), 4.0), R.plane((0, 0, -1), 8.0)], [0, 0, 6, 0, 0, 1], 0, 2.0,
                                 -1),
    "plane then inside sphere": ([R.plane((0, 0, -1), 8.0), R.sphere((0, 0, 6), 4.0)], [0, 0, 6, 0, 0, 1], 0, 2.0,
                                 1),
    "farther first": ([R.sphere((0, 0, 20), 4.0), R.plane((0, 0, -1), 8.0), R.sphere((0, 0, 10), 4.0)], Z, 1, 8.0,
                      1),
}


@pytest.mark.parametrize("name", sorted(TIES))
@pytest.mark.parametrize("traits", TRAITS)
def test_ties(traits, name):
    """Equal distances: the lowest index wins (the references' strict '<' over
    ascending indices) and the result is the winner's -- in the lean loops and,
    with a sphere of infinite radius in the scene, in the redo loop."""
    prims, ray, winner, dist, result = TIES[name]
    cands = [R.candidate(R.Scene(prims), k, ray, traits)[1] for k in range(len(prims))]
    assert min(cands) == dist and cands.index(dist) == winner and cands.count(dist) >= 2, cands
    for scene_prims, shift in ((prims, 0), (prims + [BIG], 0), ([BIG] + prims, 1)):
        scene = R.Scene(scene_prims)
        d, p, r = check_nearest(scene, [ray] * 5, traits)
        assert (p == winner + shift).all() and (d == bits1(dist)).all() and (r == result).all(), (d, p, r)


# ------------------------------------------------------------------ plane edges
@pytest.mark.parametrize("traits", TRAITS)
def test_plane_edges(traits):
    """d == +0 and -0 (parallel: no division result is kept), t == 0, t < 0,
    t == +inf, and NaN / inf components in the ray (they only feed arithmetic
    and selects: no index or address depends on a ray)."""
    scene = R.Scene([R.plane((0, 0, 1), -4.0), R.plane((0.6, 0, 0.8), -1e30), R.sphere((0, 3, 9), 4.0),
                     R.plane((0, 1, 0), 5.0)])
    rays = np.array([
        [0, 0, 0, 1, 0, 0],                 # plane 0: d = +0
        [0, 0, 0, -1, -1, -0.0],            # plane 0: d = -0
        [0, 0, 4, 0, 0, 1],                 # plane 0: t = -0
        [0, 0, 4, 0, 0, -1],                # plane 0: t = +0
        [0, 0, 9, 0, 0, 1],                 # plane 0: t < 0
        [0, 0, 0, 0, 0, 1e-30],             # plane 1: t = 1e30 / 8e-31 = +inf in float32
        [0, 0, 0, 0, 0, 1],
        [0, -5, 0, 0, 1, 0],                # on plane 3
        [NAN, 0, 0, 0, 0, 1], [0, NAN, 0, 0, 0, 1], [0, 0, NAN, 0, 0, 1],
        [0, 0, 0, NAN, 0, 1], [0, 0, 0, 0, NAN, 1], [0, 0, 0, 0, 0, NAN],
        [INF, 0, 0, 0, 0, 1], [0, 0, -INF, 0, 0, 1], [0, 0, 0, INF, 0, 1], [0, 0, 0, 0, 0, INF],
        [0, 0, 0, 0, 0, -INF], [0, 0, 0, INF, INF, INF], [INF, INF, INF, INF, INF, INF],
        [NAN] * 6,
    ], F)
    with np.errstate(all="ignore"):
        assert R.candidate(scene, 0, rays[0], traits) == (0, INF) and R.candidate(scene, 0, rays[1], traits) == (0, INF)
        assert F(1e30) / (F(0.8) * F(1e-30)) == INF
        assert R.candidate(scene, 1, rays[5], traits) == (0, INF)       # t = +inf beats no distance
    d, p, r = check_nearest(scene, rays, traits)
    assert p[6] == 0 and d[6] == bits1(4)
    assert not np.isnan(d.view(F)).any()
    for length in (INF, F(3e38), F(5.0), F(0.0)):
        check_occluder(scene, rays, np.full(len(rays), length, F), traits)


# ------------------------------------------------------------------ occluders
def test_occluder_lengths():
    """len exactly a candidate (strict '<': not occluded), one float above
    it, 0 and +inf; the counted position is the first occluding entry's in the
    non-light order even when that is a plane after the sphere loop found a
    later sphere."""
    prims = [R.sphere((0, 0, 3), 0.25, light=True), R.plane((0, 0, -1), 12.0), R.sphere((0, 0, 10), 4.0),
             R.sphere((0, 0, 30), 4.0)]
    scene = R.Scene(prims)
    lens = np.array([0.0, down(8), 8.0, up(8), 12.0, up(12), 28.0, up(28), INF], F)
    rays = [Z] * len(lens)
    for traits in TRAITS:
        first = check_occluder(scene, rays, lens, traits)
        # positions among the non-lights: plane 0, sphere (0,0,10) 1, sphere (0,0,30) 2
        assert first.tolist() == [NONE, NONE, NONE, 1, 1, 0, 0, 0, 0]


def test_occluder_compositions():
    lit = [R.sphere((0, 0, 10), 4.0, light=True), R.plane((0, 0, -1), 12.0, light=True)]
    for traits in TRAITS:
        first = check_occluder(R.Scene(lit), [Z] * 3, [0.0, 20.0, INF], traits)      # only lights
        assert (first == NONE).all()
    # no occluders: lights and primitives that are neither light nor occluder (Whitted's m_Light < 0)
    neither = lit + [R.sphere((0, 0, 10), 4.0, occluder=False), R.plane((0, 0, -1), 12.0, occluder=False)]
    first = check_occluder(R.Scene(neither), [Z] * 3, [0.0, 20.0, INF], "whitted")
    assert (first == NONE).all()
    d, p, r = check_nearest(R.Scene(neither), [Z], "whitted")
    assert p[0] == 0                                                              # still a nearest hit
    # positions skip lights and the neither-nor: the plane (position 0) before the sphere (1)
    mixed = [R.sphere((0, 0, 10), 4.0, light=True), R.sphere((0, 0, 10), 4.0, occluder=False), R.plane((0, 0, -1), 5.0),
             R.sphere((0, 0, 10), 4.0)]
    first = check_occluder(R.Scene(mixed), [Z] * 4, [5.0, up(5), 8.0, up(8)], "whitted")
    assert first.tolist() == [NONE, 0, 0, 0]
    swapped = [mixed[0], mixed[1], mixed[3], mixed[2]]
    first = check_occluder(R.Scene(swapped), [Z] * 4, [5.0, up(5), 8.0, up(8)], "whitted")
    assert first.tolist() == [NONE, 1, 1, 0]


# ------------------------------------------------------------------ batch sizes
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4096 + 17])
def test_batch_sizes(n):
    scene, rays, lens, odd, refs = room()
    reps = -(-n // len(rays))
    batch, blens = np.tile(rays, (reps, 1))[:n], np.tile(lens, reps)[:n]
    image = build(scene)
    for traits in TRAITS:
        near_ref, occ_ref = refs[traits][:2]
        check_nearest(scene, batch, traits, ref=tuple(np.tile(a, reps)[:n] for a in near_ref), image=image)
        check_occluder(scene, batch, blens, traits, ref=np.tile(occ_ref, reps)[:n], image=image)
    check_len_inv(np.tile(lens, reps)[:n] ** 2)


# ------------------------------------------------------------------ fill_lists
def composition(name, n):
    rng = np.random.default_rng(n)

    def geo():
        return rng.uniform(-9, 9, 3), rng.uniform(0.1, 9)
    if name == "spheres":
        return [R.sphere(*geo()) for _ in range(n)]
    if name == "planes":
        return [R.plane(*geo()) for _ in range(n)]
    if name == "lights":
        return [R.sphere(*geo(), light=True) for _ in range(n)]
    if name == "alternating":
        return [(R.sphere, R.plane)[i % 2](*geo(), light=i % 4 >= 2) for i in range(n)]
    if name == "neither type":
        return [(R.other(light=i % 3 == 1), R.sphere(*geo()), R.plane(*geo()))[i % 3 if i % 5 else 0] for i in range(n)]
    if name == "neither light nor occluder":
        return [(R.sphere, R.plane)[i % 2](*geo(), light=i % 3 == 0, occluder=i % 3 == 1) for i in range(n)]
    assert name == "light planes"
    return [R.plane(*geo(), light=i % 2 == 0) if i % 3 else R.sphere(*geo(), light=i % 2 == 1) for i in range(n)]


@pytest.mark.parametrize("name", ["spheres", "planes", "lights", "alternating", "neither type",
                                  "neither light nor occluder", "light planes"])
@pytest.mark.parametrize("n", [1, 2, 63, 64])
def test_fill_lists(n, name):
    """Every list, id, position and count against a plain numpy construction;
    only the first `count` entries of a list are defined."""
    scene = R.Scene(composition(name, n))
    image, rank = G.prims_build(*scene.flags())
    want, want_rank = R.lists(scene)
    counts = {"sph": "ns", "sph_id": "ns", "pln": "np", "pln_id": "np", "osph": "nos", "osph_pos": "nos",
              "opln": "nop", "opln_pos": "nop"}
    for c in ("n", "ns", "np", "nos", "nop", "nlights", "nnonlight"):
        assert int(image[c]) == want[c], (c, int(image[c]), want[c])
    for field, c in counts.items():
        got = image[field][:want[c]]
        if got.dtype == F:
            agree(field, bits(got), bits(want[field]))
        else:
            agree(field, got, want[field])
    agree("light rank", rank, want_rank)
