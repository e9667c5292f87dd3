"""CPU checks of the hierarchy layouts a scene can pick on its own
(csrc/spt_bvh.h choose_wide -- the rule spt_scene_create runs): each named
scene of tests/scenes_layouts.py lands in the layout class its name says, with
a margin of +-10 % in size, so the GPU tests built on them
(test_gpu_smallpt_layouts.py) run the leaf size they mean to; and the scalar
restatement of the wide walk (tests/native/spt_bvh_check.cpp) equals the full
scan at the chosen leaf size on the leaf-12 and leaf-16 scenes and on every
edge scene of the partition."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scenes_layouts as sl

NATIVE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "native")
WIDE_LDS_MAX = 144 * 1024


@pytest.fixture(scope="module")
def chk():
    subprocess.run(["make", "-s", "-C", NATIVE, "libspt_bvh_check.so"], check=True)
    L = C.CDLL(os.path.join(NATIVE, "libspt_bvh_check.so"))
    P = C.c_void_p
    L.spt_bvh_wide_check.restype = C.c_longlong
    L.spt_bvh_wide_check.argtypes = [P, C.c_int, P, P, C.c_longlong, P, P, P, P, P]
    L.spt_bvh_wide_choice.argtypes = [P, C.c_int, P]
    L.spt_bvh_set_leaf_max.argtypes = [C.c_int]
    return L


def choice(chk, S, n):
    """leaf_max, wnodes, wdepth, nalways, LDS bytes, and per leaf size 8, 12,
    16 the (wnodes, wdepth, LDS bytes) the rule weighed."""
    out = (C.c_longlong * 14)()
    lm = chk.spt_bvh_wide_choice(C.addressof(S), n, out)
    assert lm == out[0]
    per = {k: tuple(out[5 + 3 * i:8 + 3 * i]) for i, k in enumerate((8, 12, 16))}
    return dict(leaf_max=out[0], wnodes=out[1], wdepth=out[2], nalways=out[3], lds=out[4], per=per)


@pytest.mark.parametrize("name", list(sl.LAYOUT_SCENES))
def test_named_cloud_sizes_land_in_their_class(chk, name):
    """cloud(n) gets the leaf size its name says, and so do 0.9 n and 1.1 n;
    the choice is the smallest leaf size whose tree fits the LDS budget."""
    n, want = sl.LAYOUT_SCENES[name]
    for m in (n, int(0.9 * n), int(1.1 * n)):
        S, k = sl.cloud(m)
        c = choice(chk, S, k)
        print(name, m, c)
        assert c["leaf_max"] == want, (m, c)
        assert c["nalways"] == 2                            # the ground and the largest emitter
        fits = [lm for lm in (8, 12, 16) if c["per"][lm][2] <= WIDE_LDS_MAX]
        assert (fits[0] if fits else 0) == want
        if want:
            assert c["wdepth"] >= 2 and c["lds"] <= WIDE_LDS_MAX
            assert (c["wnodes"], c["wdepth"], c["lds"]) == c["per"][want]


def test_edge_scenes_are_what_they_claim(chk):
    """The partition's edges: no always sphere; 20 candidates of which 16 are
    taken; the 256-sphere threshold; coincident and duplicate spheres."""
    S, n = sl.no_always()
    r = sl.rows_of(S, n)[:, 0]
    assert n >= 256 and r.max() < 8 * r.min()
    c = choice(chk, S, n)
    assert c["nalways"] == 0 and c["leaf_max"] == 8 and c["wdepth"] >= 2, c

    (S, n), big = sl.many_always()
    r = sl.rows_of(S, n)[:, 0]
    assert n >= 256 and len(big) == 20 and (np.flatnonzero(r > 64 * np.median(r)) == big).all()
    c = choice(chk, S, n)
    assert c["nalways"] == 16 and c["leaf_max"] == 8 and c["wdepth"] >= 2, c

    S, n = sl.n256()
    c = choice(chk, S, n)
    assert n == 256 and c["leaf_max"] == 8 and c["wdepth"] >= 2 and c["wnodes"] >= 2, c
    T, m = sl.n255()
    assert m == 255 and bytes(T) == bytes(S)[:255 * 44]

    S, n = sl.coincident()
    rows = sl.rows_of(S, n)
    assert n >= 256
    sh, du = rows[sl.COINCIDENT_SHARED], rows[sl.COINCIDENT_DUPES]
    assert len(sh) == 40 and (sh[:, 1:4] == sh[0, 1:4]).all() and len(set(sh[:, 0])) == 40
    assert len(du) == 6 and (du[:, :4].view(np.uint32) == du[0, :4].view(np.uint32)).all()
    assert len({tuple(x) for x in du[:, 7:11].view(np.uint32)}) == 6          # colour and refl differ
    assert (np.diff(sl.COINCIDENT_DUPES) > 1).all()
    c = choice(chk, S, n)
    assert c["leaf_max"] == 8 and c["wdepth"] >= 2, c


@pytest.mark.parametrize("kind", sl.DEGENERATE_KINDS)
def test_degenerate_scenes_get_a_leaf8_hierarchy(chk, kind):
    """Negative, zero and non-finite radii and centres do not change the class
    the tests built on these scenes assume: an 8-wide tree with leaves of 8.
    The partition goes by |rad| against 64 x the median |rad| (NaNs apart):
    the first 16 spheres above it in index order are always spheres, so with
    40 infinite radii most of them land inside the tree."""
    S, n = sl.degenerate(kind)
    assert n == sl.DEGENERATE_N >= 256
    c = choice(chk, S, n)
    assert c["leaf_max"] == 8 and c["wdepth"] >= 2 and c["wnodes"] >= 2 and c["lds"] <= WIDE_LDS_MAX, c
    r = np.abs(sl.degenerate_rows(kind)[:, 0])
    with np.errstate(invalid="ignore"):
        big = int((r > np.float32(64) * np.sort(r[~np.isnan(r)])[(~np.isnan(r)).sum() // 2]).sum())
    assert c["nalways"] == min(big, 16) >= 1, (c, big)
    if kind in ("rad_inf", "rad_ninf"):
        assert big == 41 and c["nalways"] == 16
    if kind == "neg_all":
        base = choice(chk, *sl.degenerate_base())
        assert {k: c[k] for k in ("wnodes", "wdepth", "nalways", "lds")} == {k: base[k] for k in ("wnodes", "wdepth", "nalways", "lds")}


def test_small_degenerate_scenes_are_scanned_in_full():
    for kind in sl.DEGENERATE_SMALL_KINDS:
        assert sl.degenerate_small(kind)[1] == sl.DEGENERATE_SMALL_N < 256
    assert sl.nonfinite_colours()[1] < 256


def _rays(rng, rows, origin, nr, spread):
    """Origins around sphere centres and at the camera, random directions,
    some with an exactly zero component (the walk's 1e-30 clamp)."""
    cen = rows[:, 1:4].astype(np.float64)
    o = cen[rng.integers(0, len(cen), nr)] + rng.normal(0, spread, (nr, 3))
    o[: nr // 8] = origin
    d = rng.normal(0, 1, (nr, 3))
    d[: nr // 16, 1] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, d], 1)


def _on_sphere(rng, centre, rad, nr):
    """Origins on (float32-rounded, so just inside or outside) the sphere's
    surface, half the directions leaving it, half entering; then origins at
    the centre itself."""
    n = rng.normal(0, 1, (nr, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    d = rng.normal(0, 1, (nr, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.asarray(centre, np.float64) + rad * n
    o[nr // 2:] = centre
    return np.concatenate([o, d], 1)


def _walk_equals_scan(chk, S, n, rays, leaf_max):
    chk.spt_bvh_set_leaf_max(leaf_max)
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    nr = len(rays)
    tw, ts = np.zeros(nr, np.float32), np.zeros(nr, np.float32)
    iw, is_ = np.zeros(nr, np.int32), np.zeros(nr, np.int32)
    try:
        bad = chk.spt_bvh_wide_check(C.addressof(S), n, rays.ctypes.data, None, nr, tw.ctypes.data, iw.ctypes.data,
                                     ts.ctypes.data, is_.ctypes.data, None)
        assert bad == 0 and (iw >= -1).all()
        hits = is_.copy()
        # shadow queries: past the nearest hit (several occluders: the highest index counts), or a fixed reach
        maxt = np.where(is_ >= 0, ts * np.float32(1.5), np.float32(50.0)).astype(np.float32)
        bad = chk.spt_bvh_wide_check(C.addressof(S), n, rays.ctypes.data, maxt.ctypes.data, nr, tw.ctypes.data,
                                     iw.ctypes.data, ts.ctypes.data, is_.ctypes.data, None)
        assert bad == 0 and (iw >= -1).all()
    finally:
        chk.spt_bvh_set_leaf_max(4)
    return hits


@pytest.mark.parametrize("name", ["leaf12", "leaf16"])
def test_wide_walk_equals_full_scan_at_the_chosen_leaf_size(chk, name):
    n, want = sl.LAYOUT_SCENES[name]
    S, k = sl.cloud(n)
    assert choice(chk, S, k)["leaf_max"] == want
    rows = sl.rows_of(S, k)
    rays = _rays(np.random.default_rng(want), rows[4:], (1.0, 2.0, 25.0), 3000, 0.5)
    hits = _walk_equals_scan(chk, S, k, rays, want)
    assert (hits >= 4).sum() > 300                         # (rays that do hit cloud spheres, not only the ground)


@pytest.mark.parametrize("name", list(sl.EDGE_SCENES))
def test_wide_walk_equals_full_scan_on_edge_scenes(chk, name):
    make, cam = sl.EDGE_SCENES[name]
    S, n = make()
    lm = choice(chk, S, n)["leaf_max"]
    assert lm == 8
    rows = sl.rows_of(S, n)
    c = cam(64, 48)
    rng = np.random.default_rng(n)
    rays = [_rays(rng, rows, (c.orig.x, c.orig.y, c.orig.z), 3000, 0.3)]
    if name == "coincident":
        rays.append(_on_sphere(rng, sl.COINCIDENT_DUPE[:3], sl.COINCIDENT_DUPE[3], 600))
        rays.append(_on_sphere(rng, sl.COINCIDENT_CENTRE, 1.0, 600))
    rays = np.concatenate(rays)
    hits = _walk_equals_scan(chk, S, n, rays, lm)
    if name == "coincident":
        # the duplicates' nearest hits go to the tie index the full scan takes: the highest
        on_dupes = np.isin(hits, sl.COINCIDENT_DUPES)
        assert on_dupes.sum() > 200 and (hits[on_dupes] == sl.COINCIDENT_DUPES[-1]).all()
        assert np.isin(hits, sl.COINCIDENT_SHARED).sum() > 200
