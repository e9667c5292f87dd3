"""Test scenes that land in each layout the smallpt hierarchy code can pick
(csrc/spt_bvh.h choose_wide: leaf size 8, 12, 16 or no 8-wide tree) and on
the edges of its partition (the 64 x median "always" rule, the 256-sphere
threshold, coincident and duplicate spheres).  A plain helper module: every
generator is deterministic and fills the ctypes array in one copy.

tests/test_bvh_layouts.py pins each named scene to the class its name says,
so a GPU test built on one cannot quietly test another layout."""
import ctypes as C

import numpy as np

import rtamd

DIFF, SPEC, REFR = 0, 1, 2
f32 = np.float32


def pack(rows):
    """(Sphere array, count) from float32 rows [n, 11]: rad, p, e, c, refl
    (the refl column holds small integers)."""
    rows = np.ascontiguousarray(rows, dtype=f32)
    n = len(rows)
    raw = rows.copy()
    raw[:, 10].view(np.int32)[:] = rows[:, 10].astype(np.int32)
    arr = (rtamd.Sphere * n)()
    C.memmove(arr, raw.ctypes.data, raw.nbytes)
    return arr, n


def rows_of(arr, n):
    """The float view [n, 11] of a Sphere array (refl as raw bits)."""
    return np.ctypeslib.as_array(C.cast(arr, C.POINTER(C.c_float)), shape=(n * 11,)).reshape(n, 11)


def camera(orig, target, w, h, fov_deg=45.0):
    cam = rtamd.Camera()
    cam.orig = rtamd.Vec3(*map(float, orig))
    cam.target = rtamd.Vec3(*map(float, target))
    return rtamd.scenes.update_camera(cam, w, h, fov_deg=fov_deg)


def _stream(seed, k):
    # one generator per attribute: cloud(n) is a prefix of cloud(n + 1)
    return np.random.default_rng([seed, k])


def cloud_rows(n, seed=1, half=30.0, rad_exp=(-2.5, -0.5)):
    """A uniform cloud in [-half, half]^3 with radii 10^U(rad_exp), materials
    DIFF : SPEC : REFR = 3 : 1 : 1; sphere 0 is the ground, 1..3 are emitters
    of different sizes."""
    s = half / 30.0
    rows = np.zeros((n, 11), f32)
    rows[:, 0] = 10.0 ** _stream(seed, 0).uniform(rad_exp[0], rad_exp[1], n)
    rows[:, 1:4] = _stream(seed, 1).uniform(-half, half, (n, 3))
    rows[:, 7:10] = _stream(seed, 2).uniform(0.2, 0.9, (n, 3))
    rows[:, 10] = np.array([DIFF, DIFF, DIFF, SPEC, REFR], f32)[_stream(seed, 3).integers(0, 5, n)]
    rows[0] = [1e4, 0.0, -1e4 - half - 2.0, 0.0, 0, 0, 0, 0.7, 0.7, 0.7, DIFF]
    rows[1] = [3.0, 0.0, 40.0 * s, 0.0, 20, 20, 20, 0, 0, 0, DIFF]
    rows[2] = [0.5, 10.0 * s, 5.0 * s, -5.0 * s, 5, 3, 3, 0, 0, 0, DIFF]
    rows[3] = [1.5, -12.0 * s, 20.0 * s, 8.0 * s, 8, 8, 10, 0, 0, 0, DIFF]
    return rows


def cloud_camera(w, h, half=30.0):
    """Inside the cloud, looking through its centre."""
    s = half / 30.0
    return camera((1.0 * s, 2.0 * s, 25.0 * s), (0.0, 0.0, 0.0), w, h)


def cloud(n, seed=1):
    return pack(cloud_rows(n, seed))


def cloud_one_light(n, seed=1):
    """cloud(n) with emitter 1 as its only light: spheres 2 and 3 emit
    nothing and are grey (single-light scenes run the two-query kernels)."""
    rows = cloud_rows(n, seed)
    rows[2:4, 4:7] = 0.0
    rows[2:4, 7:10] = 0.5
    return pack(rows)


# Sizes of cloud(n) for the three layout classes past leaf 8 (cloud(3000)):
# each sits clear of its class's boundaries -- 0.9 n and 1.1 n land in the
# same class (test_bvh_layouts.py checks all three, and the summary of the
# change that added them lists wide nodes, depth and LDS bytes per leaf size).
N_LEAF8, N_LEAF12, N_LEAF16, N_NOWIDE = 3000, 30000, 43000, 56000
LAYOUT_SCENES = {"leaf8": (N_LEAF8, 8), "leaf12": (N_LEAF12, 12), "leaf16": (N_LEAF16, 16),
                 "nowide": (N_NOWIDE, 0)}


# ---- small scenes on the edges of the partition (each n >= 256 but n255)
_SMALL_HALF, _SMALL_EXP = 5.0, (-1.5, -0.3)


def n256():
    """The smallest scene that gets a hierarchy (sptbvh::MIN_SPHERES)."""
    return pack(cloud_rows(256, 7, _SMALL_HALF, _SMALL_EXP))


def n255():
    """n256 without its last sphere: scanned in full."""
    return pack(cloud_rows(256, 7, _SMALL_HALF, _SMALL_EXP)[:255])


def small_camera(w, h):
    return cloud_camera(w, h, _SMALL_HALF)


def no_always():
    """300 spheres whose radii lie within 8 x of each other (the light and
    the floor-like sphere included): none passes the 64 x median rule."""
    n = 300
    rows = np.zeros((n, 11), f32)
    rows[:, 0] = _stream(11, 0).uniform(0.25, 1.5, n)
    rows[:, 1:4] = _stream(11, 1).uniform(-10, 10, (n, 3))
    rows[:, 7:10] = _stream(11, 2).uniform(0.2, 0.9, (n, 3))
    rows[:, 10] = np.array([DIFF, DIFF, DIFF, SPEC, REFR], f32)[_stream(11, 3).integers(0, 5, n)]
    rows[0] = [1.9, 0.0, 9.0, 0.0, 30, 30, 30, 0, 0, 0, DIFF]
    rows[1] = [1.0, -6.0, 4.0, 5.0, 9, 6, 6, 0, 0, 0, DIFF]
    return pack(rows)


def no_always_camera(w, h):
    return camera((0.5, 1.0, 9.0), (0.0, 0.0, 0.0), w, h)


MANY_ALWAYS_BIG = 20


def many_always():
    """300 spheres, 20 of them above 64 x the median radius: the first 16 in
    index order are tested outside the tree, the last four go into it with
    boxes that span the scene."""
    n = 300
    rows = np.zeros((n, 11), f32)
    rows[:, 0] = 10.0 ** _stream(12, 0).uniform(-1.3, -0.5, n)           # median ~0.13: 64 x is ~8
    rows[:, 1:4] = _stream(12, 1).uniform(-6, 6, (n, 3))
    rows[:, 7:10] = _stream(12, 2).uniform(0.2, 0.9, (n, 3))
    rows[:, 10] = np.array([DIFF, DIFF, DIFF, SPEC, REFR], f32)[_stream(12, 3).integers(0, 5, n)]
    big = np.arange(MANY_ALWAYS_BIG) * 14 + 5                            # 5, 19, ..., 271
    rng = _stream(12, 4)
    d = rng.normal(0, 1, (MANY_ALWAYS_BIG, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rad = rng.uniform(25.0, 60.0, MANY_ALWAYS_BIG)
    rows[big, 0] = rad
    rows[big, 1:4] = d * (rad + rng.uniform(8.0, 14.0, MANY_ALWAYS_BIG))[:, None]   # a shell of walls around the cloud
    rows[big, 10] = np.array([DIFF, SPEC, DIFF, REFR], f32)[np.arange(MANY_ALWAYS_BIG) % 4]
    rows[2] = [0.8, 0.0, 5.0, 0.0, 40, 40, 40, 0, 0, 0, DIFF]
    rows[big[-1], 4:7] = [3, 3, 4]                                       # one of the in-tree huge ones is a light
    return pack(rows), big


def many_always_camera(w, h):
    """Through the small spheres towards one of the four huge ones in the tree."""
    (S, n), big = many_always()
    target = rows_of(S, n)[big[-2], 1:4].astype(np.float64)
    return camera(-5.5 * target / np.linalg.norm(target), target, w, h)


COINCIDENT_SHARED = np.arange(10, 250, 6)                                # 40 indices, one centre
COINCIDENT_DUPES = np.array([7, 59, 111, 163, 215, 297])                 # bit-identical geometry
COINCIDENT_CENTRE = (-2.5, 0.5, 0.0)
COINCIDENT_DUPE = (1.0, 0.0, 0.0, 1.0)                                   # centre, radius


def coincident():
    """300 spheres: 40 share one centre with distinct radii (SAH's
    zero-extent fallback splits them), 6 more are bit-identical in centre and
    radius and differ only in colour and refl, at non-adjacent indices.  The
    nearest hit on the duplicates is the full scan's tie index (the highest),
    whose material colours the pixel; a counted shadow query reports the
    highest occluder."""
    assert not set(COINCIDENT_SHARED) & set(COINCIDENT_DUPES)
    n = 300
    rows = np.zeros((n, 11), f32)
    rows[:, 0] = 10.0 ** _stream(13, 0).uniform(-1.3, -0.5, n)
    rows[:, 1:4] = _stream(13, 1).uniform(-6, 6, (n, 3))
    rows[:, 7:10] = _stream(13, 2).uniform(0.2, 0.9, (n, 3))
    rows[:, 10] = np.array([DIFF, DIFF, DIFF, SPEC, REFR], f32)[_stream(13, 3).integers(0, 5, n)]
    rows[0] = [1e4, 0.0, -1e4 - 8.0, 0.0, 0, 0, 0, 0.7, 0.7, 0.7, DIFF]
    rows[1] = [2.0, 0.0, 9.0, 2.0, 25, 25, 25, 0, 0, 0, DIFF]
    rows[COINCIDENT_SHARED, 0] = 0.3 + 0.03 * np.arange(len(COINCIDENT_SHARED))
    rows[COINCIDENT_SHARED, 1:4] = COINCIDENT_CENTRE
    rows[COINCIDENT_SHARED, 10] = np.array([REFR, REFR, DIFF, SPEC], f32)[np.arange(len(COINCIDENT_SHARED)) % 4]
    rows[COINCIDENT_DUPES, 0] = COINCIDENT_DUPE[3]
    rows[COINCIDENT_DUPES, 1:4] = COINCIDENT_DUPE[:3]
    rows[COINCIDENT_DUPES, 10] = [DIFF, SPEC, REFR, SPEC, REFR, DIFF]
    rows[COINCIDENT_DUPES, 7:10] = [[.9, .1, .1], [.1, .9, .1], [.1, .1, .9], [.9, .9, .1], [.1, .9, .9], [.9, .2, .8]]
    return pack(rows)


def coincident_camera(w, h):
    """Aimed between the duplicates and the shared centre: both fill a good
    part of the frame, so first hits land on them."""
    return camera((-0.5, 0.6, 5.8), (-0.6, 0.2, 0.0), w, h)


# ---- degenerate sphere data: negative, zero and non-finite radii and centres
# The reference uses a radius only as rad * rad (geomfunc.h:42): a sphere of
# radius -2 is the sphere of radius 2, and a sphere with a non-finite radius
# or centre is never hit.  Each kind edits radii and centres of the 300-sphere
# small cloud; the ground and the lights (indices 0..3) stay as they are.
DEGENERATE_N, DEGENERATE_SMALL_N = 300, 40
DEGENERATE_IDX = np.arange(20, 300, 7)                                   # 40 indices
DEGENERATE_SMALL_IDX = np.arange(5, 40, 3)                               # 12 indices
DEGENERATE_KINDS = ("neg", "neg_all", "zero", "denorm", "rad_inf", "rad_ninf", "rad_nan", "c_nan", "c_inf",
                    "c_huge", "tree_nan", "mixed")
DEGENERATE_SMALL_KINDS = ("neg", "rad_inf", "c_nan")
_MIXED = ("neg", "zero", "denorm", "rad_inf", "rad_ninf", "rad_nan", "c_nan", "c_inf", "c_huge")


def degenerate_base_rows(n=DEGENERATE_N):
    return cloud_rows(n, 7, _SMALL_HALF, _SMALL_EXP)


def _degenerate_edit(rows, kind, idx):
    """Edit `kind` on the spheres `idx` of rows, in place."""
    j = np.arange(len(idx))
    if kind == "neg":
        rows[idx, 0] *= f32(-4.0)
    elif kind == "zero":
        rows[idx, 0] = 0.0
    elif kind == "denorm":
        rows[idx, 0] = f32(1e-40)
    elif kind == "rad_inf":
        rows[idx, 0] = np.inf
    elif kind == "rad_ninf":
        rows[idx, 0] = -np.inf
    elif kind == "rad_nan":
        rows[idx, 0] = np.nan
    elif kind == "c_nan":
        rows[idx, 1 + j % 3] = np.nan
    elif kind == "c_inf":
        rows[idx, 1 + j % 3] = np.where(j % 2 == 0, np.inf, -np.inf).astype(f32)
    elif kind == "c_huge":
        # centre 3.4e38 on one axis, sign alternating; every second one with a
        # radius large enough that c + rad overflows (the others' boxes are finite)
        rows[idx, 1 + j % 3] = np.where(j % 4 < 2, 3.4e38, -3.4e38).astype(f32)
        rows[idx[1::2], 0] = f32(1e36)
    else:
        raise KeyError(kind)


def degenerate_rows(kind, n=DEGENERATE_N):
    rows = degenerate_base_rows(n)
    idx = DEGENERATE_IDX if n == DEGENERATE_N else DEGENERATE_SMALL_IDX
    if kind == "neg_all":
        rows[4:, 0] = -rows[4:, 0]
    elif kind == "tree_nan":
        rows[4:, 1:4] = np.nan
    elif kind == "mixed":
        for k, name in enumerate(_MIXED):
            _degenerate_edit(rows, name, idx[k::len(_MIXED)])
    else:
        _degenerate_edit(rows, kind, idx)
    return rows


def degenerate(kind):
    """The 300-sphere small cloud (a hierarchy scene) with edit `kind`."""
    return pack(degenerate_rows(kind))


def degenerate_base():
    return pack(degenerate_base_rows())


def degenerate_small(kind):
    """The same edits on 12 of the cloud's first 40 spheres: scanned in full."""
    return pack(degenerate_rows(kind, DEGENERATE_SMALL_N))


degenerate_camera = small_camera


def nonfinite_colours():
    """The 40-sphere cloud with the emitter (inf, 3e38, 20), every other
    emitter off and a zero channel in every diffuse colour: inf x 0 puts NaNs
    into the accumulators, 3e38 sums overflow to inf."""
    rows = degenerate_base_rows(DEGENERATE_SMALL_N)
    rows[1, 4:7] = [np.inf, 3e38, 20.0]
    rows[2:4, 4:7] = 0.0
    rows[2:4, 7:10] = 0.5
    diff = np.flatnonzero(rows[:, 10] == DIFF)
    diff = diff[diff != 1]
    rows[diff, 7 + diff % 3] = 0.0
    return pack(rows)


EDGE_SCENES = {
    "no_always": (lambda: no_always(), no_always_camera),
    "many_always": (lambda: many_always()[0], many_always_camera),
    "n256": (n256, small_camera),
    "coincident": (coincident, coincident_camera),
}
