"""CPU checks of the hierarchy builders and the refit (csrc/spt_bvh.h,
csrc/spt_refit.h) on degenerate sphere data: negative, zero, denormal and
non-finite radii, non-finite and huge centres (tests/scenes_layouts.py,
degenerate(kind)).  The reference uses a radius only as rad * rad
(smallptgpu-v1.6/geomfunc.h:32-59): a negative radius is its absolute value,
and a sphere with a non-finite radius or centre is never hit.  For every kind,
on a tree built from the kind's scene and on a tree built from the base cloud
and refitted to it,

  * the scalar restatements of the 8-wide and the binary walk
    (tests/native/spt_refit_check.cpp) give the full scan's (t bits, id) for
    20,000 rays, nearest hits and counted shadow queries with maxt = 30;
  * every box contains c -+ |rad| of every sphere of its range whose box is
    finite (the native check, in long double);
  * a refit back to the base spheres reproduces the builders' bytes.

The stand-alone form of the native check runs the same steps on scenes of its
own under the address, undefined-behaviour and float-cast sanitizers."""
import subprocess

import numpy as np
import pytest

import refit_check as rc
import scenes_layouts as sl

NRAYS = 20000
MAXT = np.float32(30.0)


def query_rays():
    """The rays every degenerate test sends (CPU and GPU): origins around the
    base cloud's centres and at one point inside it."""
    centres = sl.degenerate_base_rows()[4:, 1:4].astype(np.float64)
    return rc.rays(np.random.default_rng(3), centres, (1, 2, 4), NRAYS, 1.0)


@pytest.fixture(scope="module")
def world():
    """rays; base spheres; get(kind, wide) -> (spheres of the kind, a Host built
    from them, a Host built from the base cloud, the latter's sections as
    built).  A test leaves the second Host refitted to whatever it likes."""
    rays = query_rays()
    B, n = sl.degenerate_base()
    cache = {}

    def get(kind, wide):
        if (kind, wide) not in cache:
            S, m = sl.degenerate(kind)
            assert m == n
            built, base = rc.Host(S, n, wide=wide), rc.Host(B, n, wide=wide)
            cache[(kind, wide)] = (S, built, base, {k: v.copy() for k, v in base.sections().items()})
        return cache[(kind, wide)]

    yield rays, B, n, get
    for v in cache.values():
        v[1].close()
        v[2].close()


def test_scenes_are_what_they_claim():
    base = sl.degenerate_base_rows()
    idx = sl.DEGENERATE_IDX
    assert len(base) == 300 and len(idx) == 40 and idx[0] == 20 and idx[-1] == 293
    assert (base[:256, :10].view(np.uint32) == sl.rows_of(*sl.n256())[:, :10].view(np.uint32)).all()   # n256 grown to 300
    assert np.isfinite(base[:, :4]).all() and (base[:, 0] > 0).all()
    rest = np.setdiff1d(np.arange(300), idx)
    for kind in sl.DEGENERATE_KINDS:
        rows = sl.degenerate_rows(kind)
        assert (rows[:4].view(np.uint32) == base[:4].view(np.uint32)).all(), kind       # ground and lights
        assert (rows[:, 4:].view(np.uint32) == base[:, 4:].view(np.uint32)).all(), kind   # materials
        if kind not in ("neg_all", "tree_nan"):
            assert (rows[rest].view(np.uint32) == base[rest].view(np.uint32)).all(), kind
            assert (rows[idx, :4].view(np.uint32) != base[idx, :4].view(np.uint32)).any(axis=1).all(), kind
    r = sl.degenerate_rows
    assert (r("neg")[idx, 0] == np.float32(-4) * base[idx, 0]).all()
    assert (r("neg_all")[4:, 0] == -base[4:, 0]).all() and np.median(r("neg_all")[:, 0]) < 0
    assert (r("zero")[idx, 0] == 0).all() and (r("denorm")[idx, 0] == np.float32(1e-40)).all()
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny
    assert (r("rad_inf")[idx, 0] == np.inf).all() and (r("rad_ninf")[idx, 0] == -np.inf).all()
    assert np.isnan(r("rad_nan")[idx, 0]).all()
    assert (np.isnan(r("c_nan")[idx, 1:4]).sum(axis=1) == 1).all()
    assert (np.isinf(r("c_inf")[idx, 1:4]).sum(axis=1) == 1).all()
    huge = r("c_huge")[idx]
    assert ((np.abs(huge[:, 1:4]) == np.float32(3.4e38)).sum(axis=1) == 1).all()
    with np.errstate(over="ignore"):
        over = ~np.isfinite(np.abs(huge[:, 1:4]).max(axis=1) + huge[:, 0])
    assert over.sum() == 20                                     # c + rad overflows on half of them
    assert np.isnan(r("tree_nan")[4:, 1:4]).all()
    mixed = r("mixed")[idx, :4]
    assert (mixed[:, 0] < 0).any() and (mixed[:, 0] == 0).any() and np.isnan(mixed[:, 0]).any()
    assert np.isinf(mixed[:, 0]).sum() >= 8 and np.isnan(mixed[:, 1:4]).any() and np.isinf(mixed[:, 1:4]).any()
    for kind in sl.DEGENERATE_SMALL_KINDS:
        rows = sl.degenerate_rows(kind, sl.DEGENERATE_SMALL_N)
        assert len(rows) == 40 and (rows[sl.DEGENERATE_SMALL_IDX, :4].view(np.uint32)
                                    != base[sl.DEGENERATE_SMALL_IDX, :4].view(np.uint32)).any(axis=1).all()


def _same(got, want, what):
    for k in rc.SECTIONS:
        a, b = got[k].view(np.uint32), want[k].view(np.uint32)
        assert a.shape == b.shape, (what, k)
        assert (a == b).all(), "%s, %s: %d words differ, first at %s" % (what, k, (a != b).sum(), np.argwhere(a != b)[0])


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "binary"])
@pytest.mark.parametrize("kind", sl.DEGENERATE_KINDS)
def test_walks_equal_the_scan(world, kind, wide):
    """Created from the kind and refitted to it: both walks give the scan's
    answers, nearest and counted shadow; every finite sphere box is contained;
    a refit back gives the builders' bytes."""
    rays, B, n, get = world
    S, built, base, base_sections = get(kind, wide)
    assert (built.wnodes > 0) == wide and (base.wnodes > 0) == wide
    rows = sl.degenerate_rows(kind)
    maxt = np.full(NRAYS, MAXT, np.float32)
    for what, host in (("created", built), ("refitted", base.refit(S))):
        assert host.check() == (0, ""), what
        bad, ts, ids = host.walk(rays)
        print(kind, what, "nearest: mismatches", bad, "scan hits", (ids >= 0).sum())
        assert bad == 0, what
        assert (ids >= 0).sum() >= NRAYS // 4, "the scan must hit a quarter of the rays"
        assert np.isfinite(ts[ids >= 0]).all()
        hit = rows[ids[ids >= 0]]
        with np.errstate(invalid="ignore", over="ignore"):
            assert np.isfinite(hit[:, 0] * hit[:, 0]).all() and np.isfinite(hit[:, 1:4]).all(), \
                "a non-finite sphere is never hit"
        if kind == "neg":
            on_neg = (rows[np.maximum(ids, 0), 0] < 0) & (ids >= 0)
            print(kind, what, "rays answered by a negative-radius sphere", on_neg.sum())
            assert on_neg.sum() >= NRAYS // 10
        bad, _, occ = host.walk(rays, maxt)
        print(kind, what, "shadow: mismatches", bad, "occluded", (occ >= 0).sum())
        assert bad == 0, what
        assert (occ >= 0).sum() >= NRAYS // 4
    back = base.refit(B)
    _same(back.sections(), base_sections, "refit back from " + kind)
    assert base.check() == (0, "")


def test_partition_counts_the_radius_by_its_magnitude(world):
    """|rad| decides the always / tree partition: negating every radius moves
    no sphere across it, and the hierarchy order stays."""
    rays, B, n, get = world
    S, built, base, base_sections = get("neg_all", True)
    assert built.na == base.na and built.na >= 1
    assert (built.sections()["ids"] == base_sections["ids"]).all()
    got = built.sections()
    for k in ("nodes", "wide", "maxid"):
        assert (got[k].view(np.uint32) == base_sections[k].view(np.uint32)).all(), k


def test_standalone_check_under_sanitizers(tmp_path):
    """spt_refit_check.cpp's own main (host code, a program of its own): the
    five edits and the degenerate kinds -- build, refit there and back, both
    walks -- under -fsanitize=address,undefined,float-cast-overflow."""
    exe = str(tmp_path / "spt_refit_main")
    san = "address,undefined,float-cast-overflow"
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-fsanitize=" + san,
                    "-fno-sanitize-recover=undefined,float-cast-overflow", "-DSPT_REFIT_MAIN", "-I" + rc.CSRC, rc.SRC,
                    "-o", exe], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    print(p.stdout[-3000:], p.stderr[-3000:])
    assert p.returncode == 0
    lines = p.stdout.splitlines()
    assert sum("degenerate kind" in x for x in lines) == 26 and all("refit back equal" in x for x in lines if "degenerate" in x)
    assert "runtime error" not in p.stderr and "ERROR" not in p.stderr
