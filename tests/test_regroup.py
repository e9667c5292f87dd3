"""CPU checks of the hierarchy regroup (csrc/spt_regroup.h) through
tests/native/spt_regroup_check.cpp, on refit_check's nine scenes:

  * after an edit and regroup_host every box contains what it must, both
    scalar walks find the full scan's (t, id) -- nearest, any and highest
    occluder --, the tree entries are a permutation of what they were, the
    always entries are untouched and the highest-index table is what a direct
    recomputation gives;
  * a second regroup changes nothing where no two centres tie along a split;
  * (radius, centre) permuted among the tree spheres, then refit + regroup,
    gives back the builders' node and wide sections byte for byte: the
    definition is the builder's partition;
  * on that scene the regroup brings the summed surface area of the node boxes
    back down from the refit's;
  * negative, zero and non-finite radii and centres keep all of the above.

tests/test_gpu_regroup.py compares the device kernels with this host regroup
byte for byte."""
import numpy as np
import pytest

import refit_check as rc
import regroup_check as rg
import scenes_layouts as sl

NRAYS = 20000


@pytest.fixture(scope="module")
def world():
    """Per scene: (spheres, n, raw rows, the builders' sections).  Built on
    first use and left unchanged; every test makes the Host it edits."""
    cache = {}

    def get(name):
        if name not in cache:
            S, n = rc.SCENES[name]()
            host = rg.Host(S, n)
            cache[name] = (S, n, rc.raw_rows(S, n), {k: v.copy() for k, v in host.sections().items()})
            host.close()
        return cache[name]

    return get


def walks(host, rows, ids, seed):
    """Both walks over the host's sections against the full scan of `rows`."""
    cen = rows[ids[:host.nb], 1:4].astype(np.float64)
    cen = cen[np.isfinite(cen).all(1) & (np.abs(cen) < 1e30).all(1)]
    half = float(((cen.max(0) - cen.min(0)) / 2).max())
    lo, hi = np.percentile(cen, 5, axis=0), np.percentile(cen, 95, axis=0)
    core = max(float((hi - lo).max()) / 2, 1e-3)
    rng = np.random.default_rng([40, seed])
    r = rc.rays(rng, cen, tuple(np.median(cen, axis=0) + [0.03 * core, 0.07 * core, 0.8 * core]), NRAYS, 0.1 * core)
    bad, ts, hit = host.walk(r)
    assert bad == 0
    assert (hit >= 0).any(), "the rays must hit something"
    maxt = np.where(hit >= 0, ts * np.float32(1.5), np.float32(max(half, 1.0))).astype(np.float32)
    bad, _, occ = host.walk(r, maxt)                   # any hit and the highest occluder (the counted walk)
    assert bad == 0
    assert (occ >= 0).any()


def regrouped_ok(host, rows, before, seed):
    """The properties of a regroup of `rows` on a host whose ids were `before`."""
    got = host.sections()
    bad, msg = host.check()
    assert bad == 0, msg
    nb = host.nb
    assert (np.sort(got["ids"][:nb]) == np.sort(before[:nb])).all()
    assert (got["ids"][nb:] == before[nb:]).all()
    if host.wnodes:
        assert (got["maxid"] == rg.maxid_direct(got)).all()
    ids = got["ids"]
    with np.errstate(over="ignore"):                   # (a huge radius squares to inf, as on the device)
        want = np.concatenate([rows[ids, 1:4], (rows[ids, 0] * rows[ids, 0])[:, None]], 1).astype(np.float32)
    assert (got["geo"].view(np.uint32) == want.view(np.uint32)).all()
    walks(host, rows, ids, seed)
    return got


@pytest.mark.parametrize("name", list(rc.SCENES))
def test_edits_then_regroup(world, name):
    """Edit 1, regroup, edit 5, regroup: containment, walks, permutation, maxid."""
    S, n, rows, built = world(name)
    host = rg.Host(S, n)
    try:
        ids = built["ids"]
        for k in (1, 5):
            new = rc.edit(k, rows, built["ids"], host.nb)
            host.regroup(rc.from_raw(new))
            got = regrouped_ok(host, new, ids, k)
            # frozen: links, child words, valid masks
            assert (got["nodes"][0::2, 3].view(np.uint32) == built["nodes"][0::2, 3].view(np.uint32)).all()
            assert (got["wide"][:, 8:16] == built["wide"][:, 8:16]).all()
            assert (got["wide"][:, 3] >> 24 == built["wide"][:, 3] >> 24).all()
            ids = got["ids"]
    finally:
        host.close()


def test_regroup_without_a_wide_tree(world):
    """The binary sections alone (RT_SPT_WIDE=0): no highest-index table to rewrite."""
    S, n, rows, _ = world("cloud3000")
    host = rg.Host(S, n, wide=False)
    try:
        before = host.sections()["ids"].copy()
        new = rc.edit(1, rows, before, host.nb)
        host.regroup(rc.from_raw(new))
        got = regrouped_ok(host, new, before, 1)
        assert got["wide"].size == 0 and got["maxid"].size == 0
    finally:
        host.close()


# `coincident` is left out: its spheres share centres, so along every split
# whole groups of keys tie.  A stable sort keeps tied entries in the order in
# which they arrive, the deeper levels of one regroup reorder them, and where
# such a group straddles a child boundary the next regroup deals its members
# to the two children differently.  Both results are valid trees; they are not
# the same bytes.
@pytest.mark.parametrize("name", [k for k in rc.SCENES if k != "coincident"])
def test_second_regroup_changes_nothing(world, name):
    S, n, rows, built = world(name)
    host = rg.Host(S, n)
    try:
        new = rc.from_raw(rc.edit(1, rows, built["ids"], host.nb))
        first = {k: v.copy() for k, v in host.regroup(new).sections().items()}
        assert rg.first_difference(host.regroup(new).sections(), first) == ""
    finally:
        host.close()


# The scenes on which the identity below holds (checked on the CPU when this
# test was written): the builder split every inner node by its bins (no n / 2
# fallback) and no two centres tie across a child boundary.  Every scene but
# `coincident` (shared centres: ties across boundaries; its regrouped boxes sum
# to 13,269 against the builders' 13,215).
IDENTITY_SCENES = tuple(k for k in rc.SCENES if k != "coincident")


@pytest.mark.parametrize("name", IDENTITY_SCENES)
def test_permuted_scene_regroups_to_the_builders_tree(world, name):
    """The identity that pins the definition to the builder: the point set is
    the same, and at every node the builder's `bin < best_b` partition is the
    lowest mid - lo centres along the axis -- so dealing the permuted spheres
    back by the definition gives the builders' boxes, in every section that
    holds boxes, and the same entries up to the permutation.  Also the quality
    condition: the refit alone leaves far larger boxes than the regroup."""
    S, n, rows, built = world(name)
    host = rg.Host(S, n)
    try:
        nb = host.nb
        fresh = host.area()
        new, perm = rg.permuted(rows, built["ids"], nb)
        arr = rc.from_raw(new)
        host.refit(arr)
        refit_only = host.area()
        refitted = host.sections()
        assert (refitted["nodes"].view(np.uint32) != built["nodes"].view(np.uint32)).any()
        got = host.regroup(arr).sections()
        regrouped = host.area()
        print("%s: summed box area fresh %.6g refit only %.6g regrouped %.6g" % (name, fresh, refit_only, regrouped))
        for k in ("nodes", "wide"):
            a, b = got[k].view(np.uint32), built[k].view(np.uint32)
            assert (a == b).all(), "%s: %d words differ, first at %s" % (k, (a != b).sum(), np.argwhere(a != b)[0])
        # geo: the always entries as they were; the tree entries the same rows, leaf by leaf up to their order
        assert (got["geo"][nb:].view(np.uint32) == built["geo"][nb:].view(np.uint32)).all()

        def canon(g):
            g = g[:nb].view(np.uint32)
            return g[np.lexsort(g.T[::-1])]
        assert (canon(got["geo"]) == canon(built["geo"])).all()
        assert (np.sort(got["ids"][:nb]) == np.sort(built["ids"][:nb])).all()
        assert refit_only > 2.0 * fresh, "the permutation must stretch the refitted boxes"
        assert regrouped < refit_only
        assert regrouped == fresh
    finally:
        host.close()


@pytest.mark.parametrize("kind", sl.DEGENERATE_KINDS)
def test_degenerate_floats(world, kind):
    """Update to a degenerate kind, regroup: containment, walks, permutation,
    maxid.  The key path is integer alone (no conversion of a NaN: the
    stand-alone build of the native check runs under the sanitizers)."""
    S, n, rows, built = world("degenerate")
    host = rg.Host(S, n)
    try:
        S2, n2 = sl.degenerate(kind)
        assert n2 == n
        new = rc.raw_rows(S2, n2)
        host.regroup(S2)
        regrouped_ok(host, new, built["ids"], sl.DEGENERATE_KINDS.index(kind))
    finally:
        host.close()


def test_plan(world):
    """The launch plan: with the LDS tier at 4,096 entries a tree within them
    is one subtree and no global level; at the library's size the top levels
    are global and the rest subtrees; without the tier every level that holds
    an inner node is a global one."""
    S, n, _, _ = world("cloud3000")
    host = rg.Host(S, n)
    try:
        levels, glob, subs = host.plan(4096)
        assert glob == 0 and subs == 1 and levels > 1
        levels0, glob0, subs0 = host.plan(0)
        assert levels0 == levels and glob0 == levels - 1 and subs0 == 0
        levels1, glob1, subs1 = host.plan()
        assert levels1 == levels and 0 < glob1 < glob0 and subs1 > 1
    finally:
        host.close()
    S, n, _, _ = world("n256")
    host = rg.Host(S, n)
    try:
        assert host.plan()[1:] == (0, 1)
    finally:
        host.close()
