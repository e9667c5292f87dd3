"""CPU checks of the hierarchy refit (csrc/spt_refit.h) through
tests/native/spt_refit_check.cpp: on eight scenes covering leaf sizes 8, 12
and 16 and the scene without an 8-wide tree,

  * a refit with the unchanged spheres reproduces, byte for byte, the five
    sections the builders of csrc/spt_bvh.h produce (node records of the eight
    octant layouts, geo, ids, wide words, highest-index table);
  * after each of five edits every box contains what it must (asserted in long
    double by the native check), and what a refit must not touch is unchanged;
  * scalar restatements of the 8-wide and binary walks over the refitted
    sections find the full scan's (t, id) for 20,000 random rays per scene and
    edit, nearest hits and counted shadow queries.

tests/test_gpu_scene_update.py compares the device kernels with this host
refit byte for byte."""
import numpy as np
import pytest

import refit_check as rc

NRAYS = 20000


@pytest.fixture(scope="module")
def world():
    """Per scene: (spheres, n, raw rows, Host with the builders' sections,
    those sections).  Built on first use, shared by every test; a test
    refits the Host and leaves it refitted (a refit depends on the spheres it
    is given alone)."""
    cache = {}

    def get(name):
        if name not in cache:
            S, n = rc.SCENES[name]()
            host = rc.Host(S, n)
            cache[name] = (S, n, rc.raw_rows(S, n), host, {k: v.copy() for k, v in host.sections().items()})
        return cache[name]

    yield get
    for v in cache.values():
        v[3].close()


@pytest.mark.parametrize("name", list(rc.SCENES))
def test_layout_class(world, name):
    """Each scene lands in the layout its name says (leaf 8 / 12 / 16, none)."""
    host = world(name)[3]
    assert host.leaf_max == rc.LEAF[name]
    assert (host.wnodes > 0) == (rc.LEAF[name] > 0)
    assert host.nodes > 0 and host.nb + host.na == world(name)[1]


@pytest.mark.parametrize("name", list(rc.SCENES))
def test_identity(world, name):
    """Refit with the unchanged spheres: the builders' bytes."""
    S, n, rows, host, built = world(name)
    got = host.refit(S).sections()
    for k in rc.SECTIONS:
        a, b = got[k].view(np.uint32), built[k].view(np.uint32)
        assert a.shape == b.shape
        assert (a == b).all(), "%s: %d words differ, first at %s" % (k, (a != b).sum(), np.argwhere(a != b)[0])
    assert host.check() == (0, "")


def test_identity_without_a_wide_tree(world):
    """The binary sections alone (RT_SPT_WIDE=0)."""
    S, n = world("cloud3000")[:2]
    host = rc.Host(S, n, wide=False)
    try:
        built = {k: v.copy() for k, v in host.sections().items()}
        assert host.wnodes == 0 and built["wide"].size == 0
        got = host.refit(S).sections()
        for k in rc.SECTIONS:
            assert (got[k].view(np.uint32) == built[k].view(np.uint32)).all(), k
    finally:
        host.close()


@pytest.mark.parametrize("k", rc.EDITS)
@pytest.mark.parametrize("name", list(rc.SCENES))
def test_edit(world, name, k):
    S, n, rows, host, built = world(name)
    new = rc.edit(k, rows, built["ids"], host.nb)
    assert (new != rows).any()
    got = host.refit(rc.from_raw(new)).sections()
    bad, msg = host.check()
    assert bad == 0, msg
    # kept: links, ids, child words, valid masks, highest indices
    assert (got["nodes"][0::2, 3].view(np.uint32) == built["nodes"][0::2, 3].view(np.uint32)).all()
    assert (got["ids"] == built["ids"]).all() and (got["maxid"] == built["maxid"]).all()
    assert (got["wide"][:, 8:16] == built["wide"][:, 8:16]).all()
    assert (got["wide"][:, 3] >> 24 == built["wide"][:, 3] >> 24).all()
    assert (got["wide"][:, 6:8] == 0).all()
    # geo: (p, rad * rad) of the edited spheres in hierarchy order
    want = np.concatenate([new[got["ids"], 1:4], (new[got["ids"], 0] * new[got["ids"], 0])[:, None]], 1)
    assert (got["geo"].view(np.uint32) == want.astype(np.float32).view(np.uint32)).all()
    if k in (2, 3) and host.wnodes:
        e_new = np.stack([(got["wide"][:, 3] >> s) & 255 for s in (0, 8, 16)], 1).astype(int)
        e_old = np.stack([(built["wide"][:, 3] >> s) & 255 for s in (0, 8, 16)], 1).astype(int)
        if k == 2:      # the root's frame grows on every axis
            assert (e_new[0] > e_old[0]).all(), (e_new[0], e_old[0])
        else:           # no frame grows; a node of spheres sharing one centre spans radii alone: it shrinks
            assert (e_new <= e_old).all()
            assert name != "coincident" or (e_new < e_old).any()
    # the walks over the refitted sections against the full scan
    tree = got["ids"][:host.nb]
    cen = new[tree, 1:4].astype(np.float64)
    half = float(((cen.max(0) - cen.min(0)) / 2).max())
    lo, hi = np.percentile(cen, 5, axis=0), np.percentile(cen, 95, axis=0)
    core = max(float((hi - lo).max()) / 2, 1e-3)          # (edit 2's far sphere aside)
    rng = np.random.default_rng([30, k])
    r = rc.rays(rng, cen, tuple(np.median(cen, axis=0) + [0.03 * core, 0.07 * core, 0.8 * core]), NRAYS, 0.1 * core)
    bad, ts, ids = host.walk(r)
    assert bad == 0
    assert (ids >= 0).any(), "the rays must hit something"
    maxt = np.where(ids >= 0, ts * np.float32(1.5), np.float32(max(half, 1.0))).astype(np.float32)
    bad, _, occ = host.walk(r, maxt)
    assert bad == 0
    assert (occ >= 0).any()
