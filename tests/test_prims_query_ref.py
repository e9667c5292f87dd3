"""CPU checks around the level-pass tracers' ray queries (rtp_query_async):
the contract's "a bound is a filter on the unbounded nearest hit" equals the
oracle's own loop started at the bound (tests/prims_query_ref.py pinned on the
reference, not on the code under test); the position -> primitive mapping of
the shadow loop; the header and the Python surface; the argument errors that
need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import prims_query_ref as Q
import prims_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = F(np.inf), F(np.nan)


def scenes(tracer):
    P, n = O.whitted_scene() if tracer == "whitted" else O.queue_scene()
    assert n == 17
    return (("reference", Q.scene_of(P, n, tracer)), ("64 primitives", Q.big_scene(tracer)))


def same(what, got, want):
    for name, g, w in zip(("dist bits", "prim", "result"), got, want):
        g = g.view(np.uint32) if g.dtype == F else g
        w = w.view(np.uint32) if w.dtype == F else w
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, "%s %s: %d differ, first at %d: %r, loop from the bound %r" % (
            what, name, bad.size, bad[0], g[bad[0]], w[bad[0]])


@pytest.mark.parametrize("tracer", ["whitted", "queue"])
def test_filter_equals_the_loop_started_at_the_bound(tracer):
    """For B <= far: the unbounded nearest hit, kept when its distance is < B,
    is what the oracle's loop returns when its distance to beat starts at B --
    hit for hit, with the distance's bits, the primitive and HIT / INPRIM.
    Random bounds, and B exactly at the hit distance (a miss), one float above
    (a hit), one below, 0, negative, far itself and NaN."""
    far = Q.FAR[tracer]
    for name, scene in scenes(tracer):
        rays = Q.ray_set(scene, 160, 7)
        n = len(rays)
        t, ids, res = Q.query(scene, rays, tracer, "nearest")
        hit = ids >= 0
        assert hit.sum() > n // 4 and (~hit).sum() > 4 and (res == -1).sum() > 8, (name, hit.sum(), (res == -1).sum())
        assert (t[~hit] == far).all() and (res[~hit] == 0).all()
        rng = np.random.default_rng(11)
        with np.errstate(all="ignore"):
            bounds = {
                "random": np.minimum(rng.uniform(0.0, 60.0, n).astype(F), far),
                "random around the hit": np.minimum(t * rng.uniform(0.5, 1.5, n).astype(F), far),
                "at the hit": t.copy(),
                "one float above": np.minimum(np.nextafter(t, INF), far),
                "one float below": np.nextafter(t, -INF),
                "zero": np.zeros(n, F),
                "negative": np.full(n, -3.0, F),
                "far": np.full(n, far, F),
                "NaN": np.full(n, NAN, F),
            }
        for bname, B in bounds.items():
            with np.errstate(invalid="ignore"):
                assert (B <= far).all() or bname == "NaN"
            ft, fi, fr = Q.query(scene, rays, tracer, "nearest", tmax=B)
            ld, lp, lr = Q.loop_from(scene, rays, B, tracer)
            fhit = fi >= 0
            assert ((lp >= 0) == fhit).all(), (name, bname, np.flatnonzero((lp >= 0) != fhit)[:8])
            same("%s %s, %s" % (tracer, name, bname), (ft[fhit], fi[fhit], fr[fhit]), (ld[fhit], lp[fhit], lr[fhit]))
            # a miss: the public values, whatever the loop's start was
            assert (ft[~fhit] == far).all() and (fi[~fhit] == -1).all() and (fr[~fhit] == 0).all()
            if bname == "at the hit":
                assert not fhit.any()
            if bname in ("one float above", "far"):
                assert (fhit == hit).all()
            if bname in ("zero", "negative", "NaN", "one float below"):
                assert not fhit.any() or bname == "one float below"


@pytest.mark.parametrize("tracer", ["whitted", "queue"])
def test_occluder_is_the_first_in_index_order(tracer):
    """OCCLUDER's index is the occluder the reference's loop breaks at -- found
    here by walking the primitives themselves, lights skipped -- and SHADOW is
    (OCCLUDER != -1)."""
    f = R._intersect(tracer)
    for name, scene in scenes(tracer):
        rays = Q.ray_set(scene, 120, 3)
        lens = Q.shadow_lengths(scene, rays, tracer, 5)
        occ = Q.query(scene, rays, tracer, "occluder", tmax=lens)
        sh = Q.query(scene, rays, tracer, "shadow", tmax=lens)
        assert ((occ != -1) == (sh == 1)).all() and (sh == 1).sum() > 10 and (sh == 0).sum() > 10
        P = scene.prims(tracer)
        rr, base = R._rays(rays)
        d = C.c_float()
        for i in range(len(rr)):
            want = -1
            for s in range(scene.n):
                if not scene.occluder[s]:
                    continue
                d.value = lens[i]
                if f(P[s], base + 24 * i, d):
                    want = s
                    break
            assert occ[i] == want, (name, i, occ[i], want)


def test_header_and_python_surface():
    src = open(os.path.join(ROOT, "include", "rt_hip.h")).read()
    assert "level-pass tracers, ray queries" in src
    for name, val in (("RTP_QUERY_NEAREST", 0), ("RTP_QUERY_SHADOW", 1), ("RTP_QUERY_OCCLUDER", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), src), name
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"int\s+rtp_query_async\(const rtp_scene \*scene, const float \*d_rays, const float \*d_tmax, "
                     r"size_t nrays, int kind,\s*float \*d_t, int \*d_id, int \*d_result, void \*stream\);", code)
    import rtamd
    for name in ("rtw_prims_create", "rtq_prims_create", "rtp_scene_destroy", "rtw_prims_set_async",
                 "rtq_prims_set_async", "rtp_query_async"):
        assert name in rtamd._lib.EXPORTS and re.search(r"\b%s\(" % name, code), name
    assert (rtamd.RTP_QUERY_NEAREST, rtamd.RTP_QUERY_SHADOW, rtamd.RTP_QUERY_OCCLUDER) == (0, 1, 2)
    assert rtamd.PrimScene.QUERY_KINDS == {"nearest": 0, "shadow": 1, "occluder": 2}
    assert {k: F(v) for k, v in rtamd.PrimScene.FAR.items()} == Q.FAR
    with pytest.raises(ValueError):
        rtamd.PrimScene(None, 1, tracer="smallpt")


def test_argument_errors_need_no_device():
    """Every check that needs no device comes before the first device call:
    each fails RT_ERR_INVALID and names itself in rt_last_error."""
    import rtamd
    L = rtamd.lib()
    buf = (C.c_float * 6)()
    out = (C.c_int * 1)()
    a, o = C.addressof(buf), C.addressof(out)

    def invalid(rc, text):
        assert rc == rtamd._lib.RT_ERR_INVALID
        assert text in L.rt_last_error(), L.rt_last_error()

    q = L.rtp_query_async
    for kind in (-1, 3, 7):
        invalid(q(None, a, a, 1, kind, None, o, None, None), b"unknown kind")
    invalid(q(None, a, a, 1, 0, None, None, None, None), b"no output")
    for kind in (1, 2):
        invalid(q(None, a, None, 1, kind, None, o, None, None), b"needs d_tmax and d_id")
        invalid(q(None, a, a, 1, kind, a, None, o, None), b"needs d_tmax and d_id")
    invalid(q(None, a, a, 2 ** 31, 0, None, o, None, None), b"too many rays")
    for kind in (0, 1, 2):
        invalid(q(None, a, a, 1, kind, None, o, None, None), b"null scene or rays")
        invalid(q(None, a, a, 0, kind, None, o, None, None), b"null scene or rays")
    handle = C.c_void_p()
    prims = (rtamd.Primitive * 65)()
    qprims = (rtamd.QPrimitive * 65)()
    for create, arr in ((L.rtw_prims_create, prims), (L.rtq_prims_create, qprims)):
        name = b"rtw_prims_create" if arr is prims else b"rtq_prims_create"
        for n in (0, -1, 65):
            invalid(create(C.addressof(arr), n, C.byref(handle)), name)
        invalid(create(None, 1, C.byref(handle)), name)
        invalid(create(C.addressof(arr), 1, None), name)
        assert not handle.value
    for setter, name in ((L.rtw_prims_set_async, b"rtw_prims_set_async"), (L.rtq_prims_set_async, b"rtq_prims_set_async")):
        invalid(setter(None, C.addressof(prims), 1, None), name)
    assert L.rtp_scene_destroy(None) == 0
    for tracer in ("whitted", "queue"):
        with pytest.raises(rtamd.RTError):
            rtamd.PrimScene(None, 1, tracer=tracer)
