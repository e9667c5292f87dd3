"""CPU only.  The scenes of tests/degenerate_prims.py -- primitives with NaN,
infinite, zero, negative and huge fields, unknown `type`s and light flags --
are a domain on which the oracle is still the reference:

1. every catalogue case and every fuzz seed renders the same frame through
   the oracle and through the reference's own code (oracle/_ref: Engine_Render,
   raytrace_kernel compiled as host C++, raytracer_non_kernel), all pixels.
   These skip where oracle/_ref is not built;
2. every catalogue kind reaches the camera: it changes the oracle's frame or
   counters against the unedited scene, unless NO_OP_KINDS says why it cannot
   -- and then it changes nothing;
3. every fuzz seed's oracle frame meets lit_scenes.check_lit.
"""
import numpy as np
import pytest

import degenerate_prims as D
import lit_scenes as L
import oracle_lib as O


def _need_ref_whitted():
    libs = O.ref_libs()
    if libs is None or not (hasattr(libs[0], "ref_whitted_render") and hasattr(libs[0], "ref_whitted_render_ocl")):
        pytest.skip("oracle/_ref not built (no reference tree at build time)")


def _same(ref, got, what):
    msg = D.first_difference(ref, got)
    assert msg is None, "%s: %s (want: the reference build, got: the oracle)" % (what, msg)


# ---------------------------------------------------------------- the catalogue is complete and aimed
def test_catalogue_covers_the_field_families():
    for tracer, kinds in (("whitted", D.WHITTED_KINDS), ("queue", D.QUEUE_KINDS)):
        names = [k[0] for k in kinds]
        assert len(set(names)) == len(names)
        for base in ("ref", "lit"):
            assert sorted(D.AIM[tracer][base]) == sorted(names)
        assert {k.split("-")[-1] for k in D.NO_OP_KINDS[tracer]} < set(names)
        assert all("-" not in k or k.split("-")[0] in ("ref", "lit") for k in D.NO_OP_KINDS[tracer])
        for stem in ("centre", "radius", "rradius", "sqradius"):
            assert {stem + "_nan", stem + "_inf", stem + "_zero"} <= set(names), stem
        for name in ("centre_neg", "rradius_neg", "sqradius_neg", "radius_sign", "normal_zero", "normal_nan",
                     "normal_times5", "colour_inf", "colour_nan", "colour_neg", "colour_huge", "rindex_zero",
                     "rindex_nan", "rindex_neg", "refl_nan", "refl_inf", "refr_nan", "refr_inf", "diff_neg",
                     "spec_nan", "spec_inf", "spec_neg", "light_centre_nan", "light_centre_inf", "light_colour_nan",
                     "type_minus7", "light_flag_2", "plane_light"):
            assert name in names, (tracer, name)
    w = [k[0] for k in D.WHITTED_KINDS]
    assert {"plane_d_nan", "type_0", "type_3", "light_flag_minus1"} <= set(w)
    assert {"depth_nan", "type_2"} <= {k[0] for k in D.QUEUE_KINDS}


def test_edits_write_the_fields_they_name():
    words, _ = D._whitted_base("ref")
    e = D.prims_of(O.Primitive, D.apply_kind("whitted", words, "colour_neg", 9))
    assert e[9].m_Color.y == -3.0 and e[9].m_Color.x == 1.0 and e[9].plane_D == np.float32(5.4)
    e = D.prims_of(O.Primitive, D.apply_kind("whitted", words, "radius_inf", 2))
    assert e[2].m_SqRadius == np.inf and e[2].m_Radius == np.inf and e[2].m_RRadius == 0.0
    e = D.prims_of(O.Primitive, D.apply_kind("whitted", words, "type_minus7", 2))
    assert e[2].type == -7 and e[2].m_Light == 0
    e = D.prims_of(O.Primitive, D.apply_kind("whitted", words, "centre_nan", 2))
    assert np.isnan(e[2].m_Centre.x) and e[2].m_Centre.y == np.float32(-3.4)
    words, _ = D._queue_base("ref")
    e = D.prims_of(O.QPrimitive, D.apply_kind("queue", words, "light_flag_2", 13))
    assert e[13].is_light == 2 and e[13].type == 1 and bytes(e[13].pad_) == bytes(3)
    e = D.prims_of(O.QPrimitive, D.apply_kind("queue", words, "radius_zero", 1))
    assert e[1].radius == 0 and e[1].sq_radius == 0 and e[1].r_radius == np.inf
    e = D.prims_of(O.QPrimitive, D.apply_kind("queue", words, "normal_times5", 0))
    assert (e[0].normal.x, e[0].normal.y, e[0].normal.z) == (0.0, 3.75, 0.0)


def test_fuzz_touches_float_words_only():
    assert len(D.FUZZ_WORDS["whitted"]) == 18 and len(D.FUZZ_WORDS["queue"]) == 21
    for tracer, base in (("whitted", D._whitted_base), ("queue", D._queue_base)):
        words, _ = base("lit")
        changed = np.zeros(D.WORDS, bool)
        for seed in range(40):
            f = D.fuzz(tracer, words, seed)
            assert f.shape == words.shape and (f != words).any()
            changed |= (f != words).any(0)
            assert (D.fuzz(tracer, words, seed) == f).all()
        assert sorted(np.nonzero(changed)[0]) == D.FUZZ_WORDS[tracer]
        share = np.mean([(D.fuzz(tracer, words, s)[:, D.FUZZ_WORDS[tracer]] != words[:, D.FUZZ_WORDS[tracer]]).mean()
                         for s in range(40)])
        assert 0.02 < share < 0.05, share        # rate 0.04, less the draws that restate the old word


@pytest.mark.parametrize("case", D.WHITTED_CATALOGUE)
def test_whitted_kind_reaches_the_camera(case):
    base, _, kind = case.partition("-")
    _, _, _, _, cpu0, ocl0 = D.whitted_case(base)
    _, _, _, _, cpu, ocl = D.whitted_case(case)
    same = [(a[0] == b[0]).all() and a[1] == b[1] for a, b in ((cpu0, cpu), (ocl0, ocl))]
    if D.no_op_reason("whitted", case):
        assert all(same), D.no_op_reason("whitted", case)
    else:
        assert not any(same), "aimed at a primitive the camera does not see (unchanged: CPU %s, OpenCL %s)" % tuple(
            same)


@pytest.mark.parametrize("case", D.QUEUE_CATALOGUE)
def test_queue_kind_reaches_the_camera(case):
    base, _, kind = case.partition("-")
    _, _, _, _, f0, c0 = D.queue_case(base)
    _, _, _, _, f, c = D.queue_case(case)
    same = (f0 == f).all() and c0 == c
    if D.no_op_reason("queue", case):
        assert same, D.no_op_reason("queue", case)
    else:
        assert not same, "aimed at a primitive the camera does not see"


def test_negative_colour_reaches_the_pack():
    """openCLcode.cl:245 ORs the channels, raytracer.cpp:523 adds them.  A
    negative green channel, shifted, has every bit above it set: the ORed
    word keeps them all (0xffff.... whatever red is), a sum keeps them only
    where red is 0.  The colour_neg cases must put such words into the
    OpenCL-semantics frame, and none into the CPU-semantics one where red is
    not 0 -- so a frame packed the other way is not the reference's."""
    for case in ("ref-colour_neg", "lit-colour_neg"):
        _, _, _, _, (cpu, _), (ocl, _) = D.whitted_case(case)
        assert ((ocl >> 16) == 0xffff).sum() > 1000, case
        assert ((ocl >> 24) != 0).sum() > ((cpu >> 24) != 0).sum(), case


# ---------------------------------------------------------------- the fuzz seeds are lit
def test_fuzz_seed_lists():
    assert len(D.WHITTED_FUZZ_SEEDS) == 12 and len(set(D.WHITTED_FUZZ_SEEDS)) == 12
    assert len(D.QUEUE_FUZZ_SEEDS) == 10 and len(set(D.QUEUE_FUZZ_SEEDS)) == 10
    rpp = {s: D.whitted_rays_per_primary("fuzz-%d" % s) for s in D.WHITTED_FUZZ_SEEDS}
    assert tuple(sorted(rpp, key=rpp.get, reverse=True)[:2]) == D.WHITTED_FUZZ_DEEP, rpp
    rpp = {s: D.queue_rays_per_primary("fuzz-%d" % s) for s in D.QUEUE_FUZZ_SEEDS}
    assert tuple(sorted(rpp, key=rpp.get, reverse=True)[:2]) == D.QUEUE_FUZZ_DEEP, rpp


@pytest.mark.parametrize("case", D.WHITTED_FUZZ)
def test_whitted_fuzz_seed_is_lit(case):
    _, n, w, h, (cpu, _), (ocl, _) = D.whitted_case(case)
    wc, wo = L.whitted_windows(w, h)
    assert w * h <= 40000
    L.check_lit(cpu, wc[:2])
    L.check_lit(ocl, wo[:2])


@pytest.mark.parametrize("case", D.QUEUE_FUZZ)
def test_queue_fuzz_seed_is_lit(case):
    _, n, w, h, frame, cnt = D.queue_case(case)
    assert (w, h) == (L.QUEUE_W, L.QUEUE_H)
    L.check_lit(frame)
    # no ray of the listed seeds leaves the scene or hits a light with
    # children: the reference reads no uninitialised point there
    assert cnt[3] == 0


# ---------------------------------------------------------------- oracle == reference build
@pytest.mark.parametrize("case", D.WHITTED_CASES)
def test_whitted_oracle_is_the_reference_engine(case):
    _need_ref_whitted()
    P, n, w, h, (cpu, _), (ocl, _) = D.whitted_case(case)
    assert w * h <= 40000
    _same(O.ref_whitted_render(w, h, P, n), cpu, case + " (Engine_Render)")
    _same(O.ref_whitted_render_ocl(w, h, P, n), ocl, case + " (raytrace_kernel)")


@pytest.mark.parametrize("case", D.QUEUE_CASES)
def test_queue_oracle_is_the_reference_build(case):
    Q = O.ref_queue_lib()
    if Q is None:
        pytest.skip("oracle/_ref not built (no reference tree at build time)")
    P, n, w, h, frame, _ = D.queue_case(case)
    assert w * h <= 40000
    _same(O.ref_queue_render(Q, w, h, P, n), frame, case)
