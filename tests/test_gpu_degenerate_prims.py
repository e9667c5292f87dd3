"""GPU parity of the Whitted kernels (whitted.hip) and the queue tracer
(queue.hip) on primitives that hold any floats, any `type` and any light
flag: the catalogue and the fuzzed lit scenes of tests/degenerate_prims.py
through rtw_render, rtw_render_ocl and rtq_render against the oracle, which
tests/test_degenerate_prims.py pins to the reference's own code on the same
cases.  Bar: frames bit for bit and all four work counters, on the counted
and the uncounted kernels; the sequential and exact paths (fixup_kernel and
slabs, final_kernel's pool overflow, fix_kernel's exact pow) and the async
entry points on the fuzz seeds with the deepest trees."""
import ctypes as C

import numpy as np
import pytest

import degenerate_prims as D
import lit_scenes as L
import oracle_lib as O

pytestmark = pytest.mark.gpu


def _equal(ref, got, what):
    msg = D.first_difference(ref, got)
    assert msg is None, "%s: %s" % (what, msg)


def _whitted_vs_oracle(rt, case):
    P, n, w, h, (ref, rc), (oref, orc) = D.whitted_case(case)
    assert w * h <= 40000
    got, gc = rt.whitted_render(w, h, prims=P, nprims=n, counters=True)
    _equal(ref, got, case + " counted")
    assert gc == rc, (case, gc, rc)
    _equal(ref, rt.whitted_render(w, h, prims=P, nprims=n), case + " uncounted")
    got, gc = rt.whitted_render_ocl(w, h, prims=P, nprims=n, counters=True)
    _equal(oref, got, case + " OpenCL semantics, counted")
    assert gc == orc, (case, gc, orc)
    _equal(oref, rt.whitted_render_ocl(w, h, prims=P, nprims=n), case + " OpenCL semantics, uncounted")


def _queue_vs_oracle(rt, case):
    P, n, w, h, ref, rc = D.queue_case(case)
    assert w * h <= 40000
    got, gc = rt.queue_render(w, h, P, n, counters=True)
    _equal(ref, got, case + " counted")
    assert gc == rc, (case, gc, rc)
    _equal(ref, rt.queue_render(w, h, P, n), case + " uncounted")


@pytest.mark.parametrize("case", D.WHITTED_CATALOGUE)
def test_whitted_catalogue(rt, case):
    """One degenerate field of one primitive the camera sees, in the
    reference scene and in a lit walled scene."""
    _whitted_vs_oracle(rt, case)


@pytest.mark.parametrize("case", D.WHITTED_FUZZ)
def test_whitted_fuzzed_lit_scenes(rt, case):
    """A lit walled scene with 4 % of its float words replaced by special
    values; the oracle's frame must still be lit before it is compared."""
    _, _, w, h, (ref, _), (oref, _) = D.whitted_case(case)
    wc, wo = L.whitted_windows(w, h)
    L.check_lit(ref, wc[:2])
    L.check_lit(oref, wo[:2])
    _whitted_vs_oracle(rt, case)


@pytest.mark.parametrize("case", D.QUEUE_CATALOGUE)
def test_queue_catalogue(rt, case):
    _queue_vs_oracle(rt, case)


@pytest.mark.parametrize("case", D.QUEUE_FUZZ)
def test_queue_fuzzed_lit_scenes(rt, case):
    L.check_lit(D.queue_case(case)[4])
    _queue_vs_oracle(rt, case)


# ---------------------------------------------------------------- the sequential and exact paths
@pytest.mark.parametrize("seed", D.WHITTED_FUZZ_DEEP)
def test_whitted_fuzz_through_fixup_and_slabs(rt, seed, monkeypatch):
    """Child queues of 1000 items and three interleaved slabs: most trees of
    the deepest fuzzed scenes finish in fixup_kernel's sequential pass."""
    monkeypatch.setenv("RT_WHITTED_QUEUE_CAP", "1000")
    monkeypatch.setenv("RT_WHITTED_SLABS", "3")
    assert D.whitted_rays_per_primary("fuzz-%d" % seed) > 3.0
    _whitted_vs_oracle(rt, "fuzz-%d" % seed)


@pytest.mark.parametrize("cap", ["20000", "150000"])
@pytest.mark.parametrize("case", ["lit-rradius_zero", "lit-rindex_nan"])
def test_whitted_tir_heavy_trees_with_full_lists(rt, case, cap, monkeypatch):
    """A sphere whose every refraction is a total internal reflection (over
    100,000 of them a frame) in pools that hold part of the trees: the TIR
    lists (a 64th of the pool) and the pool overflow while the level pass is
    still tracing the trees' other nodes.  A tree that lost a node must leave
    its later stale-ray children to fixup_kernel, or the level pass traces --
    and counts -- rays the reference never does."""
    monkeypatch.setenv("RT_WHITTED_QUEUE_CAP", cap)
    assert D.whitted_case(case)[4][1][3] > 100000
    _whitted_vs_oracle(rt, case)


@pytest.mark.parametrize("seed", D.QUEUE_FUZZ_DEEP)
def test_queue_fuzz_pool_overflow(rt, seed, monkeypatch):
    """A record pool of 4096 for over a million rays: final_kernel and
    fix_kernel re-evaluate the trees whose nodes did not fit."""
    monkeypatch.setenv("RT_QUEUE_POOL_CAP", "4096")
    assert D.queue_case("fuzz-%d" % seed)[5][0] > 100 * 4096
    _queue_vs_oracle(rt, "fuzz-%d" % seed)


@pytest.mark.parametrize("seed", D.QUEUE_FUZZ_DEEP)
def test_queue_fuzz_exact_path_everywhere(rt, seed, monkeypatch):
    """RT_QUEUE_EXACT_ALL=1: every specular term by rtm::pow_d in fix_kernel,
    with any dot > 0 and any m_spec > 0."""
    monkeypatch.setenv("RT_QUEUE_EXACT_ALL", "1")
    _queue_vs_oracle(rt, "fuzz-%d" % seed)


@pytest.mark.parametrize("case", ["ref-spec_inf", "lit-spec_inf", "ref-normal_times5", "ref-light_colour_nan"])
def test_queue_catalogue_exact_path_everywhere(rt, case, monkeypatch):
    """The kinds that reach the specular factor's edges (an infinite m_spec,
    a dot far above 2, a NaN light colour behind an occluder) with every term
    on the exact path."""
    monkeypatch.setenv("RT_QUEUE_EXACT_ALL", "1")
    _queue_vs_oracle(rt, case)


# ---------------------------------------------------------------- async entry points
def _device_prims(P, n):
    import torch
    return torch.frombuffer(bytearray(bytes(P)[:96 * n]), dtype=torch.uint8).cuda()


def test_whitted_async_row_window_on_stream(rt):
    """rtw_render_async: a fuzzed scene in device memory, a row window, a
    non-default stream; rows outside the window untouched."""
    import torch
    P, n, w, h, _, _ = D.whitted_case("fuzz-%d" % D.WHITTED_FUZZ_DEEP[0])
    r0, r1 = 33, h - 41
    assert 20 <= r0 < r1 <= h
    ref, rc = O.whitted_render(w, h, row_begin=r0, row_end=r1, nthreads=L.NT, prims=P, n=n)
    d_prims = _device_prims(P, n)
    frame = torch.full((h, w), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rt.check(rt.lib().rtw_render_async(d_prims.data_ptr(), n, frame.data_ptr(), w, h, r0, r1, cnt.data_ptr(),
                                           C.c_void_p(s.cuda_stream)))
    s.synchronize()
    got = frame.cpu().numpy().view(np.uint32)
    _equal(ref[r0:r1], got[r0:r1], "rows [%d, %d)" % (r0, r1))
    assert (got[:r0] == 0x7f7f7f7f).all() and (got[r1:] == 0x7f7f7f7f).all()
    assert cnt.cpu().tolist() == rc


def test_queue_async_row_window_on_stream(rt):
    import torch
    P, n, w, h, _, _ = D.queue_case("fuzz-%d" % D.QUEUE_FUZZ_DEEP[0])
    r0, r1 = 13, h - 22
    ref, rc = O.queue_render(w, h, P, n, row_begin=r0, row_end=r1, nthreads=L.NT)
    d_prims = _device_prims(P, n)
    frame = torch.full((h, w), 0x7f7f7f7f, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        rt.check(rt.lib().rtq_render_async(d_prims.data_ptr(), n, frame.data_ptr(), w, h, r0, r1, cnt.data_ptr(),
                                           C.c_void_p(s.cuda_stream)))
    s.synchronize()
    got = frame.cpu().numpy().view(np.uint8).reshape(h, w, 4)
    _equal(ref[r0:r1], got[r0:r1], "rows [%d, %d)" % (r0, r1))
    assert (got[:r0] == 0x7f).all() and (got[r1:] == 0x7f).all()
    assert cnt.cpu().tolist() == rc
