"""CPU pins of what tests/test_gpu_queue_trace.py compares rtq_trace with: the
chain reference (tests/native/queue_trace_ref.c), fed
rtamd.scenes.queue_camera_rays at group 9 and packed by
rtamd.scenes.queue_pack, reproduces the oracle's frames (orq_render) and all
four counters -- so the chain contract (a pixel's push and drain loop along
the rays as given) is the frame's, and the two numpy helpers restate the
camera and the pack exactly."""
import numpy as np
import pytest

import degenerate_prims as D
import lit_scenes
import oracle_lib as O
import prims_query_ref as Q
import queue_trace_ref as R
import rtamd
from rtamd import scenes

F = np.float32


def _frame_from_rays(P, n, w, h):
    rays = scenes.queue_camera_rays(w, h)
    assert rays.shape == (h, w, 9, 6) and rays.dtype == np.float32
    col, t, ids, cnt = R.trace(P, n, rays, 9)
    px = scenes.queue_pack(col.reshape(h, w, 3))
    assert px.dtype == np.uint32 and px.shape == (h, w)
    return px, cnt


def test_reference_scene_frame_and_counters():
    P, n = O.queue_scene()
    ref, rcnt = O.queue_render(120, 90, nthreads=R.NT)
    px, cnt = _frame_from_rays(P, n, 120, 90)
    assert (px == R.frame_words(ref)).all(), "%d pixels differ" % (px != R.frame_words(ref)).sum()
    assert cnt == rcnt
    assert len(np.unique(px)) > 50                          # (not an empty frame)


@pytest.mark.parametrize("seed", [0, lit_scenes.QUEUE_EXACT_SEED, 7])
def test_lit_scenes_frames_and_counters(seed):
    P, n, ref, rcnt = lit_scenes.queue_lit(seed)
    px, cnt = _frame_from_rays(P, n, lit_scenes.QUEUE_W, lit_scenes.QUEUE_H)
    assert (px == R.frame_words(ref)).all(), "%d pixels differ" % (px != R.frame_words(ref)).sum()
    assert cnt == rcnt


CASES = ["ref-centre_nan", "ref-colour_inf", "ref-refr_inf", "lit-rindex_zero", "lit-spec_inf", "lit-type_minus7",
         "fuzz-0", "fuzz-5", "fuzz-14"]


@pytest.mark.parametrize("case", CASES)
def test_degenerate_primitives_frames_and_counters(case):
    assert case in D.QUEUE_CATALOGUE or case in D.QUEUE_FUZZ
    P, n, w, h, rays, out, frame, fcnt = R.case_set(case)
    px = scenes.queue_pack(out[0].reshape(h, w, 3))
    assert (px == R.frame_words(frame)).all(), "%d pixels differ" % (px != R.frame_words(frame)).sum()
    assert out[3] == fcnt


def test_camera_rays_row_window():
    full = scenes.queue_camera_rays(40, 30)
    part = scenes.queue_camera_rays(40, 30, 7, 19)
    assert part.shape == (12, 40, 9, 6) and (R.bits(part) == R.bits(full[7:19])).all()
    with pytest.raises(ValueError):
        scenes.queue_camera_rays(40, 30, 5, 31)
    with pytest.raises(ValueError):
        scenes.queue_camera_rays(40, 30, 5, 5)


def test_chain_rule():
    """acc is carried along the chain, so a chain whose first k - 1 rays add
    nothing has the colour of its last ray alone; a chain is not the float sum
    of its rays' own colours in general; t and id do not depend on group."""
    P, n, w, h, rays, single = R.camera_set("ref", 1)
    flat = rays.reshape(-1, 6)
    sel = flat[np.arange(512) * 53 % len(flat)]
    alone = R.trace(P, n, sel, 1)
    miss = R.trace(P, n, np.array([R.MISS], F), 1)
    assert miss[2][0] == -1 and miss[1][0] == R.FAR and (R.bits(miss[0]) == 0).all() and miss[3][3] == 1
    for k in (2, 5):
        chains = np.concatenate([np.tile(np.array(R.MISS, F), (len(sel), k - 1, 1)), sel[:, None, :]], axis=1)
        col, t, ids, cnt = R.trace(P, n, chains, k)
        assert (R.bits(col) == R.bits(alone[0])).all()
        assert (ids.reshape(-1, k)[:, :k - 1] == -1).all() and (R.bits(t.reshape(-1, k)[:, k - 1]) == R.bits(alone[1])).all()
        assert cnt[0] == alone[3][0] + (k - 1) * len(sel) and cnt[3] == alone[3][3] + (k - 1) * len(sel)
    nine = R.camera_set("ref", 9)[5]
    assert (R.bits(nine[1]) == R.bits(single[1])).all() and (nine[2] == single[2]).all()
    assert nine[3] == single[3]
    summed = np.zeros((h * w, 3), F)
    for k in range(9):
        summed = summed + single[0].reshape(-1, 9, 3)[:, k]
    assert (R.bits(summed) != R.bits(nine[0])).any()       # node order, not ray order: one float chain


def test_t_and_id_are_the_nearest_hit_querys():
    """d_t / d_id of arbitrary rays equal prims_query_ref's NEAREST answer for
    the queue tracer; a miss gives 1e7 and -1."""
    P, n = O.queue_scene()
    rays = np.concatenate([R.arbitrary_rays(1024), R.explicit_rows(P, n), Q.escapes()])
    col, t, ids, cnt = R.trace(P, n, rays, 1)
    qt, qid, _ = Q.query(Q.scene_of(P, n, "queue"), rays, "queue", "nearest")
    assert R.same_floats(qt, t) and (qid == ids).all()
    assert (ids == -1).sum() >= 12 and (t[ids == -1] == R.FAR).all() and (t[ids != -1] < R.FAR).all()
    assert cnt[0] > len(rays) and cnt[3] >= (ids == -1).sum()


def test_arbitrary_rays_recipe():
    """The fixed recipe of the GPU test walks more than the roots: trees with
    children, root hits on lights, undefined-behaviour events."""
    P, n = O.queue_scene()
    rays = R.arbitrary_rays()
    assert rays.shape == (4096, 6)
    col, t, ids, cnt = R.trace(P, n, rays, 1)
    lights = [i for i in range(n) if P[i].is_light]
    assert cnt[0] > 2 * len(rays) and np.isin(ids, lights).sum() > 100 and cnt[3] > 0
    length = np.linalg.norm(rays[:, 3:], axis=1)
    assert length.min() < 0.2 and length.max() > 3.9


def test_pack_conversion_edges():
    """x28, (int) as x86 converts (INT_MIN for NaN and out of range), the
    clamp from above only, each channel's low byte."""
    c = np.array([[1.0, 0.5, 0.25],                  # 28 14 7
                  [100.0, np.nan, 0.0],              # 255, INT_MIN & 0xff = 0, 0
                  [-1.0, 255.99 / 28.0, 0.0],        # -28 & 0xff = 228, 255, 0
                  [np.inf, -np.inf, 1e30],           # INT_MIN x 3 -> 0
                  [2.0 ** 31 / 28.0, -0.26, 9.2],    # 2^31: INT_MIN -> 0; -7 & 0xff = 249; 257 -> 255
                  [-(2.0 ** 31) / 28.0, 255.0 / 28.0, 256.0 / 28.0]], F)
    lo = -(1 << 31)

    def cvt(x):                                      # cvt_i32_x86 on the float32 product
        v = F(x) * F(28.0)
        return int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else lo

    want = []
    for row in c:
        r, g, b = (min(cvt(x), 255) & 0xff for x in row)
        want.append(r | g << 8 | b << 16)
    got = [int(v) for v in scenes.queue_pack(c)]
    assert got == want
    assert got[0] == 28 | 14 << 8 | 7 << 16 and got[1] == 255 and got[3] == 0
    assert got[2] == 228 | 255 << 8 and got[4] == 249 << 8 | 255 << 16
    assert scenes.queue_pack(np.zeros((4, 5, 3), F)).shape == (4, 5)


def test_python_surface():
    assert callable(rtamd.queue_trace) and callable(rtamd.queue_trace_async)
    assert "queue_trace" in rtamd.__all__ and "queue_trace_async" in rtamd.__all__
