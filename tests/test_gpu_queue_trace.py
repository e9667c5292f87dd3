"""GPU parity of rtq_trace / rtq_trace_async (csrc/queue.hip): the colour the
queue tracer computes along the caller's chains of rays, bit for bit -- chain
colours, root distance, root primitive and the four work counters -- against
tests/queue_trace_ref.py (the oracle's q_raytrace under q_pixel's push and
drain loop; tests/test_queue_trace_ref.py pins that to the oracle's frames).
Where the reference's float is a NaN, any NaN is accepted."""
import contextlib
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import lit_scenes
import oracle_lib as O
import prims_query_ref as Q
import queue_trace_ref as R
from rtamd import scenes

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 8                         # elements past the end of every output
FILL_F, FILL_I = -777.25, -777


@contextlib.contextmanager
def env(**kv):
    """RT_QUEUE_TRACE_SLAB / RT_QUEUE_POOL_CAP / RT_QUEUE_EXACT_ALL / RT_POOL_FRAC, all read at the call."""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()       # (a copy: the shared references are read-only)


def prim_bytes(P, n):
    return dev(np.frombuffer(P, dtype=np.uint8, count=C.sizeof(P._type_) * n).copy())


class Call:
    """One rtq_trace_async through the C entry point: sentinel-filled outputs
    with guard elements, issue(stream), then fetch() after a synchronise."""

    def __init__(self, rt, P, n, rays, group, want_t=True, want_id=True, counters=True):
        import torch
        self.rt, self.n, self.group = rt, n, group
        rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
        self.nr = nr = len(rays)
        assert nr % group == 0
        self.nc = nc = nr // group
        self.d_prims, self.d_rays = prim_bytes(P, n), dev(rays if nr else np.zeros((1, 6), F))
        self.col = torch.full((3 * (nc + GUARD),), FILL_F, dtype=torch.float32, device="cuda")
        self.t = torch.full((nr + GUARD,), FILL_F, dtype=torch.float32, device="cuda")
        self.ids = torch.full((nr + GUARD,), FILL_I, dtype=torch.int32, device="cuda")
        self.cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.want_t, self.want_id, self.counters = want_t, want_id, counters

    def issue(self, stream=None):
        import torch
        s = (stream or torch.cuda.current_stream()).cuda_stream
        return self.rt.entry("rtq_trace_async")(self.d_prims.data_ptr(), self.n, self.d_rays.data_ptr(), self.nr,
                                                self.group, self.col.data_ptr(),
                                                self.t.data_ptr() if self.want_t else None,
                                                self.ids.data_ptr() if self.want_id else None,
                                                self.cnt.data_ptr() if self.counters else None, s)

    def fetch(self):
        nr, nc = self.nr, self.nc
        col, t, ids = self.col.cpu().numpy(), self.t.cpu().numpy(), self.ids.cpu().numpy()
        assert (col[3 * nc:] == F(FILL_F)).all() and (t[nr:] == F(FILL_F)).all() and (ids[nr:] == FILL_I).all(), \
            "written past the end"
        assert self.want_t or (t == F(FILL_F)).all(), "d_t was not asked for but written"
        assert self.want_id or (ids == FILL_I).all(), "d_id was not asked for but written"
        cnt = [int(v) for v in self.cnt.cpu().numpy()]
        assert self.counters or cnt == [0, 0, 0, 0]
        return col[:3 * nc].reshape(nc, 3), t[:nr], ids[:nr], cnt


def gpu_trace(rt, P, n, rays, group, **kw):
    import torch
    call = Call(rt, P, n, rays, group, **kw)
    rt.check(call.issue())
    torch.cuda.synchronize()
    return call.fetch()


def agree(what, got, ref, want_t=True, want_id=True, counters=True):
    """got = (colour, t, id, counters) of the GPU, ref = R.trace()'s tuple."""
    col, t, ids, cnt = got
    assert col.shape == ref[0].shape
    bad = np.flatnonzero(~((R.bits(col) == R.bits(ref[0])) | (np.isnan(col) & np.isnan(ref[0]))).all(axis=1))
    assert bad.size == 0, "%s: %d of %d colours differ, first chain %d: got %r, reference %r" % (
        what, bad.size, len(col), bad[0], col[bad[0]], ref[0][bad[0]])
    if want_t:
        assert R.same_floats(ref[1], t), "%s: t differs on %d rays" % (what, (R.bits(ref[1]) != R.bits(t)).sum())
    if want_id:
        assert (ids == ref[2]).all(), "%s: id differs on %d rays" % (what, (ids != ref[2]).sum())
    if counters:
        assert cnt == ref[3], "%s: counters %r, reference %r" % (what, cnt, ref[3])


def deep_condition(rays, ref):
    """The deep set walks the level pass and the fold: at least 8 traced rays
    per caller ray in the reference."""
    assert ref[3][0] >= 8 * rays.reshape(-1, 6).shape[0], ref[3]


# ---------------------------------------------------------------- 1. camera-ray sets
@pytest.mark.parametrize("name", ["ref", "deep"])
@pytest.mark.parametrize("group", [9, 1])
def test_camera_ray_sets(rt, name, group):
    P, n, w, h, rays, ref = R.camera_set(name, group)
    if name == "deep":
        deep_condition(rays, ref)
    got = gpu_trace(rt, P, n, rays, group)
    agree("%s set, group %d" % (name, group), got, ref)
    if group == 9:
        frame, fcnt = O.queue_render(w, h, P, n, nthreads=R.NT)
        assert (scenes.queue_pack(got[0].reshape(h, w, 3)) == R.frame_words(frame)).all() and got[3] == fcnt


# ---------------------------------------------------------------- 2. group sizes
@pytest.mark.parametrize("group", [1, 2, 3, 9, 10, 64])
def test_group_sizes(rt, group):
    P, n, w, h, rays, _ = R.camera_set("deep", 9)
    flat = rays.reshape(-1, 6)[20000:25760]
    sel = flat[:len(flat) // group * group]
    assert len(sel) >= 5000
    want = R.trace(P, n, sel, group)
    assert want[3][0] > 4 * len(sel)
    agree("group %d" % group, gpu_trace(rt, P, n, sel, group), want)


# ---------------------------------------------------------------- 3. batch edges
@pytest.mark.parametrize("nchains", [1, 63, 64, 65, 255, 256, 257, 4113])
@pytest.mark.parametrize("group", [1, 9])
def test_batch_edges(rt, nchains, group):
    """Around the wave and the block; the guard elements past the end stay."""
    P, n, w, h, rays, _ = R.camera_set("ref", 9)
    flat = rays.reshape(-1, 6)
    sel = flat[(np.arange(nchains * group) * 3 + 14030) % len(flat)]    # from the rows through the spheres
    want = R.trace(P, n, sel, group)
    assert want[3][0] > nchains * group                                  # (some trees have children)
    agree("%d chains of %d" % (nchains, group), gpu_trace(rt, P, n, sel, group), want)


def test_zero_rays(rt):
    import torch
    P, n = O.queue_scene()
    call = Call(rt, P, n, np.zeros((0, 6), F), 9)
    assert call.issue() == 0
    torch.cuda.synchronize()
    assert call.fetch()[3] == [0, 0, 0, 0]


# ---------------------------------------------------------------- 4. arbitrary rays
@pytest.mark.parametrize("group", [1, 4])
def test_arbitrary_rays(rt, group):
    """The fixed 4,096-ray recipe plus explicit rows: misses, origins inside
    glass spheres, root hits on lights, zero-length directions, NaN and +-inf
    in every component."""
    P, n = O.queue_scene()
    rays = np.concatenate([R.arbitrary_rays(), R.explicit_rows(P, n), Q.escapes()])
    rays = rays[:len(rays) // group * group]
    assert len(rays) > 4096 + 30
    ref = R.trace(P, n, rays, group)
    lights = [i for i in range(n) if P[i].is_light]
    assert ref[3][0] > 2 * len(rays) and np.isin(ref[2], lights).sum() > 100 and ref[3][3] > 0
    assert (ref[2] == -1).sum() >= 12 and not np.isfinite(rays).all()
    agree("arbitrary, group %d" % group, gpu_trace(rt, P, n, rays, group), ref)


# ---------------------------------------------------------------- 5. degenerate primitives
@pytest.mark.parametrize("case", ["ref-colour_inf", "lit-rindex_zero", "lit-spec_inf", "lit-type_minus7",
                                  "fuzz-5", "fuzz-14"])
def test_degenerate_primitives(rt, case):
    P, n, w, h, rays, ref, frame, fcnt = R.case_set(case)
    got = gpu_trace(rt, P, n, rays, 9)
    agree(case, got, ref)
    assert (scenes.queue_pack(got[0].reshape(h, w, 3)) == R.frame_words(frame)).all() and got[3] == fcnt


# ---------------------------------------------------------------- 6. the frames' environment hooks
@pytest.mark.parametrize("cap", [1, 1000])
@pytest.mark.parametrize("group", [9, 1])
def test_pool_overflow_finishes_in_fix_kernel(rt, cap, group):
    """Far more nodes than the pool holds: the chains left over are finished
    exactly from the caller's rays."""
    P, n, w, h, rays, ref = R.camera_set("deep", group)
    deep_condition(rays, ref)
    with env(RT_QUEUE_POOL_CAP=cap):
        got = gpu_trace(rt, P, n, rays, group)
    agree("cap %d, group %d" % (cap, group), got, ref)


@pytest.mark.parametrize("name,group", [("deep", 9), ("ref", 1), ("ref", 9)])
def test_exact_all(rt, name, group):
    """Every specular term uncertified: every chain with one goes through the
    view-parameterised exact path."""
    P, n, w, h, rays, ref = R.camera_set(name, group)
    with env(RT_QUEUE_EXACT_ALL=1):
        got = gpu_trace(rt, P, n, rays, group)
    agree("exact all, %s, group %d" % (name, group), got, ref)


# ---------------------------------------------------------------- 7. slabs
@pytest.mark.parametrize("name,group,slab", [("deep", 9, 20000), ("deep", 1, 9000), ("ref", 9, 1000)])
def test_slabs(rt, name, group, slab):
    """deep, group 9: 20,000 rays (not a multiple of 9) -> 2,223 chains ->
    2,240: slabs of 2,240, 2,240, 2,240 and 192 chains.  deep, group 1: 9,024
    rays: seven slabs.  ref, group 9: 128 chains: 24 slabs."""
    P, n, w, h, rays, ref = R.camera_set(name, group)
    nchains = rays.reshape(-1, 6).shape[0] // group
    assert nchains > 2 * ((-(-slab // group) + 63) // 64 * 64)            # three or more slabs
    with env(RT_QUEUE_TRACE_SLAB=slab):
        got = gpu_trace(rt, P, n, rays, group)
    agree("slabs", got, ref)


# ---------------------------------------------------------------- 8. nullable outputs
@pytest.mark.parametrize("want_t,want_id,counters", list(itertools.product([False, True], repeat=3)))
def test_nullable_outputs(rt, want_t, want_id, counters):
    P, n, w, h, rays, ref = R.camera_set("ref", 9)
    got = gpu_trace(rt, P, n, rays, 9, want_t=want_t, want_id=want_id, counters=counters)
    agree("nullable", got, ref, want_t, want_id, counters)


# ---------------------------------------------------------------- 9. the ray query's answer
def test_t_and_id_are_rtp_querys_nearest(rt):
    import torch
    P, n = O.queue_scene()
    rays = np.concatenate([R.arbitrary_rays(), R.explicit_rows(P, n), Q.escapes()])
    got = gpu_trace(rt, P, n, rays, 1)
    ps = rt.PrimScene(P, n, tracer="queue")
    t, ids, _ = ps.query(dev(rays))
    torch.cuda.synchronize()
    t, ids = t.cpu().numpy(), ids.cpu().numpy()
    assert (R.bits(t) == R.bits(got[1])).all() and (ids == got[2]).all()
    assert (ids == -1).sum() >= 12 and (t[ids == -1] == R.FAR).all()
    ps.close()


# ---------------------------------------------------------------- 10. stream ordering
def test_trace_frame_trace_on_three_streams(rt):
    """A trace, a frame and a trace issued back to back on three streams share
    the level pass's arena: serialised on the device, all exact."""
    import torch
    P, n, w, h, rays, ref = R.camera_set("deep", 9)
    P2, n2, w2, h2, rays2, ref2 = R.camera_set("ref", 1)
    _, _, frame, fcnt = lit_scenes.queue_lit(lit_scenes.QUEUE_EXACT_SEED)
    a, b = Call(rt, P, n, rays, 9), Call(rt, P2, n2, rays2, 1)
    d_prims = prim_bytes(P, n)
    d_frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = [torch.cuda.Stream() for _ in range(3)]
    rt.check(a.issue(s[0]))
    rt.check(rt.lib().rtq_render_async(d_prims.data_ptr(), n, d_frame.data_ptr(), w, h, 0, h, d_cnt.data_ptr(),
                                       s[1].cuda_stream))
    rt.check(b.issue(s[2]))
    torch.cuda.synchronize()
    agree("first trace", a.fetch(), ref)
    agree("second trace", b.fetch(), ref2)
    assert (d_frame.cpu().numpy().view(np.uint32) == R.frame_words(frame)).all() and d_cnt.cpu().tolist() == fcnt


# ---------------------------------------------------------------- 11. memory
@pytest.mark.parametrize("group", [9, 1, 64])
def test_a_trace_caches_no_more_than_a_frame_of_as_many_trees(rt, group):
    import torch
    w, h = 64, 32                                                     # x 9 = 18,432 trees
    P, n, _, _, rays, _ = R.camera_set("ref", 9)
    many = rays.reshape(-1, 6)[:w * h * 9]
    assert len(many) == 18432 and len(many) % group == 0
    sizes = {}
    rt.lib().rt_release()
    call = Call(rt, P, n, many, group)
    rt.check(call.issue())
    torch.cuda.synchronize()
    sizes["trace"] = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    rt.queue_trace(many, P, n, group=group)
    sizes["blocking trace"] = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    d_frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    rt.check(rt.lib().rtq_render_async(call.d_prims.data_ptr(), n, d_frame.data_ptr(), w, h, 0, h, None,
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    sizes["frame"] = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    assert 0 < sizes["trace"] <= sizes["frame"] and sizes["blocking trace"] == sizes["trace"], sizes


# ---------------------------------------------------------------- 12. arguments
def test_argument_errors_come_before_any_device_work(rt):
    """Every refusal returns RT_ERR_INVALID and writes nothing: real rays and
    primitives, sentinel-filled outputs (device buffers for rtq_trace_async,
    host arrays for rtq_trace) that are untouched after a synchronise, counters
    included.  So are they after nrays == 0, which is RT_OK."""
    import torch
    P, n, _, _, rays, _ = R.camera_set("ref", 9)
    flat = np.ascontiguousarray(rays.reshape(-1, 6)[:64])
    call = Call(rt, P, n, flat, 1)
    call.cnt.fill_(FILL_I)
    h_prims = np.frombuffer(P, dtype=np.uint8, count=96 * n).copy()
    h_col, h_t = np.full(3 * 64, FILL_F, F), np.full(64, FILL_F, F)
    h_id, h_cnt = np.full(64, FILL_I, np.int32), np.full(4, 12345, np.uint64)
    fn, blocking = rt.entry("rtq_trace_async"), rt.entry("rtq_trace")
    dev_args = dict(prims=call.d_prims.data_ptr(), nprims=n, rays=call.d_rays.data_ptr(), nrays=64, group=1,
                    color=call.col.data_ptr())
    host_args = dict(prims=h_prims.ctypes.data, nprims=n, rays=flat.ctypes.data, nrays=64, group=1,
                     color=h_col.ctypes.data)
    dev_tail = (call.t.data_ptr(), call.ids.data_ptr(), call.cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    host_tail = (h_t.ctypes.data, h_id.ctypes.data, h_cnt.ctypes.data)

    def untouched():
        torch.cuda.synchronize()
        assert (call.col.cpu().numpy() == F(FILL_F)).all() and (call.t.cpu().numpy() == F(FILL_F)).all()
        assert (call.ids.cpu().numpy() == FILL_I).all() and (call.cnt.cpu().numpy() == FILL_I).all()
        assert (h_col == F(FILL_F)).all() and (h_t == F(FILL_F)).all() and (h_id == FILL_I).all()

    bad = [dict(prims=None), dict(rays=None), dict(color=None), dict(nprims=0), dict(nprims=65), dict(nprims=-1),
           dict(group=0), dict(group=65), dict(group=-1), dict(group=9), dict(nrays=63, group=2),
           dict(nrays=2 ** 31), dict(nrays=2 ** 31 + 1, group=1)]
    for kw in bad:
        for f, base, tail in ((fn, dev_args, dev_tail), (blocking, host_args, host_tail)):
            a = dict(base)
            a.update(kw)
            rc = f(a["prims"], a["nprims"], a["rays"], a["nrays"], a["group"], a["color"], *tail)
            assert rc == -1, (kw, rc)
            assert b"rtq_trace" in rt.lib().rt_last_error()
        untouched()
        assert (h_cnt == 12345).all()                     # (a refused blocking call leaves the host counters too)
    # nrays == 0: RT_OK, nothing launched, nothing written but the blocking form's counters (this call's: 0)
    for f, base, tail in ((fn, dev_args, dev_tail), (blocking, host_args, host_tail)):
        a = dict(base, nrays=0, group=9)
        assert f(a["prims"], a["nprims"], a["rays"], 0, a["group"], a["color"], *tail) == 0
    untouched()
    assert (h_cnt == 0).all()


# ---------------------------------------------------------------- 13. Python surfaces
def test_blocking_numpy_surface(rt):
    P, n, w, h, rays, ref = R.camera_set("ref", 9)
    col, t, ids, cnt = rt.queue_trace(rays, P, n, group=9, counters=True)
    agree("queue_trace", (col, t, ids, cnt), ref)
    col, t, ids = rt.queue_trace(rays.reshape(-1, 6)[:5])             # the default scene, group 1
    agree("queue_trace default", (col, t, ids, None), R.trace(*O.queue_scene(), rays.reshape(-1, 6)[:5]),
          counters=False)


def test_torch_surface(rt):
    import torch
    P, n, w, h, rays, ref = R.camera_set("deep", 9)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    col, t, ids = rt.queue_trace_async(dev(rays.reshape(-1, 6)), prim_bytes(P, n), n, group=9, counters=cnt)
    torch.cuda.synchronize()
    agree("queue_trace_async", (col.cpu().numpy(), t.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().tolist()), ref)
    out = (torch.full((len(ref[0]), 3), FILL_F, dtype=torch.float32, device="cuda"), None, None)
    got = rt.queue_trace_async(dev(rays.reshape(-1, 6)), prim_bytes(P, n), n, group=9, out=out)
    torch.cuda.synchronize()
    assert got[0] is out[0] and got[1] is None and got[2] is None and R.same_floats(ref[0], out[0].cpu().numpy())
    with pytest.raises(ValueError):
        rt.queue_trace_async(dev(rays.reshape(-1, 6)[:10]), prim_bytes(P, n), n, group=9)


def test_the_frame_is_the_pack_of_the_trace_of_its_camera_rays(rt):
    w, h = 64, 48
    col, _, _ = rt.queue_trace(scenes.queue_camera_rays(w, h), group=9)
    frame = rt.queue_render(w, h)
    assert (scenes.queue_pack(col.reshape(h, w, 3)) == R.frame_words(frame)).all()


# ---------------------------------------------------------------- 14. the pool fractions
def diffuse_scene():
    """The reference scene without mirrors or glass: no tree has children, so a
    record pool of any size holds every frame."""
    P, n = O.queue_scene()
    for p in P[:n]:
        p.m_refl = p.m_refr = 0.0
    return P, n


def test_traces_of_many_sizes_leave_a_frame_sizes_fraction_alone(rt):
    """A frame size's learnt pool fraction survives more than 16 traces of
    different sizes (the frames' table has 16 entries).  The frame learns a
    small fraction (RT_POOL_FRAC at its entry's creation: 0.05 of its trees,
    enough for a scene without children); were its entry evicted, the next
    frame of that size would start from the default 0.8 again and the arena,
    which only grows, would come out larger."""
    import torch
    w, h = 64, 32
    P, n = diffuse_scene()
    ref, rcnt = O.queue_render(w, h, P, n, nthreads=R.NT)
    d_prims = prim_bytes(P, n)
    d_frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def frame():
        d_frame.zero_()
        rt.check(rt.lib().rtq_render_async(d_prims.data_ptr(), n, d_frame.data_ptr(), w, h, 0, h, None, s))
        torch.cuda.synchronize()
        assert (d_frame.cpu().numpy().view(np.uint32) == R.frame_words(ref)).all()
        return rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    with env(RT_POOL_FRAC=0.05):
        before = frame()
    Pt, nt, _, _, rays, _ = R.camera_set("ref", 9)
    flat = rays.reshape(-1, 6)
    sizes = [37 * k + 1 for k in range(1, 21)]                       # 20 sizes, up to 741 rays
    for k in sizes:
        sel = flat[14030:14030 + k]
        agree("%d rays" % k, gpu_trace(rt, Pt, nt, sel, 1), R.trace(Pt, nt, sel, 1))
    assert rt.lib().rt_cached_bytes() == before                      # (their arenas fit into the frame's)
    after = frame()
    rt.lib().rt_release()
    assert after == before, (before, after)


def test_a_trace_learns_its_fraction_per_size_bucket(rt):
    """A trace whose pool overflowed enlarges the pool of the next trace in
    its power-of-two size bucket, whatever that one's exact ray count: after
    62,208 rays at a pool of 0.25 (15,552 records -> four 4,096-record page
    rows, for more than 400,000 child nodes), 62,000 rays get 0.3125 (19,375:
    five page rows) -- a larger arena, though of fewer rays."""
    P, n, w, h, rays, ref = R.camera_set("deep", 1)
    flat = rays.reshape(-1, 6)
    assert len(flat) == 62208 and ref[3][0] - len(flat) > 400000
    rt.lib().rt_release()
    with env(RT_POOL_FRAC=0.25):
        agree("first", gpu_trace(rt, P, n, flat, 1), ref)
        first = rt.lib().rt_cached_bytes()
        agree("second", gpu_trace(rt, P, n, flat[:62000], 1), R.trace(P, n, flat[:62000], 1))
        second = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    assert second > first, (first, second)
