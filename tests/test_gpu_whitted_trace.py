"""GPU parity of rtw_trace / rtw_trace_async (csrc/whitted.hip): the colour the
Whitted tracer computes along the caller's rays, bit for bit -- colours, root
distance, root primitive and the four work counters -- against
tests/whitted_trace_ref.py (the oracle's engine_raytrace under the reference's
tree loop; tests/test_whitted_trace_ref.py pins that to the oracle's frames).
Where the reference's float is a NaN, any NaN is accepted."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import degenerate_prims as D
import lit_scenes
import oracle_lib as O
import whitted_trace_ref as R
from rtamd import scenes

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 8                         # elements past the end of every output
FILL_F, FILL_I = -777.25, -777


@contextlib.contextmanager
def env(**kv):
    """RT_WHITTED_TRACE_SLAB / RT_WHITTED_QUEUE_CAP, both read at the call."""
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
    """One rtw_trace_async through the C entry point: sentinel-filled outputs
    with guard elements, issue(stream), then fetch() after a synchronise."""

    def __init__(self, rt, P, n, rays, ocl, want_t=True, want_id=True, counters=True):
        import torch
        self.rt, self.n, self.ocl = rt, n, ocl
        rays = np.ascontiguousarray(rays, F).reshape(-1, 6)
        self.nr = nr = len(rays)
        self.d_prims, self.d_rays = prim_bytes(P, n), dev(rays if nr else np.zeros((1, 6), F))
        self.col = torch.full((3 * (nr + GUARD),), FILL_F, dtype=torch.float32, device="cuda")
        self.t = torch.full((nr + GUARD,), FILL_F, dtype=torch.float32, device="cuda")
        self.ids = torch.full((nr + GUARD,), FILL_I, dtype=torch.int32, device="cuda")
        self.cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.want_t, self.want_id, self.counters = want_t, want_id, counters

    def issue(self, stream=None):
        import torch
        s = (stream or torch.cuda.current_stream()).cuda_stream
        rt = self.rt
        return rt.entry("rtw_trace_async")(self.d_prims.data_ptr(), self.n, self.d_rays.data_ptr(), self.nr,
                                           rt.RTW_TRACE_OCL if self.ocl else 0, self.col.data_ptr(),
                                           self.t.data_ptr() if self.want_t else None,
                                           self.ids.data_ptr() if self.want_id else None,
                                           self.cnt.data_ptr() if self.counters else None, s)

    def fetch(self):
        nr = self.nr
        col, t, ids = self.col.cpu().numpy(), self.t.cpu().numpy(), self.ids.cpu().numpy()
        assert (col[3 * nr:] == F(FILL_F)).all() and (t[nr:] == F(FILL_F)).all() and (ids[nr:] == FILL_I).all(), \
            "written past nrays"
        assert self.want_t or (t == F(FILL_F)).all(), "d_t was not asked for but written"
        assert self.want_id or (ids == FILL_I).all(), "d_id was not asked for but written"
        cnt = [int(v) for v in self.cnt.cpu().numpy()]
        assert self.counters or cnt == [0, 0, 0, 0]
        return col[:3 * nr].reshape(nr, 3), t[:nr], ids[:nr], cnt


def gpu_trace(rt, P, n, rays, ocl, **kw):
    import torch
    call = Call(rt, P, n, rays, ocl, **kw)
    rt.check(call.issue())
    torch.cuda.synchronize()
    return call.fetch()


def agree(what, got, ref, want_t=True, want_id=True, counters=True):
    """got = (colour, t, id, counters) of the GPU, ref = R.trace()'s tuple."""
    col, t, ids, cnt = got
    bad = np.flatnonzero(~((R.bits(col) == R.bits(ref[0])) | (np.isnan(col) & np.isnan(ref[0]))).all(axis=1))
    assert bad.size == 0, "%s: %d of %d colours differ, first ray %d: got %r, reference %r" % (
        what, bad.size, len(col), bad[0], col[bad[0]], ref[0][bad[0]])
    if want_t:
        assert R.same_floats(ref[1], t), "%s: t differs on %d rays" % (what, (R.bits(ref[1]) != R.bits(t)).sum())
    if want_id:
        assert (ids == ref[2]).all(), "%s: id differs on %d rays" % (what, (ids != ref[2]).sum())
    if counters:
        assert cnt == ref[3], "%s: counters %r, reference %r" % (what, cnt, ref[3])


# ---------------------------------------------------------------- 1. camera-ray sets
@pytest.mark.parametrize("name", ["ref", "low"])
@pytest.mark.parametrize("ocl", [False, True], ids=["cpu", "ocl"])
def test_camera_ray_sets(rt, name, ocl):
    """The two 64 x 48 sets (stale ray = an earlier node's / the caller's own);
    whitted_pack of the result is the oracle's frame."""
    P, n, rays, ref = R.camera_set(name, ocl)
    if not ocl:
        assert ref[4] == ([9, 0] if name == "ref" else [0, 1323])
    got = gpu_trace(rt, P, n, rays, ocl)
    agree("%s set" % name, got, ref)
    oracle = (O.whitted_render_ocl(64, 48, nthreads=R.NT, prims=P, n=n) if ocl
              else O.whitted_render(64, 48, 20, 48, nthreads=R.NT, prims=P, n=n))
    px = scenes.whitted_pack(got[0].reshape(rays.shape[:3] + (3,)), ocl=ocl)
    assert (px == oracle[0][20:48]).all() and got[3] == oracle[1]


def test_blocking_numpy_surface(rt):
    P, n, rays, ref = R.camera_set("ref", False)
    col, t, ids, cnt = rt.whitted_trace(rays, P, n, counters=True)
    agree("whitted_trace", (col, t, ids, cnt), ref)
    col, t, ids = rt.whitted_trace(rays[:3], ocl=True)              # the default scene
    ref = R.trace(*O.whitted_scene(), rays[:3], True)
    agree("whitted_trace ocl", (col, t, ids, None), ref, counters=False)


def test_torch_surface(rt):
    import torch
    P, n, rays, ref = R.camera_set("low", False)
    cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    col, t, ids = rt.whitted_trace_async(dev(rays.reshape(-1, 6)), prim_bytes(P, n), n, counters=cnt)
    torch.cuda.synchronize()
    agree("whitted_trace_async", (col.cpu().numpy(), t.cpu().numpy(), ids.cpu().numpy(), cnt.cpu().tolist()), ref)


# ---------------------------------------------------------------- 2. walled scenes
@pytest.mark.parametrize("seed", [lit_scenes.WALLED_DEEP_SEED, lit_scenes.WALLED_SEEDS[0], lit_scenes.WALLED_SEEDS[4]])
@pytest.mark.parametrize("ocl", [False, True], ids=["cpu", "ocl"])
def test_walled_scenes(rt, seed, ocl):
    P, n, w, h, rays, ref, (frame, fcnt) = R.walled_set(seed, ocl)
    r0, r1 = R.window_rows(w, h, ocl)
    lit_scenes.check_lit(frame, (r0, r1))
    got = gpu_trace(rt, P, n, rays, ocl)
    agree("walled %d" % seed, got, ref)
    px = scenes.whitted_pack(got[0].reshape(rays.shape[:3] + (3,)), ocl=ocl)
    assert (px == frame[r0:r1]).all() and got[3] == fcnt


# ---------------------------------------------------------------- 3. batch edges
@pytest.mark.parametrize("nrays", [1, 63, 64, 65, 255, 256, 257, 4113])
def test_batch_edges(rt, nrays):
    """Around the wave and the block; the guard elements past nrays stay."""
    P, n, rays, ref = R.camera_set("ref", False)
    sel = rays.reshape(-1, 6)[(np.arange(nrays) * 3 + 5000) % 16128]     # from the rows through the spheres
    want = R.trace(P, n, sel)
    assert want[3][0] > nrays                                        # (some trees have children)
    agree("%d rays" % nrays, gpu_trace(rt, P, n, sel, False), want)


def test_zero_rays(rt):
    P, n = O.whitted_scene()
    call = Call(rt, P, n, np.zeros((0, 6), F), False)
    assert call.issue() == 0
    import torch
    torch.cuda.synchronize()
    assert call.fetch()[3] == [0, 0, 0, 0]


# ---------------------------------------------------------------- 4. arbitrary rays
def arbitrary_rays(P, n, count=4096, seed=7):
    """A quarter each, shuffled so that every wave mixes them: origins inside
    glass spheres; directions of length 1e-3 .. 1e3 from around the camera;
    ordinary unit rays with one component NaN / +inf / -inf; and ordinary unit
    rays among which every sixteenth has a zero direction."""
    rng = np.random.default_rng(seed)
    q = count // 4

    def unit(k):
        d = rng.standard_normal((k, 3))
        return d / np.linalg.norm(d, axis=1, keepdims=True)
    glass = [p for p in P[:n] if p.type == 1 and p.m_Refr > 0 and p.m_Light <= 0]
    assert glass
    g = [glass[i] for i in rng.integers(0, len(glass), q)]
    cen = np.array([[p.m_Centre.x, p.m_Centre.y, p.m_Centre.z] for p in g])
    rad = np.array([p.m_Radius for p in g])[:, None]
    inside = np.concatenate([cen + unit(q) * rad * rng.uniform(0, 0.95, (q, 1)), unit(q)], axis=1)
    eye = lit_scenes.CAMERA + rng.uniform(-2, 2, (q, 3))
    aim = np.array([0.0, 0.0, 20.0]) + rng.uniform(-8, 8, (q, 3)) - eye
    aim /= np.linalg.norm(aim, axis=1, keepdims=True)
    scaled = np.concatenate([eye, aim * 10.0 ** rng.uniform(-3, 3, (q, 1))], axis=1)
    odd = np.concatenate([lit_scenes.CAMERA + rng.uniform(-1, 1, (q, 3)), unit(q)], axis=1)
    odd[np.arange(q), rng.integers(0, 6, q)] = rng.choice([np.nan, np.inf, -np.inf], q)
    plain = np.concatenate([lit_scenes.CAMERA + rng.uniform(-1, 1, (q, 3)), unit(q)], axis=1)
    plain[:, 5] = np.abs(plain[:, 5])                                # into the scene
    plain[::16, 3:] = 0.0
    rays = np.concatenate([inside, scaled, odd, plain]).astype(F)
    return rays[rng.permutation(len(rays))]


ARBITRARY = ["lit", "lit-colour_nan", "lit-rindex_zero", "lit-refr_inf", "lit-light_flag_minus1", "lit-centre_inf"]


@pytest.mark.parametrize("case", ARBITRARY)
@pytest.mark.parametrize("ocl", [False, True], ids=["cpu", "ocl"])
def test_arbitrary_rays(rt, case, ocl):
    """4,096 rays that no camera makes, against the 64-primitive walled scene
    and five degenerate edits of it."""
    words, _ = D.whitted_words(case)
    P, n = D.prims_of(O.Primitive, words), len(words)
    assert n == 64
    base, _ = D.whitted_words("lit")
    rays = arbitrary_rays(D.prims_of(O.Primitive, base), n)
    assert len(rays) == 4096
    ref = R.trace(P, n, rays, ocl)
    assert ref[3][0] > 2 * len(rays) and (ref[2] == -1).any()         # trees with children, and misses
    assert np.isnan(ref[0]).any() == (case == "lit-colour_nan")
    if case == "lit-rindex_zero":
        assert min(ref[4]) > 100                                      # TIR nodes of both stale-ray kinds
    agree(case, gpu_trace(rt, P, n, rays, ocl), ref)


# ---------------------------------------------------------------- 5. overflow
@pytest.mark.parametrize("cap", [1, 1000])
@pytest.mark.parametrize("ocl", [False, True], ids=["cpu", "ocl"])
def test_pool_overflow_finishes_in_fixup(rt, cap, ocl):
    P, n, w, h, rays, ref, _ = R.walled_set(lit_scenes.WALLED_DEEP_SEED, ocl)
    assert ref[3][0] > 3 * rays.reshape(-1, 6).shape[0]              # far more nodes than the pool holds
    with env(RT_WHITTED_QUEUE_CAP=cap):
        got = gpu_trace(rt, P, n, rays, ocl)
    agree("cap %d" % cap, got, ref)


def test_tir_with_a_small_pool(rt):
    """The caller's-own-ray set where the TIR lists and the pool overflow."""
    P, n, rays, ref = R.camera_set("low", False)
    with env(RT_WHITTED_QUEUE_CAP=3000):
        got = gpu_trace(rt, P, n, rays, False)
    agree("low, cap 3000", got, ref)


# ---------------------------------------------------------------- 6. slabs
@pytest.mark.parametrize("name", ["ref", "low"])
def test_slabs(rt, name):
    """16,128 rays in slabs of 4,096: four, the last one ragged (3,840)."""
    P, n, rays, ref = R.camera_set(name, False)
    with env(RT_WHITTED_TRACE_SLAB=4090):                            # (rounded up to 4,096)
        got = gpu_trace(rt, P, n, rays, False)
    agree("slabs", got, ref)


# ---------------------------------------------------------------- 7. nullable outputs
@pytest.mark.parametrize("want_t,want_id,counters", [(False, False, False), (True, False, True), (False, True, False)])
def test_nullable_outputs(rt, want_t, want_id, counters):
    P, n, rays, ref = R.camera_set("ref", True)
    got = gpu_trace(rt, P, n, rays, True, want_t=want_t, want_id=want_id, counters=counters)
    agree("nullable", got, ref, want_t, want_id, counters)


# ---------------------------------------------------------------- 8. negative zero and lights
def test_light_hit_at_the_root(rt):
    """A light whose colour has a -0.0 channel: openCLcode.h adds the colour
    to 0 (+0.0); the CPU path adds 1."""
    P, n = O.whitted_scene()
    lights = [i for i in range(n) if P[i].m_Light > 0 and P[i].type == 1]
    for i in lights:
        P[i].m_Color.y = -0.0
    aim = np.array([[P[i].m_Centre.x, P[i].m_Centre.y - 0.25, P[i].m_Centre.z + 7] for i in lights])
    rays = np.concatenate([np.tile([0, 0.25, -7], (len(lights), 1)), aim / np.linalg.norm(aim, axis=1, keepdims=True)],
                          axis=1).astype(F)
    for ocl in (True, False):
        ref = R.trace(P, n, rays, ocl)
        assert list(ref[2]) == lights
        want = [[P[i].m_Color.x, 0.0, P[i].m_Color.z] for i in lights] if ocl else [[1, 1, 1]] * len(lights)
        assert (R.bits(ref[0]) == R.bits(np.array(want, F))).all()   # (+0.0: bits 0)
        agree("light, ocl=%s" % ocl, gpu_trace(rt, P, n, rays, ocl), ref)


# ---------------------------------------------------------------- 9. stream ordering
def test_trace_frame_trace_on_three_streams(rt):
    """A trace, a frame and a trace issued back to back on three streams share
    the level pass's arena: serialised on the device, all exact."""
    import torch
    seed = lit_scenes.WALLED_DEEP_SEED
    P, n, w, h, rays, ref, (frame, fcnt) = R.walled_set(seed, False)
    P2, n2, rays2, ref2 = R.camera_set("low", False)
    a, b = Call(rt, P, n, rays, False), Call(rt, P2, n2, rays2, False)
    d_prims = prim_bytes(P, n)
    d_frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = [torch.cuda.Stream() for _ in range(3)]
    rt.check(a.issue(s[0]))
    rt.check(rt.lib().rtw_render_async(d_prims.data_ptr(), n, d_frame.data_ptr(), w, h, 20, h - 70, d_cnt.data_ptr(),
                                       s[1].cuda_stream))
    rt.check(b.issue(s[2]))
    torch.cuda.synchronize()
    agree("first trace", a.fetch(), ref)
    agree("second trace", b.fetch(), ref2)
    assert (d_frame.cpu().numpy().view(np.uint32) == frame).all() and d_cnt.cpu().tolist() == fcnt


# ---------------------------------------------------------------- 10. memory
def test_a_trace_caches_no_more_than_a_frame_of_as_many_trees(rt):
    import torch
    w, h, r0, r1 = 64, 120, 20, 52                                   # 64 x 32 rows x 9 = 18,432 trees
    P, n, rays, _ = R.camera_set("ref", False)
    flat = rays.reshape(-1, 6)
    many = np.concatenate([flat, flat[:w * (r1 - r0) * 9 - len(flat)]])
    assert len(many) == 18432
    sizes = {}
    rt.lib().rt_release()
    call = Call(rt, P, n, many, False)
    rt.check(call.issue())
    torch.cuda.synchronize()
    sizes["trace"] = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    rt.whitted_trace(many, P, n)
    sizes["blocking trace"] = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    d_frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    rt.check(rt.lib().rtw_render_async(call.d_prims.data_ptr(), n, d_frame.data_ptr(), w, h, r0, r1, None,
                                       torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    sizes["frame"] = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    assert 0 < sizes["trace"] <= sizes["frame"] and sizes["blocking trace"] == sizes["trace"], sizes


# ---------------------------------------------------------------- 11. arguments
def test_argument_errors_come_before_any_device_work(rt):
    """Every refusal returns RT_ERR_INVALID and writes nothing: real rays and
    primitives, sentinel-filled outputs (device buffers for rtw_trace_async,
    host arrays for rtw_trace) that are untouched after a synchronise, counters
    included.  So are they after nrays == 0, which is RT_OK."""
    import torch
    P, n, rays, _ = R.camera_set("ref", False)
    flat = np.ascontiguousarray(rays.reshape(-1, 6)[:64])
    call = Call(rt, P, n, flat, False)
    call.cnt.fill_(FILL_I)
    h_prims = np.frombuffer(P, dtype=np.uint8, count=96 * n).copy()
    h_col, h_t = np.full(3 * 64, FILL_F, F), np.full(64, FILL_F, F)
    h_id, h_cnt = np.full(64, FILL_I, np.int32), np.full(4, 12345, np.uint64)
    fn, blocking = rt.entry("rtw_trace_async"), rt.entry("rtw_trace")
    dev_args = dict(prims=call.d_prims.data_ptr(), nprims=n, rays=call.d_rays.data_ptr(), nrays=64, flags=0,
                    color=call.col.data_ptr())
    host_args = dict(prims=h_prims.ctypes.data, nprims=n, rays=flat.ctypes.data, nrays=64, flags=0,
                     color=h_col.ctypes.data)
    dev_tail = (call.t.data_ptr(), call.ids.data_ptr(), call.cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    host_tail = (h_t.ctypes.data, h_id.ctypes.data, h_cnt.ctypes.data)

    def untouched():
        torch.cuda.synchronize()
        assert (call.col.cpu().numpy() == F(FILL_F)).all() and (call.t.cpu().numpy() == F(FILL_F)).all()
        assert (call.ids.cpu().numpy() == FILL_I).all() and (call.cnt.cpu().numpy() == FILL_I).all()
        assert (h_col == F(FILL_F)).all() and (h_t == F(FILL_F)).all() and (h_id == FILL_I).all()

    bad = [dict(prims=None), dict(rays=None), dict(color=None), dict(nprims=0), dict(nprims=65), dict(flags=2),
           dict(flags=-1), dict(nrays=2 ** 31)]
    for kw in bad:
        for f, base, tail in ((fn, dev_args, dev_tail), (blocking, host_args, host_tail)):
            a = dict(base)
            a.update(kw)
            rc = f(a["prims"], a["nprims"], a["rays"], a["nrays"], a["flags"], a["color"], *tail)
            assert rc == -1, (kw, rc)
            assert b"rtw_trace" in rt.lib().rt_last_error()
        untouched()
        assert (h_cnt == 12345).all()                     # (a refused blocking call leaves the host counters too)
    # nrays == 0: RT_OK, nothing launched, nothing written but the blocking form's counters (this call's: 0)
    for f, base, tail in ((fn, dev_args, dev_tail), (blocking, host_args, host_tail)):
        a = dict(base, nrays=0, flags=1)
        assert f(a["prims"], a["nprims"], a["rays"], 0, a["flags"], a["color"], *tail) == 0
    untouched()
    assert (h_cnt == 0).all()


# ---------------------------------------------------------------- 12. the pool fractions
def diffuse_scene():
    """The reference scene without mirrors or glass: no tree has children, so a
    record pool of any size holds every frame."""
    P, n = O.whitted_scene()
    for p in P[:n]:
        p.m_Refl = p.m_Refr = 0.0
    return P, n


def test_traces_of_many_sizes_leave_a_frame_sizes_fraction_alone(rt):
    """A frame size's learnt pool fraction survives more than 16 traces of
    different sizes (the frames' table has 16 entries).  The frame learns a
    small fraction (RT_POOL_FRAC at its entry's creation: 0.05 of its trees,
    enough for a scene without children); were its entry evicted, the next
    frame of that size would start from the default 0.9 again and the arena,
    which only grows, would come out larger."""
    import torch
    w, h, r0, r1 = 64, 120, 20, 52
    P, n = diffuse_scene()
    ref, rcnt = O.whitted_render(w, h, r0, r1, nthreads=R.NT, prims=P, n=n)
    d_prims = prim_bytes(P, n)
    d_frame = torch.zeros((h, w), dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def frame():
        d_frame.zero_()
        rt.check(rt.lib().rtw_render_async(d_prims.data_ptr(), n, d_frame.data_ptr(), w, h, r0, r1, None, s))
        torch.cuda.synchronize()
        assert (d_frame.cpu().numpy().view(np.uint32) == ref).all()
        return rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    with env(RT_POOL_FRAC=0.05):
        before = frame()
    Pt, nt, rays, _ = R.camera_set("ref", False)
    flat = rays.reshape(-1, 6)
    sizes = [37 * k + 1 for k in range(1, 21)]                       # 20 sizes, up to 741 rays
    for k in sizes:
        sel = flat[5000:5000 + k]
        agree("%d rays" % k, gpu_trace(rt, Pt, nt, sel, False), R.trace(Pt, nt, sel))
    assert rt.lib().rt_cached_bytes() == before                      # (their arenas fit into the frame's)
    after = frame()
    rt.lib().rt_release()
    assert after == before, (before, after)


def test_a_trace_learns_its_fraction_per_size_bucket(rt):
    """A trace whose pool overflowed enlarges the pool of the next trace in
    its power-of-two size bucket, whatever that one's exact ray count: after
    16,128 rays at a pool of 0.25 (4,032 records, one 4,096-record page row,
    for 21,159 child nodes), 16,000 rays get 0.3125 (5,000: two page rows) --
    a larger arena, though of fewer rays."""
    P, n, rays, ref = R.camera_set("ref", False)
    flat = rays.reshape(-1, 6)
    rt.lib().rt_release()
    assert ref[3][0] - len(flat) == 21159
    with env(RT_POOL_FRAC=0.25):
        agree("first", gpu_trace(rt, P, n, flat, False), ref)
        first = rt.lib().rt_cached_bytes()
        agree("second", gpu_trace(rt, P, n, flat[:16000], False), R.trace(P, n, flat[:16000]))
        second = rt.lib().rt_cached_bytes()
    rt.lib().rt_release()
    assert second > first, (first, second)
