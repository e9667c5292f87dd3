"""rtamd -- host-side Python binding of the MI355X ray-trace hot path.

Thin ctypes layer over librt_hip.so (include/rt_hip.h).  The C++ drop-in
shims (csrc/shim_*.cpp) are the reference-facing host API; this module is
what the tests, bench.py and __graft_entry__ drive.

    Whitted  : whitted_render()  ~ Engine_InitRender + Engine_Render
               (raytracer3.0.06.no_rec.samp/raytracer.cpp:278-530) on the GPU
    smallpt  : SmallptFrame.render(k)  ~ k x UpdateRenderingCPU
               (smallptgpu-v1.6/smallptCPU.cpp:77-132) on the GPU, or
               tiled in row bands over several GPUs (devices=[...]);
               SmallptMulti: the device-resident multi-GPU frame (spt_multi_*);
               SmallptDeviceFrame (device.py): one prepared scene plus
               device-resident buffers, launched asynchronously
               (spt_scene_render_async / _groups_async / _list_async)
    Queue    : queue_render()  ~ raytracer_non_kernel
               (Raytracer3.2.03/.../raytracer_non_OpenCL.c:285-449) on the GPU
    Queries  : SmallptScene.query() / .radiance() on a prepared smallpt scene;
               PrimScene.query() on the Whitted or the queue tracer's
               primitives (rtp_query_async): nearest hit, shadowed or not,
               the first occluder;
               whitted_trace() / whitted_trace_async(): the colour the Whitted
               tracer computes along the caller's rays (rtw_trace_async);
               queue_trace() / queue_trace_async(): the queue tracer's, along
               the caller's chains of rays (rtq_trace_async)
"""
import ctypes as C

import numpy as np

from . import ppm, scenes
from .device import SmallptDeviceFrame
from ._lib import (Camera, Float4, Primitive, QPrimitive, RTError, Sphere, Vec3, check, device_count, entry, lib,
                   set_device, SPT_COST_MAX, SPT_COUNT_RAYS, SPT_LIST_SET, SPT_DIRECT_LIGHTING, SPT_PATH_TRACING,
                   SPT_QUERY_ANY, SPT_QUERY_NEAREST, SPT_QUERY_OCCLUDER, RTP_QUERY_NEAREST, RTP_QUERY_SHADOW,
                   RTP_QUERY_OCCLUDER, RTW_TRACE_OCL)

__all__ = ["Camera", "Primitive", "QPrimitive", "Float4", "Sphere", "Vec3", "RTError", "scenes", "lib", "check",
           "device_count", "set_device", "whitted_render", "whitted_trace", "whitted_trace_async",
           "RTW_TRACE_OCL", "queue_render", "queue_trace", "queue_trace_async", "SmallptFrame", "SmallptScene",
           "SmallptMulti", "SmallptDeviceFrame", "PrimScene",
           "SPT_PATH_TRACING", "SPT_DIRECT_LIGHTING", "SPT_COUNT_RAYS", "SPT_COST_MAX", "SPT_LIST_SET",
           "SPT_QUERY_NEAREST", "SPT_QUERY_ANY", "SPT_QUERY_OCCLUDER",
           "RTP_QUERY_NEAREST", "RTP_QUERY_SHADOW", "RTP_QUERY_OCCLUDER"]


def whitted_render(w, h, row_begin=20, row_end=None, prims=None, nprims=None, frame=None,
                   counters=False):
    """Render rows [row_begin,row_end) (default the reference window
    [20, h-70)) into a uint32 [h, w] frame (zero-cleared unless given).
    Returns frame, or (frame, [traced, shadow, tests, tir]) if counters."""
    if prims is None:
        prims, nprims = scenes.whitted_scene()
    if row_end is None:
        row_end = h - 70
    if frame is None:
        frame = np.zeros((h, w), dtype=np.uint32)
    assert frame.dtype == np.uint32 and frame.shape == (h, w) and frame.flags.c_contiguous
    cnt = (C.c_uint64 * 4)()
    check(lib().rtw_render(C.addressof(prims), nprims, frame.ctypes.data, w, h, row_begin,
                           row_end, C.addressof(cnt) if counters else None))
    return (frame, list(cnt)) if counters else frame


def whitted_render_ocl(w, h, prims=None, nprims=None, frame=None, counters=False):
    """The reference's OpenCL kernel semantics (raytrace_kernel of
    openCLcode.cl): rows [20, min(530, h)) of a uint32 [h, w] frame."""
    if prims is None:
        prims, nprims = scenes.whitted_scene()
    if frame is None:
        frame = np.zeros((h, w), dtype=np.uint32)
    assert frame.dtype == np.uint32 and frame.shape == (h, w) and frame.flags.c_contiguous
    cnt = (C.c_uint64 * 4)()
    check(lib().rtw_render_ocl(C.addressof(prims), nprims, frame.ctypes.data, w, h,
                               C.addressof(cnt) if counters else None))
    return (frame, list(cnt)) if counters else frame


def whitted_trace(rays, prims=None, nprims=None, ocl=False, counters=False):
    """The colour the Whitted tracer computes along each ray (rtw_trace;
    blocking, numpy): `rays` is float32 [..., 6] (o.xyz, d.xyz; the direction
    is used as given), e.g. scenes.whitted_camera_rays().  One sub-sample's
    63-node ray tree and back-accumulation per ray, bit for bit the
    reference's; ocl: openCLcode.cl's semantics.  Returns (colours float32
    [n, 3], t float32 [n] -- the root's distance, 1e6 on a miss --, id int32
    [n] -- the root's primitive or -1), and [traced, shadow, tests, tir] as a
    fourth item if counters.  scenes.whitted_pack() turns a pixel's
    sub-sample colours into the frame's word."""
    if prims is None:
        prims, nprims = scenes.whitted_scene()
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = rays.shape[0]
    col = np.empty((n, 3), np.float32)
    t = np.empty(n, np.float32)
    ids = np.empty(n, np.int32)
    cnt = (C.c_uint64 * 4)()
    check(entry("rtw_trace")(C.addressof(prims), nprims, rays.ctypes.data, n, RTW_TRACE_OCL if ocl else 0,
                             col.ctypes.data, t.ctypes.data, ids.ctypes.data, C.addressof(cnt) if counters else None))
    return (col, t, ids, list(cnt)) if counters else (col, t, ids)


def whitted_trace_async(rays, d_prims, nprims, ocl=False, out=None, counters=None, stream=None):
    """whitted_trace on device memory (rtw_trace_async): `rays` a contiguous
    float32 device tensor [n, 6]; `d_prims` a contiguous device tensor of any
    dtype holding at least nprims 96-byte primitives (a uint8 tensor made from
    the ctypes array's bytes, say) or a raw device address.  out=(colours, t,
    id) takes the caller's tensors (float32 [n, 3], float32 [n], int32 [n]; t
    and id may be None, which leaves that output out); by default all three
    are allocated.  counters: an int64 device tensor [4] accumulated into.
    Asynchronous on `stream` (a torch stream or a raw handle; default: torch's
    current stream), ordered with the level-pass frames as rtw_render_async
    is; not for graph capture.  Returns (colours, t, id)."""
    import torch
    if not (rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 6
            and rays.is_contiguous()):
        raise ValueError("whitted_trace_async: rays must be a contiguous float32 device tensor [n, 6]")
    n = rays.shape[0]
    if hasattr(d_prims, "data_ptr"):
        if not (d_prims.is_cuda and d_prims.is_contiguous()
                and d_prims.numel() * d_prims.element_size() >= C.sizeof(Primitive) * max(int(nprims), 0)):
            raise ValueError("whitted_trace_async: d_prims must be a contiguous device tensor of at least "
                             "96 x nprims bytes")
        d_prims = d_prims.data_ptr()
    if out is None:
        col = torch.empty((n, 3), dtype=torch.float32, device=rays.device)
        t = torch.empty(n, dtype=torch.float32, device=rays.device)
        ids = torch.empty(n, dtype=torch.int32, device=rays.device)
    else:
        col, t, ids = out
        for x, dt, numel in ((col, torch.float32, 3 * n), (t, torch.float32, n), (ids, torch.int32, n)):
            if (x is None and x is not col) or (x is not None and x.is_cuda and x.dtype == dt and x.numel() >= numel
                                                  and x.is_contiguous()):
                continue
            raise ValueError("whitted_trace_async: out must hold contiguous device tensors: float32 [n, 3], "
                             "float32 [n] or None, int32 [n] or None")
    if counters is not None and not (counters.is_cuda and counters.dtype == torch.int64 and counters.numel() == 4
                                     and counters.is_contiguous()):
        raise ValueError("whitted_trace_async: counters must be a contiguous int64 device tensor [4]")
    if stream is None:
        stream = torch.cuda.current_stream(rays.device)
    stream = getattr(stream, "cuda_stream", stream)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    if n:                                                  # (an empty tensor has no address to pass)
        check(entry("rtw_trace_async")(d_prims, nprims, rays.data_ptr(), n, RTW_TRACE_OCL if ocl else 0, ptr(col),
                                       ptr(t), ptr(ids), ptr(counters), stream))
    return col, t, ids


def queue_render(w, h, prims=None, nprims=None, counters=False):
    """raytracer_non_kernel on the GPU: the uchar4 (r, g, b, 0) frame as
    uint8 [h, w, 4].  Returns frame, or (frame, [rays, shadow rays, intersect
    calls, undefined-behaviour events]) if counters."""
    if prims is None:
        prims, nprims = scenes.queue_scene()
    frame = np.zeros((h, w, 4), dtype=np.uint8)
    cnt = (C.c_uint64 * 4)()
    check(lib().rtq_render(C.addressof(prims), nprims, frame.ctypes.data, w, h,
                           C.addressof(cnt) if counters else None))
    return (frame, list(cnt)) if counters else frame


def queue_trace(rays, prims=None, nprims=None, group=1, counters=False):
    """The colour the queue tracer computes along the caller's rays (rtq_trace;
    blocking, numpy): `rays` is float32 [..., 6] (o.xyz, d.xyz; the direction
    is used as given), e.g. scenes.queue_camera_rays().  `group` (1..64)
    consecutive rays form a chain: one accumulator that every node of their
    trees is added to in the reference's queue order, as a pixel's nine
    primaries are -- group=1 is the colour along one ray, group=9 over a
    frame's camera rays the frame's pixel sums (scenes.queue_pack() packs
    them).  Returns (colours float32 [n / group, 3], t float32 [n] -- the
    root's distance, 1e7 on a miss --, id int32 [n] -- the root's primitive or
    -1), and [rays, shadow rays, intersect calls, undefined-behaviour events]
    as a fourth item if counters."""
    if prims is None:
        prims, nprims = scenes.queue_scene()
    rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
    n = rays.shape[0]
    col = np.empty((n // group if 1 <= group <= 64 else 0, 3), np.float32)
    t = np.empty(n, np.float32)
    ids = np.empty(n, np.int32)
    cnt = (C.c_uint64 * 4)()
    check(entry("rtq_trace")(C.addressof(prims), nprims, rays.ctypes.data, n, group, col.ctypes.data, t.ctypes.data,
                             ids.ctypes.data, C.addressof(cnt) if counters else None))
    return (col, t, ids, list(cnt)) if counters else (col, t, ids)


def queue_trace_async(rays, d_prims, nprims, group=1, out=None, counters=None, stream=None):
    """queue_trace on device memory (rtq_trace_async): `rays` a contiguous
    float32 device tensor [n, 6], n a multiple of `group`; `d_prims` a
    contiguous device tensor of any dtype holding at least nprims 96-byte
    primitives or a raw device address.  out=(colours, t, id) takes the
    caller's tensors (float32 [n / group, 3], float32 [n], int32 [n]; t and id
    may be None, which leaves that output out); by default all three are
    allocated.  counters: an int64 device tensor [4] accumulated into.
    Asynchronous on `stream` (a torch stream or a raw handle; default: torch's
    current stream), ordered with the level-pass frames as rtq_render_async
    is; not for graph capture.  Returns (colours, t, id)."""
    import torch
    if not (rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 6
            and rays.is_contiguous()):
        raise ValueError("queue_trace_async: rays must be a contiguous float32 device tensor [n, 6]")
    n = rays.shape[0]
    if not (isinstance(group, int) and 1 <= group <= 64 and n % group == 0):
        raise ValueError("queue_trace_async: group must be 1..64 and divide the number of rays")
    nc = n // group
    if hasattr(d_prims, "data_ptr"):
        if not (d_prims.is_cuda and d_prims.is_contiguous()
                and d_prims.numel() * d_prims.element_size() >= C.sizeof(QPrimitive) * max(int(nprims), 0)):
            raise ValueError("queue_trace_async: d_prims must be a contiguous device tensor of at least "
                             "96 x nprims bytes")
        d_prims = d_prims.data_ptr()
    if out is None:
        col = torch.empty((nc, 3), dtype=torch.float32, device=rays.device)
        t = torch.empty(n, dtype=torch.float32, device=rays.device)
        ids = torch.empty(n, dtype=torch.int32, device=rays.device)
    else:
        col, t, ids = out
        for x, dt, numel in ((col, torch.float32, 3 * nc), (t, torch.float32, n), (ids, torch.int32, n)):
            if (x is None and x is not col) or (x is not None and x.is_cuda and x.dtype == dt and x.numel() >= numel
                                                  and x.is_contiguous()):
                continue
            raise ValueError("queue_trace_async: out must hold contiguous device tensors: float32 [n / group, 3], "
                             "float32 [n] or None, int32 [n] or None")
    if counters is not None and not (counters.is_cuda and counters.dtype == torch.int64 and counters.numel() == 4
                                     and counters.is_contiguous()):
        raise ValueError("queue_trace_async: counters must be a contiguous int64 device tensor [4]")
    if stream is None:
        stream = torch.cuda.current_stream(rays.device)
    stream = getattr(stream, "cuda_stream", stream)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    if n:                                                  # (an empty tensor has no address to pass)
        check(entry("rtq_trace_async")(d_prims, nprims, rays.data_ptr(), n, group, ptr(col), ptr(t), ptr(ids),
                                       ptr(counters), stream))
    return col, t, ids


class SmallptFrame:
    """Progressive smallpt frame state: colors / seeds / pixels exactly as
    smallptGPU.cpp's AllocateBuffers lays them out, and currentSample."""

    def __init__(self, w, h, spheres=None, nspheres=None, camera=None, seed=1,
                 mode=SPT_PATH_TRACING):
        if spheres is None:
            spheres, nspheres = scenes.cornell()
        if camera is None:
            camera = scenes.cornell_camera(w, h)
        self.w, self.h = w, h
        self.spheres, self.nspheres, self.camera, self.mode = spheres, nspheres, camera, mode
        self.colors = np.zeros(3 * w * h, dtype=np.float32)
        self.seeds = scenes.seeds(w, h, seed)
        self.pixels = np.zeros(w * h, dtype=np.uint32)
        self.current_sample = 0
        self.counters = [0, 0, 0, 0]

    def render(self, nsamples=1, counters=True, devices=None):
        """nsamples successive UpdateRenderingCPU passes on the GPU.  With
        counters=False no counter buffer is passed (the kernels without the
        work counters: the ones bench.py times).  devices=[d0, d1, ...]: the
        frame tiled in row bands over those devices (spt_render_multi; a
        device may repeat)."""
        cnt = (C.c_uint64 * 4)()
        args = (C.addressof(self.spheres), self.nspheres, C.byref(self.camera), self.colors.ctypes.data,
                self.seeds.ctypes.data, self.pixels.ctypes.data, self.w, self.h, self.current_sample,
                nsamples, self.mode, C.addressof(cnt) if counters else None)
        if devices is None:
            check(lib().spt_render(*args))
        else:
            devs = (C.c_int * len(devices))(*devices)
            check(lib().spt_render_multi(*args, devs, len(devices)))
        self.current_sample += nsamples
        self.counters = [a + b for a, b in zip(self.counters, cnt)]
        return self


class SmallptScene:
    """Prepared device scene (spt_scene_create); .handle is passed to
    spt_scene_render_async.  Freed with close() / garbage collection."""

    def __init__(self, spheres, nspheres):
        self.handle = C.c_void_p()
        check(lib().spt_scene_create(C.addressof(spheres), nspheres, C.byref(self.handle)))
        self.n = nspheres

    # spt_scene_info's words in order (include/rt_hip.h); "family" is one of FAMILIES
    FAMILIES = ("GEO_LDS", "GEO_GLOBAL", "GEO_BVH", "GEO_WIDE")
    INFO = ("family", "nspheres", "nlights", "nalways", "nodes", "wnodes", "wdepth", "leaf_max", "no_refr",
            "launches", "wpb", "nblocks", "cg", "n1", "n2", "two_query", "lds_bytes")

    def info(self):
        """The scene's kernel family and hierarchy layout, and the shape and
        tiers of the most recent launch on it (spt_scene_info): a dict keyed
        by INFO.  Host bookkeeping only, no device work."""
        out = (C.c_int * len(self.INFO))()
        check(lib().spt_scene_info(self.handle, out, len(out)))
        d = dict(zip(self.INFO, out))
        d["family"] = self.FAMILIES[d["family"]]
        d["no_refr"], d["two_query"] = bool(d["no_refr"]), bool(d["two_query"])
        return d

    def update(self, spheres, first=0, count=None, stream=None):
        """Replaces spheres [first, first + count) with spheres[0 .. count) in
        place (spt_scene_update_async): asynchronous on `stream` (a torch
        stream or a raw handle; default: torch's current stream where torch
        is loaded, else the null stream), a hierarchy is refitted on the
        device.  `spheres` is a Sphere array, or a pointer to one (then give
        count); it is free again when the call returns.  count defaults to the
        array's length."""
        if count is None:
            count = len(spheres)
        ptr = None if spheres is None else C.cast(spheres, C.c_void_p)
        check(entry("spt_scene_update_async")(self.handle, ptr, first, count, self._stream(stream)))

    # spt_scene_update_info's words in order
    UPDATE_INFO = ("updates", "refits", "light_rebuilds", "reallocations", "metadata_bytes")

    def update_info(self):
        """Host bookkeeping of update() (spt_scene_update_info): a dict keyed by UPDATE_INFO."""
        out = (C.c_uint64 * len(self.UPDATE_INFO))()
        check(entry("spt_scene_update_info")(self.handle, out, len(out)))
        return dict(zip(self.UPDATE_INFO, (int(v) for v in out)))

    def regroup(self, stream=None):
        """Re-deals the scene's current spheres into the frozen shape of its
        hierarchy on the device and refits (spt_scene_regroup_async):
        asynchronous on `stream` (as update()), the frames keep their bits,
        the walks get tighter leaves.  Nothing happens on a scene without a
        hierarchy."""
        check(entry("spt_scene_regroup_async")(self.handle, self._stream(stream)))

    # spt_scene_regroup_info's words in order
    REGROUP_INFO = ("regroups", "levels", "global_levels", "bytes")

    def regroup_info(self):
        """Host bookkeeping of regroup() (spt_scene_regroup_info): a dict keyed by REGROUP_INFO."""
        out = (C.c_uint64 * len(self.REGROUP_INFO))()
        check(entry("spt_scene_regroup_info")(self.handle, out, len(out)))
        return dict(zip(self.REGROUP_INFO, (int(v) for v in out)))

    @staticmethod
    def _stream(stream):
        """`stream` as a raw handle; None: torch's current stream where torch is in use, else the null stream."""
        if stream is None:
            import sys
            torch = sys.modules.get("torch")
            stream = torch.cuda.current_stream() if torch is not None and torch.cuda.is_initialized() else None
        return getattr(stream, "cuda_stream", stream)

    def move(self, geom, first=0, stream=None):
        """Moves spheres [first, first + count) to the centres and radii in
        `geom` (spt_scene_move_async): a contiguous float32 device tensor
        [count, 4] of p.x, p.y, p.z, rad, 16-byte aligned, on the scene's
        device.  Emission, colour and refl stay.  Asynchronous on `stream` (as
        update()); nothing is copied to or from the host and `geom` may be
        overwritten in stream order right after the call.  On a capturing
        stream the move is recorded (move_prepare() first); a replay reads what
        `geom` holds then."""
        import torch
        if not (isinstance(geom, torch.Tensor) and geom.is_cuda and geom.dtype == torch.float32 and geom.dim() == 2
                and geom.shape[1] == 4 and geom.is_contiguous()):
            raise ValueError("move: geom must be a contiguous float32 device tensor [count, 4]")
        if geom.shape[0] == 0:                                 # (an empty tensor has no address to pass)
            return
        check(entry("spt_scene_move_async")(self.handle, geom.data_ptr(), first, geom.shape[0], self._stream(stream)))

    def move_prepare(self, stream=None):
        """Builds what move() relies on (spt_scene_move_prepare): the refit
        metadata, the light indices on the device, one whole-scene refit on
        `stream`.  Allocates and waits for `stream`; needed before a move is
        captured, optional otherwise (the first uncaptured move does it)."""
        check(entry("spt_scene_move_prepare")(self.handle, self._stream(stream)))

    # spt_scene_move_info's words in order
    MOVE_INFO = ("moves", "captured", "refits")

    def move_info(self):
        """Host bookkeeping of move() (spt_scene_move_info): a dict keyed by MOVE_INFO."""
        out = (C.c_uint64 * len(self.MOVE_INFO))()
        check(entry("spt_scene_move_info")(self.handle, out, len(out)))
        return dict(zip(self.MOVE_INFO, (int(v) for v in out)))

    def spheres(self):
        """The spheres as the device holds them (spt_scene_read_spheres; waits
        for the device): float32 [n, 11] rows of rad, p, e, c and refl as raw
        bits -- Sphere's layout."""
        rows = np.zeros((self.n, 11), np.float32)
        check(entry("spt_scene_read_spheres")(self.handle, rows.ctypes.data, self.n))
        return rows

    def hierarchy(self):
        """The hierarchy as the device holds it (spt_scene_read_hierarchy;
        waits for the device): "nodes" float32 [16 x binary nodes, 4] (the
        eight octant layouts, two rows per record), "geo" float32 [entries, 4],
        "ids" int32 [entries], "wide" uint32 [8-wide nodes, 28], "maxid" uint32
        [8-wide nodes, 8]; every array empty for a scene without one."""
        read = entry("spt_scene_read_hierarchy")
        sizes = (C.c_size_t * 5)()
        check(read(self.handle, None, 0, sizes))
        raw = np.zeros(max(sum(sizes), 1), np.uint8)
        check(read(self.handle, raw.ctypes.data, raw.nbytes, sizes))
        kinds = (("nodes", np.float32, (-1, 4)), ("geo", np.float32, (-1, 4)), ("ids", np.int32, (-1,)),
                 ("wide", np.uint32, (-1, 28)), ("maxid", np.uint32, (-1, 8)))
        out, o = {}, 0
        for (name, kind, shape), nbytes in zip(kinds, sizes):
            out[name] = raw[o:o + nbytes].view(kind).reshape(shape)
            o += nbytes
        return out

    # query kinds by name (include/rt_hip.h SPT_QUERY_*)
    QUERY_KINDS = {"nearest": SPT_QUERY_NEAREST, "any": SPT_QUERY_ANY, "occluder": SPT_QUERY_OCCLUDER}

    def query(self, rays, tmax=None, kind="nearest", out=None, stream=None):
        """What the rays hit (spt_scene_query_async): `rays` is a contiguous
        float32 device tensor [n, 6] (o.xyz, d.xyz; the direction is used as
        given), `tmax` a float32 device tensor [n] -- required for "any" and
        "occluder", the optional initial bound of "nearest".  Returns (t, id):
        "nearest" the distance (float32; on a miss the bound's bits) and the
        sphere index or -1; "any" (None, 1 or 0); "occluder" (None, the highest
        occluder's index or -1); id is int32.  out=(t, id) takes the caller's
        tensors (for "nearest" either may be None; the occlusion kinds use
        id only).  Asynchronous on `stream` (a torch stream or a raw handle;
        default: torch's current stream); allocates only the outputs it was
        not given."""
        import torch
        if kind not in self.QUERY_KINDS:
            raise ValueError("query: kind %r is not one of %s" % (kind, sorted(self.QUERY_KINDS)))
        if not (rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 6
                and rays.is_contiguous()):
            raise ValueError("query: rays must be a contiguous float32 device tensor [n, 6]")
        n = rays.shape[0]
        if tmax is not None and not (tmax.is_cuda and tmax.dtype == torch.float32 and tmax.numel() == n
                                     and tmax.is_contiguous()):
            raise ValueError("query: tmax must be a contiguous float32 device tensor [n]")
        nearest = kind == "nearest"
        if out is None:
            t = torch.empty(n, dtype=torch.float32, device=rays.device) if nearest else None
            ids = torch.empty(n, dtype=torch.int32, device=rays.device)
        else:
            t, ids = out
            t = t if nearest else None
            for x, dt in ((t, torch.float32), (ids, torch.int32)):
                if x is not None and not (x.is_cuda and x.dtype == dt and x.numel() == n and x.is_contiguous()):
                    raise ValueError("query: out must hold contiguous device tensors [n], float32 and int32")
        if stream is None:
            stream = torch.cuda.current_stream(rays.device)
        stream = getattr(stream, "cuda_stream", stream)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        if n:                                                  # (an empty tensor has no address to pass)
            check(entry("spt_scene_query_async")(self.handle, rays.data_ptr(), ptr(tmax), n, self.QUERY_KINDS[kind],
                                                 ptr(t), ptr(ids), stream))
        return t, ids

    def radiance(self, rays, seeds, nsamples=1, first_sample=0, mode=SPT_PATH_TRACING, out=None, seeds_out=None,
                 stream=None):
        """The reference's radiance along the rays (spt_scene_radiance_async):
        `rays` as for query(); `seeds` a contiguous int32 device tensor [n, 2]
        (SmallptDeviceFrame's seed dtype; the 32-bit patterns of the two MWC
        words), each ray's RNG state.  Samples first_sample .. first_sample +
        nsamples - 1 of RadiancePathTracing (or, mode=SPT_DIRECT_LIGHTING,
        RadianceDirectLighting) are folded into the running average `out`
        (float32 [n, 3]; read when first_sample > 0, so then required).
        Returns (radiance, seeds): `out` or a new tensor, and the advanced
        states in `seeds_out` (which may be `seeds` itself) or a new tensor.
        Asynchronous on `stream` (a torch stream or a raw handle; default:
        torch's current stream); allocates only the outputs it was not given."""
        import torch
        if not (rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 6
                and rays.is_contiguous()):
            raise ValueError("radiance: rays must be a contiguous float32 device tensor [n, 6]")
        n = rays.shape[0]

        def is_seeds(x):
            return (x.is_cuda and x.dtype == torch.int32 and x.dim() == 2 and tuple(x.shape) == (n, 2)
                    and x.is_contiguous())
        if not is_seeds(seeds):
            raise ValueError("radiance: seeds must be a contiguous int32 device tensor [n, 2]")
        if seeds_out is not None and not is_seeds(seeds_out):
            raise ValueError("radiance: seeds_out must be a contiguous int32 device tensor [n, 2]")
        if out is not None and not (out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (n, 3)
                                    and out.is_contiguous()):
            raise ValueError("radiance: out must be a contiguous float32 device tensor [n, 3]")
        if nsamples < 0 or first_sample < 0:
            raise ValueError("radiance: nsamples and first_sample must not be negative")
        if out is None:
            if first_sample > 0:
                raise ValueError("radiance: first_sample > 0 continues the running average in out=")
            out = torch.zeros((n, 3), dtype=torch.float32, device=rays.device)
        if seeds_out is None:
            seeds_out = torch.empty_like(seeds)
        if stream is None:
            stream = torch.cuda.current_stream(rays.device)
        stream = getattr(stream, "cuda_stream", stream)
        if n:                                                  # (an empty tensor has no address to pass)
            check(entry("spt_scene_radiance_async")(self.handle, rays.data_ptr(), n, seeds.data_ptr(),
                                                    seeds_out.data_ptr(), out.data_ptr(), first_sample, nsamples,
                                                    mode, stream))
        return out, seeds_out

    def pick(self, cam, w, h, x, y):
        """The sphere under pixel (x, y) of a w x h view through `cam` -- the
        pixel `pixels` holds at y * w + x: (id, t) of the pixel-centre camera
        ray's nearest hit (scenes.camera_rays; id -1 on a miss).  Blocking."""
        import torch
        if not (0 <= x < w and 0 <= y < h):
            raise ValueError("pick: pixel (%d, %d) outside %d x %d" % (x, y, w, h))
        t, ids = self.query(torch.from_numpy(scenes.camera_rays(cam, w, h, [x], [y])).cuda())
        return int(ids.cpu()[0]), float(t.cpu()[0])

    def close(self):
        if self.handle:
            lib().spt_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PrimScene:
    """The Whitted or the queue tracer's primitives prepared for ray queries
    (rtw_prims_create / rtq_prims_create): `prims` is a host array of
    Primitive (tracer="whitted") or QPrimitive (tracer="queue"), 1..64 of
    them.  .handle is passed to rtp_query_async.  Freed with close() / garbage
    collection."""

    TRACERS = {"whitted": ("rtw_prims_create", "rtw_prims_set_async", Primitive),
               "queue": ("rtq_prims_create", "rtq_prims_set_async", QPrimitive)}
    # query kinds by name (include/rt_hip.h RTP_QUERY_*)
    QUERY_KINDS = {"nearest": RTP_QUERY_NEAREST, "shadow": RTP_QUERY_SHADOW, "occluder": RTP_QUERY_OCCLUDER}
    FAR = {"whitted": 1000000.0, "queue": 10000000.0}      # d_t of a miss

    def __init__(self, prims, nprims, tracer="whitted"):
        if tracer not in self.TRACERS:
            raise ValueError("PrimScene: tracer %r is not one of %s" % (tracer, sorted(self.TRACERS)))
        self.tracer, self.n = tracer, nprims
        self.handle = C.c_void_p()
        ptr = None if prims is None else C.cast(prims, C.c_void_p)
        check(entry(self.TRACERS[tracer][0])(ptr, nprims, C.byref(self.handle)))

    def set(self, d_prims, nprims, stream=None):
        """Replaces the whole primitive array (rtw_ / rtq_prims_set_async) from
        DEVICE memory: `d_prims` is a contiguous torch device tensor of any
        dtype holding at least nprims 96-byte primitives (a uint8 tensor made
        from the ctypes array's bytes, say), or a raw device address (an int).
        nprims may differ from the scene's.  Asynchronous on `stream` (a torch
        stream or a raw handle; default: torch's current stream where torch is
        loaded, else the null stream): queries enqueued after it on that
        stream see the new primitives.  The tensor must stay alive until the
        stream has passed the call."""
        size = C.sizeof(self.TRACERS[self.tracer][2])
        if hasattr(d_prims, "data_ptr"):
            if not (d_prims.is_cuda and d_prims.is_contiguous()
                    and d_prims.numel() * d_prims.element_size() >= size * max(int(nprims), 0)):
                raise ValueError("set: d_prims must be a contiguous device tensor of at least %d x nprims bytes" % size)
            dev, d_prims = d_prims.device, d_prims.data_ptr()
        else:
            dev = None
        if stream is None:
            import sys
            torch = sys.modules.get("torch")
            stream = torch.cuda.current_stream(dev) if torch is not None and torch.cuda.is_initialized() else None
        stream = getattr(stream, "cuda_stream", stream)
        check(entry(self.TRACERS[self.tracer][1])(self.handle, d_prims, nprims, stream))
        self.n = nprims

    def query(self, rays, tmax=None, kind="nearest", out=None, stream=None):
        """What the rays hit (rtp_query_async): `rays` is a contiguous float32
        device tensor [n, 6] (o.xyz, d.xyz; the direction is used as given),
        `tmax` a float32 device tensor [n] -- required for "shadow" and
        "occluder" (the distance an occluder must be nearer than), the
        optional bound of "nearest" (a hit must be strictly nearer).  Returns
        (t, id, result): "nearest" the distance (float32; FAR[tracer] on a
        miss), the primitive index or -1, and 1 (hit from outside), -1 (from
        inside a sphere) or 0 (miss); "shadow" (None, 1 or 0, None);
        "occluder" (None, the first occluder's index in primitive order or -1,
        None); id and result are int32.  out=(t, id, result) takes the
        caller's tensors: for "nearest" any may be None, which leaves that
        output out (not all three); the shadow kinds use id only.
        Asynchronous on `stream` (a torch stream or a raw handle; default:
        torch's current stream); allocates only the outputs it was not given."""
        import torch
        if kind not in self.QUERY_KINDS:
            raise ValueError("query: kind %r is not one of %s" % (kind, sorted(self.QUERY_KINDS)))
        if not (rays.is_cuda and rays.dtype == torch.float32 and rays.dim() == 2 and rays.shape[1] == 6
                and rays.is_contiguous()):
            raise ValueError("query: rays must be a contiguous float32 device tensor [n, 6]")
        n = rays.shape[0]
        if tmax is not None and not (tmax.is_cuda and tmax.dtype == torch.float32 and tmax.numel() == n
                                     and tmax.is_contiguous()):
            raise ValueError("query: tmax must be a contiguous float32 device tensor [n]")
        nearest = kind == "nearest"
        if not nearest and tmax is None:
            raise ValueError("query: kind %r needs tmax" % kind)
        if out is None:
            t = torch.empty(n, dtype=torch.float32, device=rays.device) if nearest else None
            ids = torch.empty(n, dtype=torch.int32, device=rays.device)
            res = torch.empty(n, dtype=torch.int32, device=rays.device) if nearest else None
        else:
            t, ids, res = out
            t, res = (t, res) if nearest else (None, None)
            for x, dt in ((t, torch.float32), (ids, torch.int32), (res, torch.int32)):
                if x is not None and not (x.is_cuda and x.dtype == dt and x.numel() == n and x.is_contiguous()):
                    raise ValueError("query: out must hold contiguous device tensors [n]: float32, int32, int32")
            if ids is None and (not nearest or (t is None and res is None)):
                raise ValueError("query: out holds no tensor that kind %r writes" % kind)
        if stream is None:
            stream = torch.cuda.current_stream(rays.device)
        stream = getattr(stream, "cuda_stream", stream)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        if n:                                                  # (an empty tensor has no address to pass)
            check(entry("rtp_query_async")(self.handle, rays.data_ptr(), ptr(tmax), n, self.QUERY_KINDS[kind],
                                           ptr(t), ptr(ids), ptr(res), stream))
        return t, ids, res

    def close(self):
        if self.handle:
            lib().rtp_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SmallptMulti:
    """A frame tiled in row bands over several devices (spt_multi_*): band k
    renders pixel rows [h - rows[k+1], h - rows[k]) on devices[k]; gather()
    assembles the whole frame on every band's device (one RCCL all-gather of
    the equal padded bands, or peer copies when a device repeats)."""

    def __init__(self, w, h, devices, spheres=None, nspheres=None):
        if spheres is None:
            spheres, nspheres = scenes.cornell()
        self.w, self.h, self.devices = w, h, list(devices)
        self.handle = C.c_void_p()
        devs = (C.c_int * len(self.devices))(*self.devices)
        check(lib().spt_multi_create(C.addressof(spheres), nspheres, w, h, devs, len(self.devices),
                                     C.byref(self.handle)))
        rows = (C.c_int * (len(self.devices) + 1))()
        check(lib().spt_multi_bands(self.handle, rows))
        self.rows = list(rows)

    def set_scene(self, spheres, nspheres):
        check(lib().spt_multi_set_scene(self.handle, C.addressof(spheres), nspheres))

    def update_scene(self, spheres, first=0, count=None):
        """SmallptScene.update on every band's scene, each on its band's
        stream (spt_multi_update_scene): no band is re-prepared."""
        if count is None:
            count = len(spheres)
        check(entry("spt_multi_update_scene")(self.handle, C.cast(spheres, C.c_void_p), first, count))

    def regroup_scene(self):
        """SmallptScene.regroup on every band's scene, each on its band's
        stream (spt_multi_regroup_scene)."""
        check(entry("spt_multi_regroup_scene")(self.handle))

    def upload(self, seeds, colors=None):
        check(lib().spt_multi_upload(self.handle, colors.ctypes.data if colors is not None else None,
                                     seeds.ctypes.data))

    def render(self, camera, first_sample, nsamples, mode=SPT_PATH_TRACING, counters=False):
        check(lib().spt_multi_render_async(self.handle, C.byref(camera), first_sample, nsamples, mode,
                                           int(bool(counters))))

    def gather(self):
        check(lib().spt_multi_gather_async(self.handle))

    def sync(self):
        check(lib().spt_multi_sync(self.handle))

    def download(self, colors=None, seeds=None, pixels=None):
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        check(lib().spt_multi_download(self.handle, ptr(colors), ptr(seeds), ptr(pixels)))

    def read_frame(self, k):
        """Band k's whole device frame: (colors float32[3*w*h], pixels uint32[w*h])."""
        col = np.empty(3 * self.w * self.h, np.float32)
        px = np.empty(self.w * self.h, np.uint32)
        check(lib().spt_multi_read_frame(self.handle, k, col.ctypes.data, px.ctypes.data))
        return col, px

    def counters(self):
        out = (C.c_uint64 * 4)()
        check(lib().spt_multi_counters(self.handle, out))
        return list(out)

    def band_buffers(self, k):
        """(device, d_colors, d_seeds, d_pixels, stream) of band k."""
        dev = C.c_int()
        p = [C.c_void_p() for _ in range(4)]
        check(lib().spt_multi_band_buffers(self.handle, k, C.byref(dev), *[C.byref(x) for x in p]))
        return (dev.value,) + tuple(x.value for x in p)

    def close(self):
        if self.handle:
            lib().spt_multi_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
