"""SmallptDeviceFrame: one prepared smallpt scene plus device-resident frame
buffers, launched asynchronously -- the path the GPU tests and the tools
drive.  This module is the one place in the package that spells out the calls
to spt_scene_render_async, spt_scene_render_groups_async,
spt_scene_render_list_async, spt_scene_render_pixels_async,
spt_scene_render_pixels_stats_async and spt_frame_plan_async
(include/rt_hip.h).

torch is imported inside the functions, so `import rtamd` works without it.
"""
import ctypes as C

import numpy as np

from . import scenes
from ._lib import SPT_PATH_TRACING, PlanParams, check as _check, entry, lib


def _i32(v):
    """A 32-bit pattern given signed or unsigned, as the int32 torch fills with."""
    return (int(v) + (1 << 31)) % (1 << 32) - (1 << 31)


class SmallptDeviceFrame:
    """colors / seeds / pixels / counters of one w x h frame on `device`, and
    the launches of `scene` (a SmallptScene, borrowed: the caller closes it)
    into them.  seeds0 holds the initial seeds and is never written.  Where
    `device` is not the current HIP device the caller selects it
    (rtamd.set_device) around scene creation and launches, as without the
    class."""

    def __init__(self, scene, camera, w, h, seed=1, device=0):
        import torch
        self.scene, self.camera, self.w, self.h = scene, camera, w, h
        self.device = torch.device("cuda", device)
        self.seeds0 = torch.from_numpy(scenes.seeds(w, h, seed).view(np.int32)).to(self.device)
        self.seeds = torch.zeros_like(self.seeds0)
        self.colors = torch.zeros(3 * w * h, dtype=torch.float32, device=self.device)
        self.pixels = torch.zeros(w * h, dtype=torch.int32, device=self.device)
        self.counters = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._done = None
        self._m2 = None
        self._plan = {}                     # cap -> (pixels, take): frame.plan()'s lists
        self._plan_scratch = None
        self._plan_totals = None
        self._error = None

    @property
    def m2(self):
        """The running mean of the samples' |R|^2 per pixel, float32 [w * h]
        in slot order like `done` (render_pixels(stats=True) keeps it beside
        the colour); made, zeroed, at its first use."""
        if self._m2 is None:
            import torch
            self._m2 = torch.zeros(self.w * self.h, dtype=torch.float32, device=self.device)
        return self._m2

    @property
    def plan_totals(self):
        """int64 [2] on the device: the pixels the last plan() listed (before
        truncation at its cap) and the sum of their takes."""
        if self._plan_totals is None:
            import torch
            self._plan_totals = torch.zeros(2, dtype=torch.int64, device=self.device)
        return self._plan_totals

    @property
    def error(self):
        """float32 [w * h] in slot order: every pixel's relative standard
        error as the last plan(error=True) saw it (+inf below min_samples)."""
        if self._error is None:
            import torch
            self._error = torch.zeros(self.w * self.h, dtype=torch.float32, device=self.device)
        return self._error

    @property
    def done(self):
        """The samples every pixel has had (its currentSample), int32 [w * h]
        in slot order (h - y - 1) * w + x like `colors`; made, zeroed, at its
        first use (render_pixels(use_done=True))."""
        if self._done is None:
            import torch
            self._done = torch.zeros(self.w * self.h, dtype=torch.int32, device=self.device)
        return self._done

    @property
    def groups_total(self):
        """spt_group_count(w, h): the frame's tile groups."""
        return entry("spt_group_count")(self.w, self.h)

    def render(self, nsamples, *, first_sample=0, mode=SPT_PATH_TRACING, counted=False, rows=None, share=None,
               groups=None, ngroups=None, cost=None, seeds_in=None, stream=None, check=True):
        """One asynchronous launch of samples [first_sample, first_sample +
        nsamples) into the frame; returns the entry point's code (raises
        RTError on failure unless check=False).  The window is at most one of
        rows=(r0, r1) (spt_scene_render_async; the default, (0, h)),
        share=(k, N) (spt_scene_render_groups_async) and groups=<int32 device
        tensor> (spt_scene_render_list_async; ngroups overrides its length,
        cost is its optional int32 d_group_cost).  counted: False (no counter
        buffer), True (self.counters) or an int64 tensor of the caller's.
        seeds_in defaults to seeds0; a progressive caller passes self.seeds.
        stream (a torch stream or a raw handle) defaults to torch's current
        stream on the frame's device at the time of the call.  Allocates
        nothing on the device and never synchronises."""
        if sum(x is not None for x in (rows, share, groups)) > 1:
            raise ValueError("render: at most one of rows=, share= and groups=")
        if groups is None and (ngroups is not None or cost is not None):
            raise ValueError("render: ngroups= and cost= go with groups=")
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(self.device)
        L = lib()
        # the locals below carry the header's parameter names, in its order
        scene = self.scene.handle
        camera = C.byref(self.camera)
        d_colors = self.colors.data_ptr()
        d_seeds_in = (self.seeds0 if seeds_in is None else seeds_in).data_ptr()
        d_seeds_out = self.seeds.data_ptr()
        d_pixels = self.pixels.data_ptr()
        w, h = self.w, self.h
        d_counters = None if counted is False else (self.counters if counted is True else counted).data_ptr()
        stream = getattr(stream, "cuda_stream", stream)
        if share is not None:
            group, ngroups = share
            # (scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, group, ngroups, first_sample,
            #  nsamples, mode, d_counters, stream)
            entry("spt_scene_render_groups_async")       # (RTError where an older build lacks it)
            rc = L.spt_scene_render_groups_async(
                scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, group, ngroups, first_sample,
                nsamples, mode, d_counters, stream)
        elif groups is not None:
            d_groups = groups.data_ptr()
            ngroups = groups.numel() if ngroups is None else ngroups
            d_group_cost = None if cost is None else cost.data_ptr()
            # (scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, d_groups, ngroups, first_sample,
            #  nsamples, mode, d_counters, d_group_cost, stream)
            entry("spt_scene_render_list_async")
            rc = L.spt_scene_render_list_async(
                scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, d_groups, ngroups, first_sample,
                nsamples, mode, d_counters, d_group_cost, stream)
        else:
            row_begin, row_end = (0, h) if rows is None else rows
            # (scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, row_begin, row_end, first_sample,
            #  nsamples, mode, d_counters, stream)
            rc = L.spt_scene_render_async(
                scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, row_begin, row_end, first_sample,
                nsamples, mode, d_counters, stream)
        return _check(rc) if check else rc

    def render_pixels(self, pixels, take=None, nsamples=0, *, use_done=True, first_sample=0, mode=SPT_PATH_TRACING,
                      seeds_in=None, stream=None, check=True, stats=False):
        """One asynchronous launch (spt_scene_render_pixels_async) that adds
        samples to the listed pixels only: `pixels` is a contiguous int32
        device tensor of indices y * w + x (the index of `self.pixels`; an
        entry outside the frame, -1 say, is skipped; no pixel may repeat),
        `take` a contiguous int32 device tensor of as many sample counts, or
        None: every entry takes `nsamples`.  use_done=True numbers a pixel's
        samples from self.done and adds its take there, so successive calls
        continue every pixel where it stands; use_done=False numbers them from
        first_sample, as render() does.  seeds_in defaults to self.seeds with
        use_done (a progressive loop: start it with
        frame.seeds.copy_(frame.seeds0)), else to seeds0, as for render().
        stats=True (spt_scene_render_pixels_stats_async) also keeps self.m2,
        the running mean of the samples' |R|^2, and changes no other bit.
        Unlisted pixels are not touched in any buffer.  Returns the entry
        point's code (raises RTError on failure unless check=False).
        Allocates nothing on the device (but self.done and self.m2 at their
        first use) and never synchronises."""
        import torch

        def is_list(x):
            return x.is_cuda and x.dtype == torch.int32 and x.dim() == 1 and x.is_contiguous()
        if not is_list(pixels):
            raise ValueError("render_pixels: pixels must be a contiguous int32 device tensor [n]")
        if take is not None and not (is_list(take) and take.numel() == pixels.numel()):
            raise ValueError("render_pixels: take must be a contiguous int32 device tensor as long as pixels")
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        if seeds_in is None:
            seeds_in = self.seeds if use_done else self.seeds0
        # the locals below carry the header's parameter names, in its order
        scene = self.scene.handle
        camera = C.byref(self.camera)
        d_colors = self.colors.data_ptr()
        d_seeds_in = seeds_in.data_ptr()
        d_seeds_out = self.seeds.data_ptr()
        d_pixels = self.pixels.data_ptr()
        w, h = self.w, self.h
        nlist = pixels.numel()
        d_list = pixels.data_ptr() if nlist else self.pixels.data_ptr()   # (an empty tensor has no address to pass)
        d_take = None if take is None else (take.data_ptr() if nlist else self.pixels.data_ptr())
        d_done = self.done.data_ptr() if use_done else None
        stream = getattr(stream, "cuda_stream", stream)
        if stats:
            d_m2 = self.m2.data_ptr()
            rc = entry("spt_scene_render_pixels_stats_async")(
                scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, d_m2, w, h, d_list, d_take, nlist, nsamples,
                d_done, first_sample, mode, stream)
        else:
            rc = entry("spt_scene_render_pixels_async")(
                scene, camera, d_colors, d_seeds_in, d_seeds_out, d_pixels, w, h, d_list, d_take, nlist, nsamples,
                d_done, first_sample, mode, stream)
        return _check(rc) if check else rc

    def plan(self, tol, min_samples, max_samples, step, floor=1e-3, cap=None, error=False, *, stream=None,
             check=True):
        """The next pixel list, built on the device (spt_frame_plan_async)
        from colors, m2 and done: a pixel below min_samples is brought up to
        it; one whose relative standard error sqrt(max(m2 - |c|^2, 0) /
        (done * (|c|^2 + floor))) is above tol takes `step` more, never past
        max_samples.  Returns the frame-owned (pixels, take) int32 tensors of
        length cap (default w * h; made at the first call with that cap and
        reused): the listed pixels in 8 x 8 tile order, then -1 / 0 padding, so
        render_pixels takes them as they are.  Fills self.plan_totals and,
        with error=True, self.error.  Asynchronous on `stream` (default:
        torch's current one); after the buffers' first use it allocates
        nothing and never synchronises, so (plan, render_pixels) pairs may be
        enqueued back to back or captured."""
        import torch
        cap = self.w * self.h if cap is None else int(cap)
        if cap < 0:
            raise ValueError("plan: negative cap")
        if cap not in self._plan:
            self._plan[cap] = (torch.full((cap,), -1, dtype=torch.int32, device=self.device),
                               torch.zeros(cap, dtype=torch.int32, device=self.device))
        if self._plan_scratch is None:
            nbytes = entry("spt_frame_plan_scratch_bytes")(self.w, self.h)
            self._plan_scratch = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=self.device)
        pixels, take = self._plan[cap]
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        stream = getattr(stream, "cuda_stream", stream)
        params = PlanParams(min_samples, max_samples, step, tol, floor)
        # (d_colors, d_m2, d_done, w, h, params, d_list, d_take, cap, d_error, d_totals, d_scratch, stream)
        rc = entry("spt_frame_plan_async")(
            self.colors.data_ptr(), self.m2.data_ptr(), self.done.data_ptr(), self.w, self.h, C.byref(params),
            pixels.data_ptr() if cap else None, take.data_ptr() if cap else None, cap,
            self.error.data_ptr() if error else None, self.plan_totals.data_ptr(), self._plan_scratch.data_ptr(),
            stream)
        if check:
            _check(rc)
        return pixels, take

    def refine(self, passes, *, mode=SPT_PATH_TRACING, stream=None, **params):
        """`passes` x (plan(**params), render_pixels(stats=True,
        use_done=True)) on one stream with no synchronisation in between: the
        closed loop of adaptive sampling.  A pass whose plan lists nothing
        renders nothing; self.plan_totals tells the caller, when it wants to
        know, whether the last plan was empty.  Start a frame with reset() and
        seeds.copy_(seeds0)."""
        for _ in range(passes):
            pixels, take = self.plan(stream=stream, **params)
            self.render_pixels(pixels, take, mode=mode, stream=stream, stats=True)
        return self

    def budget_list(self, budget, order="tile"):
        """(pixels, take) for render_pixels from an h x w integer budget map
        (torch or numpy; budget[y, x] = the samples to add to the pixel
        `self.pixels` holds at y * w + x): the non-zero entries only, in 8 x 8
        tile order (tiles row by row, a tile's pixels row by row), so that
        neighbouring pixels share a wave -- or, order="row", by pixel index,
        64 pixels of one row to a wave: a wave's paths are less alike, its
        share of the frame is spread wider ("Pixel lists": the
        faster order on a 10k-sphere scene).  Two int32 device tensors.
        Waits for the device (it counts the entries)."""
        if order not in ("tile", "row"):
            raise ValueError("budget_list: order is 'tile' or 'row'")
        import torch
        b = torch.as_tensor(np.asarray(budget) if not torch.is_tensor(budget) else budget).to(self.device)
        if tuple(b.shape) != (self.h, self.w) or b.dtype.is_floating_point or b.dtype == torch.bool:
            raise ValueError("budget_list: budget must be an integer map [h, w] = [%d, %d]" % (self.h, self.w))
        if bool((b < 0).any()):
            raise ValueError("budget_list: negative budget")
        y, x = torch.nonzero(b, as_tuple=True)
        tiles_x = (self.w + 7) // 8
        if order == "tile":                                 # (nonzero's own order is the row order)
            key = ((y >> 3) * tiles_x + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7)
            rank = torch.argsort(key)
            y, x = y[rank], x[rank]
        return (y * self.w + x).to(torch.int32).contiguous(), b[y, x].to(torch.int32).contiguous()

    def reset(self, colors=0.0, pixels=0, seeds=0):
        """Refills the output tensors in place (pixels and seeds take a 32-bit
        pattern) and zeroes the counters (and `done` and `m2`, where they exist)."""
        self.colors.fill_(colors)
        self.pixels.fill_(_i32(pixels))
        self.seeds.fill_(_i32(seeds))
        self.counters.zero_()
        if self._done is not None:
            self._done.zero_()
        if self._m2 is not None:
            self._m2.zero_()
        return self

    def host(self):
        """Synchronises the device; (colors float32, seeds uint32, pixels
        uint32) as numpy arrays."""
        import torch
        torch.cuda.synchronize(self.device)
        return (self.colors.cpu().numpy(), self.seeds.cpu().numpy().view(np.uint32),
                self.pixels.cpu().numpy().view(np.uint32))

    def same_bits(self, other):
        """Colours (as bit patterns), seeds and pixels equal another frame's."""
        import torch
        return (torch.equal(self.colors.view(torch.int32), other.colors.view(torch.int32))
                and torch.equal(self.seeds, other.seeds) and torch.equal(self.pixels, other.pixels))
