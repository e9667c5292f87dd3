"""Explicit tile-group lists (spt_scene_render_list_async, the cost-balanced
multi-GPU split of configs[4]), the group pack / unpack of their exchange,
and the rays-only counter mode (SPT_COUNT_RAYS).

Every pixel is independent (own RNG words, own accumulator: smallptCPU.cpp:
84-123), so any partition of the frame's tile groups rendered list by list
must give the full-frame render's bits -- which the other GPU tests pin to
the reference (oracle, reference-core goldens)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _open(rt, kind, w, h):
    """A prepared scene and a function that makes a zeroed device frame of it."""
    S, n, cam = rt.scenes.smallpt(kind, w, h)
    sc = rt.SmallptScene(S, n)
    return sc, lambda: rt.SmallptDeviceFrame(sc, cam, w, h)


@pytest.mark.parametrize("kind,w,h,spp,env", [
    ("cornell", 200, 120, 3, {}),
    ("cornell", 197, 61, 2, {}),                          # ragged: groups straddle tile rows
    ("complex", 320, 180, 2, {}),                         # 8-wide hierarchy (persistent waves)
    ("complex", 320, 180, 2, {"RT_SPT_WIDE": "0"}),       # binary hierarchy (staged group stores)
    ("complex", 250, 130, 2, {"RT_SPT_WIDE": "0"}),
])
def test_lists_partition_the_frame(rt, monkeypatch, kind, w, h, spp, env):
    """A random partition of the frame's tile groups into 3 lists (random
    order within each), rendered list by list into one frame == one
    full-frame render: colours, seeds, pixels bit for bit, counters summed
    (full and rays-only).  Entries outside [0, groups) are skipped."""
    import torch
    from rtamd import dist as rd
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    sc, frame = _open(rt, kind, w, h)
    ref, got = frame(), frame()
    ng = ref.groups_total
    assert ng == rd.group_count(w, h)
    ref.render(spp, counted=True)
    rng = np.random.default_rng(w + h)
    perm = rng.permutation(ng)
    cuts = sorted(rng.choice(np.arange(1, ng), 2, replace=False))
    lists = [perm[:cuts[0]], perm[cuts[0]:cuts[1]], perm[cuts[1]:]]
    for mode in (0, rt.SPT_COUNT_RAYS, rt.SPT_LIST_SET):
        got.reset()
        got.counters[2] = 12345                            # rays-only leaves counters[2] untouched
        for i, lst in enumerate(lists):
            # out-of-range entries: skipped (SPT_LIST_SET: the caller promises none, and no dedup pass runs)
            lst = list(lst) + ([-7, ng, 1 << 30] if i == 1 and mode != rt.SPT_LIST_SET else [])
            got.render(spp, mode=mode, counted=True, groups=torch.tensor(lst, dtype=torch.int32, device=got.device))
        torch.cuda.synchronize()
        assert got.same_bits(ref), mode
        c, r = got.counters.tolist(), ref.counters.tolist()
        if mode == rt.SPT_COUNT_RAYS:
            assert (c[0], c[1], c[3]) == (r[0], r[1], r[3]) and c[2] == 12345, (c, r)
        else:
            assert c == [r[0], r[1], r[2] + 12345, r[3]], (c, r)


def test_list_costs_and_bad_arguments(rt):
    """d_group_cost gets a positive wave time for every listed group of a
    hierarchy scene and nothing for the others; a list longer than the
    frame's group count is refused."""
    import torch
    w, h = 320, 180
    sc, frame = _open(rt, "complex", w, h)
    f = frame()
    dev, ng = f.device, f.groups_total
    lst = list(range(0, ng, 3))
    d = torch.tensor(lst, dtype=torch.int32, device=dev)
    cost = torch.zeros(ng, dtype=torch.int32, device=dev)
    for cbuf in (None, cost):                 # (a warm-up launch first: the timed ones compare)
        f.render(2, groups=d, cost=cbuf)
    torch.cuda.synchronize()
    c = cost.cpu().numpy()
    mask = np.zeros(ng, bool)
    mask[lst] = True
    assert (c[mask] > 0).all() and (c[~mask] == 0).all()
    # SPT_COST_MAX: each listed group's longest tile instead of the sum of its
    # (up to four) tiles -- over all groups well below the sums and above a
    # quarter of them (two launches' wave times, so only in aggregate); the
    # same frame
    cmax = torch.zeros(ng, dtype=torch.int32, device=dev)
    f2 = frame()
    f2.render(2, mode=rt.SPT_COST_MAX, groups=d, cost=cmax)
    torch.cuda.synchronize()
    m = cmax.cpu().numpy().astype(np.int64)
    assert (m[mask] > 0).all() and (m[~mask] == 0).all()
    ratio = m[mask].sum() / c[mask].sum()
    assert 0.15 < ratio < 0.9, ratio
    assert torch.equal(f2.colors.view(torch.int32), f.colors.view(torch.int32)) and torch.equal(f2.pixels, f.pixels)
    # Full counters (the refilling kernel: a lane's unit is a pixel): the sum
    # of each group's pixel durations, or with SPT_COST_MAX the longest one --
    # which no launch can exceed (100 MHz ticks against the launch's own
    # duration), while a sum over a group's pixels far exceeds its max.
    csum = torch.zeros(ng, dtype=torch.int32, device=dev)
    cmx = torch.zeros(ng, dtype=torch.int32, device=dev)
    cnt = torch.zeros(4, dtype=torch.int64, device=dev)
    for mode, cb in ((0, csum), (rt.SPT_COST_MAX, cmx)):
        f3 = frame()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        f3.render(2, mode=mode, counted=cnt, groups=d, cost=cb)
        e1.record()
        torch.cuda.synchronize()
        assert torch.equal(f3.colors.view(torch.int32), f.colors.view(torch.int32))
        assert torch.equal(f3.pixels, f.pixels)
    launch_ticks = e0.elapsed_time(e1) * 1e5
    s, mx = csum.cpu().numpy().astype(np.int64), cmx.cpu().numpy().astype(np.int64)
    assert (mx[mask] > 0).all() and (mx[~mask] == 0).all() and (s[mask] > 0).all()
    assert mx.max() <= 1.05 * launch_ticks + 1000, (mx.max(), launch_ticks)
    assert mx[mask].sum() < 0.5 * s[mask].sum(), (mx[mask].sum(), s[mask].sum())
    assert f2.render(1, mode=0x400, groups=d, check=False) == rt._lib.RT_ERR_INVALID
    big = torch.zeros(ng + 1, dtype=torch.int32, device=dev)
    assert f.render(1, groups=big, ngroups=ng + 1, check=False) == rt._lib.RT_ERR_INVALID


@pytest.mark.parametrize("kind", ["cornell", "complex"])
def test_list_repeated_entries_render_once(rt, kind):
    """A list naming groups more than once (and out-of-range entries) is
    taken as a set: the frame equals the same groups listed once (a group
    rendered twice with first_sample > 0 would fold its samples into the
    accumulator twice), so do the counters, and each group's wave time is
    added to its cost entry once (a repeat would roughly double it).  The
    whole frame as a list equals the full-frame render."""
    import torch
    w, h = 160, 96
    sc, new_frame = _open(rt, kind, w, h)
    dev = torch.device("cuda", 0)
    ng = rt.lib().spt_group_count(w, h)

    def frame(lst, cost=None):
        f = new_frame()
        d = None if lst is None else torch.tensor(lst, dtype=torch.int32, device=dev)
        f.render(2, counted=True, groups=d)
        f.render(2, first_sample=2, counted=True, groups=d, cost=cost, seeds_in=f.seeds)
        torch.cuda.synchronize()
        return f

    ref = frame(None)
    rng = np.random.default_rng(5)
    base = [int(g) for g in rng.permutation(ng)]
    assert frame(base).same_bits(ref)
    cover = base[: ng // 2]                        # half the frame, then repeats (a list is <= ng long)
    lst = cover + [int(g) for g in rng.choice(cover, ng // 4)] + [-1, ng]
    rng.shuffle(lst)
    c1 = torch.zeros(ng, dtype=torch.int32, device=dev)
    c2 = torch.zeros(ng, dtype=torch.int32, device=dev)
    once = frame(cover, c1)
    got = frame(lst, c2)
    assert got.same_bits(once) and got.counters.tolist() == once.counters.tolist()
    if kind == "complex":                     # costs are recorded by the hierarchy kernels
        a, b = c1.cpu().numpy().astype(np.float64)[cover], c2.cpu().numpy().astype(np.float64)[cover]
        assert (a > 0).all() and (b > 0).all()
        assert np.median(b / a) < 1.5, np.median(b / a)


@pytest.mark.parametrize("w,h", [(1920, 1080), (197, 61), (33, 9)])
def test_groups_pack_unpack(rt, w, h):
    """spt_groups_pack_async == the host-side slot map (rtamd.dist.group_slots)
    with 0 for pixels outside the frame; unpacking into a cleared frame
    restores exactly the listed groups' slots and nothing else."""
    import torch
    from rtamd import dist as rd
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream(dev).cuda_stream
    L = rt.lib()
    ng = rd.group_count(w, h)
    rng = np.random.default_rng(w)
    col = torch.from_numpy(rng.standard_normal(3 * w * h).astype(np.float32)).to(dev)
    lst = rng.permutation(ng)[: max(1, ng // 3)]
    d = torch.tensor(lst, dtype=torch.int32, device=dev)
    buf = torch.full((len(lst) * 768,), 7.0, dtype=torch.float32, device=dev)
    rt.check(L.spt_groups_pack_async(col.data_ptr(), w, h, d.data_ptr(), len(lst), buf.data_ptr(), st))
    torch.cuda.synchronize()
    slots = rd.group_slots(lst, w, h)                                    # [n, 256]
    c3 = col.cpu().numpy().reshape(-1, 3)
    want = np.where((slots >= 0)[..., None], c3[np.maximum(slots, 0)], 0).astype(np.float32)
    assert (buf.cpu().numpy().view(np.uint32) == want.reshape(-1).view(np.uint32)).all()
    out = torch.zeros_like(col)
    rt.check(L.spt_groups_unpack_async(out.data_ptr(), w, h, d.data_ptr(), len(lst), buf.data_ptr(), st))
    torch.cuda.synchronize()
    o3 = out.cpu().numpy().reshape(-1, 3)
    m = np.zeros(w * h, bool)
    m[slots[slots >= 0]] = True
    assert (o3[m].view(np.uint32) == c3[m].view(np.uint32)).all() and (o3[~m] == 0).all()


@pytest.mark.parametrize("kind,env", [("cornell", {}), ("complex", {}), ("complex", {"RT_SPT_WIDE": "0"})])
def test_count_rays_mode(rt, monkeypatch, kind, env):
    """SPT_COUNT_RAYS: the same frame, and Intersect / IntersectP calls and
    samples equal to the full counters (SURVEY §8(d)'s ray count), with the
    uncounted queries; counters[2] is left as it was."""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w, h = 240, 136
    sc, frame = _open(rt, kind, w, h)
    fr = []
    for mode in (0, rt.SPT_COUNT_RAYS, rt.SPT_COUNT_RAYS | rt.SPT_DIRECT_LIGHTING, rt.SPT_DIRECT_LIGHTING):
        f = frame()
        f.counters[2] = -1
        f.render(3, mode=mode, counted=True)
        torch.cuda.synchronize()
        fr.append(f)
    for a, b in ((fr[0], fr[1]), (fr[3], fr[2])):
        assert a.same_bits(b)
        ca, cb = a.counters.tolist(), b.counters.tolist()
        assert (ca[0], ca[1], ca[3]) == (cb[0], cb[1], cb[3]) and cb[2] == -1 and ca[2] > 0, (ca, cb)
    assert fr[0].render(1, mode=0x400, check=False) == rt._lib.RT_ERR_INVALID      # (0x200 is SPT_COST_MAX)
