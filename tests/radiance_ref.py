"""The reference's radiance along one ray, from the oracle as it is, and the
rays the radiance tests and tools/radiance_query_time.py send.  A plain helper
module.

oracle/ exposes no per-ray radiance.  ors_render on a 1 x 1 frame with a
degenerate camera is exactly one ray: with cam.x = cam.y = 0, cam.dir = D and
cam.orig = O it takes its two jitter draws, whose values then multiply zeros,
and traces o = 0.1f * D + O, d = vnorm(D) -- with first_sample = k and
nsamples = 1 that is sample k of RadiancePathTracing (or
RadianceDirectLighting) along (o, d) folded into the running average, the
oracle's own code throughout.  So a test ray is a pair (D, O): the oracle gets
the pair and the RNG state *before* the two draws; the device gets the float32
(o, d) computed by the same formula (launch_rays) and the state *after* them
(after_jitter).  A jittered camera ray is the pair (rdir, cam.orig) of the
real camera's unnormalised direction: the renderer's own primary ray.

tests/test_radiance_ref.py pins this harness against whole-frame ors_render."""
import ctypes as C

import numpy as np

import oracle_lib
import rtamd
import scenes_layouts as sl

f32 = np.float32


def launch_rays(D, O):
    """float32 [n, 6] rows (o.xyz, d.xyz) of the rays the oracle traces for
    the pairs (D, O): ors_render's own statements for a 1 x 1 frame whose
    camera has x = y = 0 -- the jitter terms included, so that a zero
    component keeps the sign it gets there -- one float32 operation per numpy
    call.  (kcx, kcy are finite whatever was drawn; any value gives the same
    products, so 0 stands for the draws.)"""
    D, O = np.ascontiguousarray(D, dtype=f32), np.ascontiguousarray(O, dtype=f32)
    kc = (f32(0.0) + f32(0.0)) * f32(1.0) - f32(0.5)
    out = np.empty((len(D), 6), dtype=f32)
    rdir = [f32(0.0) * kc + f32(0.0) * kc + D[:, a] for a in range(3)]
    for a in range(3):
        out[:, a] = f32(0.1) * rdir[a] + O[:, a]
    dot = rdir[0] * rdir[0] + rdir[1] * rdir[1] + rdir[2] * rdir[2]
    with np.errstate(all="ignore"):
        l = f32(1.0) / np.sqrt(dot)                             # vnorm (vec.h:50)
        for a in range(3):
            out[:, 3 + a] = l * rdir[a]
    return out


def after_jitter(seeds):
    """uint32 [n, 2] states after the camera's two draws, and the draws' values
    minus .5f (smallptCPU.cpp:89-90's r1, r2)."""
    seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
    v1, s0, s1 = rtamd.scenes.mwc_draw(seeds[:, 0], seeds[:, 1])
    v2, s0, s1 = rtamd.scenes.mwc_draw(s0, s1)
    return np.stack([s0, s1], axis=1), v1 - f32(0.5), v2 - f32(0.5)


def oracle_sample(S, n, D, O, seeds, col, k, dl=0):
    """Sample number k along every pair (D[r], O[r]) by one 1 x 1 ors_render
    call each: seeds (uint32 [nr, 2], the states before the jitter draws) and
    col (float32 [nr, 3], the running averages) are left alone; returns (col,
    seeds, counters) after the sample, counters uint64 [nr, 4] = Intersect
    calls, IntersectP calls, sphere tests, samples of each ray."""
    L = oracle_lib.lib()
    D, O = np.ascontiguousarray(D, dtype=f32), np.ascontiguousarray(O, dtype=f32)
    col = np.array(col, dtype=f32, order="C")
    seeds = np.array(seeds, dtype=np.uint32, order="C")
    nr = len(D)
    assert col.shape == (nr, 3) and seeds.shape == (nr, 2) and O.shape == D.shape == (nr, 3)
    cnt = np.zeros((nr, 4), np.uint64)
    cam = oracle_lib.Camera()                                   # x = y = 0
    px = np.zeros(1, np.uint32)
    one = (C.c_uint64 * 4)()
    sph = C.addressof(S)
    for r in range(nr):
        cam.dir = oracle_lib.V3(float(D[r, 0]), float(D[r, 1]), float(D[r, 2]))
        cam.orig = oracle_lib.V3(float(O[r, 0]), float(O[r, 1]), float(O[r, 2]))
        L.ors_render(sph, n, C.addressof(cam), col[r:r + 1].ctypes.data, seeds[r:r + 1].ctypes.data, px.ctypes.data,
                     1, 1, 0, 1, k, 1, dl, one, 1)
        cnt[r] = one[:]
    return col, seeds, cnt


# ---- rays, as pairs (D, O)
def camera_pairs(cam, w, h, r1=None, r2=None, x=None, y=None):
    """The pairs of the real camera's rays (rtamd.scenes.camera_rays' pixels
    and jitter): D the unnormalised direction (smallptCPU.cpp:95-97), O the
    camera's origin."""
    inv_w, inv_h = f32(1.0) / f32(w), f32(1.0) / f32(h)
    if x is None:
        x, y = np.tile(np.arange(w), h), np.repeat(np.arange(h), w)
    x, y = np.asarray(x).astype(f32), np.asarray(y).astype(f32)
    r1 = f32(0.0) if r1 is None else np.asarray(r1, dtype=f32)
    r2 = f32(0.0) if r2 is None else np.asarray(r2, dtype=f32)
    kcx = (x + r1) * inv_w - f32(0.5)
    kcy = (y + r2) * inv_h - f32(0.5)
    D = np.stack([f32(getattr(cam.x, a)) * kcx + f32(getattr(cam.y, a)) * kcy + f32(getattr(cam.dir, a))
                  for a in "xyz"], axis=1).astype(f32)
    O = np.broadcast_to(np.array([cam.orig.x, cam.orig.y, cam.orig.z], f32), D.shape).copy()
    return D, O


CORNELL_ROOM = ((1.0, 0.0, 0.0), (99.0, 81.6, 170.0))          # inside scene.h's walls


def aimed_pairs(S, n, count, seed=1, inside=None, box=None):
    """`count` pairs aimed at sphere centres (a little off them) from random
    origins in `box` = (lo, hi) (default: the box of the scene's ordinary
    spheres), D of random length in [0.5, 2).  inside=i: the origins lie
    inside sphere i instead and the directions are uniform."""
    rows = sl.rows_of(S, n)
    p, rad = rows[:, 1:4].astype(np.float64), rows[:, 0].astype(np.float64)
    rng = np.random.default_rng([seed, n, 300])
    small = np.flatnonzero(rad < 100 * np.median(rad))
    lo = (p[small] - rad[small, None]).min(axis=0)
    hi = (p[small] + rad[small, None]).max(axis=0)
    if box is not None:
        lo, hi = np.asarray(box[0], np.float64), np.asarray(box[1], np.float64)
    if inside is None:
        o = rng.uniform(lo, hi, (count, 3))
        si = small[rng.integers(0, len(small), count)]
        v = p[si] + 0.5 * rad[si, None] * rng.normal(0, 1, (count, 3)) - o
    else:
        u = rng.normal(0, 1, (count, 3))
        o = p[inside] + 0.9 * rad[inside] * rng.random((count, 1)) ** (1 / 3) * u / np.linalg.norm(u, axis=1, keepdims=True)
        v = rng.normal(0, 1, (count, 3))
    v = v / np.linalg.norm(v, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, (count, 1))
    D = v.astype(f32)
    # O such that the traced origin 0.1f * D + O is (about) o
    return D, (o - 0.1 * v).astype(f32)


def seeds_for(count, seed=1):
    """uint32 [count, 2] states as AllocateBuffers makes them (>= 2)."""
    return rtamd.scenes.seeds(count, 1, seed).reshape(count, 2)


def reference(S, n, cam_of, grid, count, dl, samples=2, box=None, inside=None, ninside=0, seed=1):
    """The ray mix of the GPU tests and what the oracle returns for it over
    `samples` successive single-sample calls: grid = (w, h) jittered camera
    rays of cam_of(w, h) (the jitter drawn anew for every sample, from the
    state the previous one left), ninside rays started inside sphere `inside`,
    the rest aimed at sphere centres.  A list, one dict per sample: "rays"
    float32 [count, 6] and "seeds_in" uint32 [count, 2] for the device (the
    state after the jitter draws), "col", "seeds_out" and "cnt" as
    oracle_sample returns them, "pairs" = (D, O) and "seeds_before" as it
    was given them."""
    w, h = grid
    ncam = w * h
    cam = cam_of(w, h)
    parts = [aimed_pairs(S, n, count - ncam - ninside, seed, box=box)]
    if ninside:
        parts.append(aimed_pairs(S, n, ninside, seed + 1, inside=inside))
    s = seeds_for(count, seed)
    col = np.zeros((count, 3), f32)
    out = []
    for k in range(samples):
        after, r1, r2 = after_jitter(s)
        cp = camera_pairs(cam, w, h, r1[:ncam], r2[:ncam])
        D = np.concatenate([cp[0]] + [p[0] for p in parts])
        O = np.concatenate([cp[1]] + [p[1] for p in parts])
        before = s
        col, s, cnt = oracle_sample(S, n, D, O, s, col, k, dl)
        out.append({"rays": launch_rays(D, O), "seeds_in": after, "col": col.copy(), "seeds_out": s.copy(), "cnt": cnt,
                    "pairs": (D, O), "seeds_before": before.copy()})
    return out
