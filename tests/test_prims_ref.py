"""CPU pin of tests/prims_ref.py (the reference of tests/test_gpu_prims.py):
on the two reference scenes, opened (three walls dropped, so rays miss) and
with reflection and refraction off (so only camera rays are traced), its
nearest hits and first occluders over the frame's camera rays must add up to
the frame oracle's work counters: traced rays, misses, shadow rays (one per
light per ray that hit a non-light) and intersection tests (n per traced ray,
position + 1 or every non-light per shadow ray)."""
import numpy as np
import pytest

import oracle_lib as O
import prims_ref as R

F = np.float32
W = 48


def camera_rays(w, h, rows, accumulate):
    """The nine sub-sample rays of every pixel of `rows` (raytracer.cpp:278-367,
    raytracer_non_OpenCL.c:304-331), in float32.  accumulate: Whitted's SX / SY
    recurrences; else the queue tracer's WX1 + x * DX."""
    DX, DY = (F(3) - F(-3)) / F(w), (F(-2.25) - F(2.25)) / F(h)
    if accumulate:
        SX = np.empty(w, F)
        sx = F(-3)
        for x in range(w):
            SX[x] = sx
            sx = F(sx + DX)
        SY = np.empty(h, F)
        sy = F(F(2.25) + F(20) * DY)
        for y in range(20, h):
            SY[y] = sy
            sy = F(sy + DY)
    else:
        SX = F(-3) + np.arange(w).astype(F) * DX
        SY = F(2.25) + np.arange(h).astype(F) * DY
    rays = []
    for y in rows:
        for x in range(w):
            for tx in (-1, 0, 1):
                for ty in (-1, 0, 1):
                    d = np.array([F(SX[x] + DX * F(tx / 2.0)) - F(0), F(SY[y] + DY * F(ty / 2.0)) - F(0.25), F(7)], F)
                    inv = F(1) / np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
                    rays.append([F(0), F(0.25), F(-7)] + list(d * inv))
    return np.array(rays, F)


def shadow_ray(ray, dist, centre):
    """The shadow ray of raytracer.cpp:61-82 / raytracer_non_OpenCL.c:201-222
    from a hit to a light centre, and its length, in float32."""
    o, d = ray[:3], ray[3:]
    pi = d * F(dist) + o
    L = np.asarray(centre, F) - pi
    length = np.sqrt(F(F(L[0] * L[0] + L[1] * L[1]) + L[2] * L[2]))
    L = L * (F(1) / length)
    return np.concatenate([pi + L * F(0.001), L]).astype(F), length


def opened(prims, n, drop, flat):
    """The scene without the walls `drop` and with refl = refr = 0."""
    keep = [i for i in range(n) if i not in drop]
    Q = (type(prims[0]) * 64)()
    for k, i in enumerate(keep):
        Q[k] = prims[i]
        flat(Q[k])
    return Q, len(keep)


def check(traits, scene, rays, counters, centres, misses):
    dist, prim, result = R.nearest(scene, rays, traits)
    miss = R.TRAITS[traits][2]
    hit = prim != miss
    lit = np.zeros(len(rays), bool)
    lit[hit] = scene.light[prim[hit]]
    shaded = hit & ~lit
    assert hit.any() and (~hit).any() and lit.any() and shaded.any()
    assert counters[0] == len(rays)
    if misses is not None:
        assert misses == int((~hit).sum())
    assert counters[1] == len(centres) * int(shaded.sum())
    srays, lens = [], []
    for i in np.flatnonzero(shaded):
        for c in centres:
            r, length = shadow_ray(rays[i], dist[i], c)
            srays.append(r)
            lens.append(length)
    first = R.first_occluder(scene, np.array(srays, F), np.array(lens, F), traits)
    tests = np.where(first == R.NONE, int(scene.occluder.sum()), first + 1)
    assert (first != R.NONE).any() and (first == R.NONE).any()
    assert counters[2] == len(rays) * scene.n + int(tests.sum())


def test_whitted_counters():
    P, n = O.whitted_scene()

    def flat(p):
        p.m_Refl = p.m_Refr = 0.0
    Q, m = opened(P, n, (0, 9, 12), flat)           # no floor, left or back wall
    w, h, rows = 96, 240, range(156, 170)     # the rows of the low light (primitive 16)
    _, cnt = O.whitted_render(w, h, rows[0], rows[-1] + 1, prims=Q, n=m)
    scene = R.Scene([R.sphere((q.m_Centre.x, q.m_Centre.y, q.m_Centre.z), q.m_SqRadius, light=q.m_Light > 0)
                     if q.type == 1 else R.plane((q.plane_N.x, q.plane_N.y, q.plane_N.z), q.plane_D)
                     for q in (Q[i] for i in range(m))])
    centres = [(Q[i].m_Centre.x, Q[i].m_Centre.y, Q[i].m_Centre.z) for i in range(m) if Q[i].m_Light > 0]
    check("whitted", scene, camera_rays(w, h, rows, True), cnt, centres, None)


def test_queue_counters():
    P, n = O.queue_scene()

    def flat(p):
        p.m_refl = p.m_refr = 0.0
    Q, m = opened(P, n, (10, 11, 12), flat)
    h = 12
    _, cnt = O.queue_render(W, h, Q, m)
    scene = R.Scene([R.sphere((q.center.x, q.center.y, q.center.z), q.sq_radius, light=bool(q.is_light))
                     if q.type == 1 else R.plane((q.normal.x, q.normal.y, q.normal.z), q.depth)
                     for q in (Q[i] for i in range(m))])
    centres = [(Q[i].center.x, Q[i].center.y, Q[i].center.z) for i in range(m) if Q[i].is_light]
    # counters[3]: with refl = refr = 0 everywhere, exactly the rays that hit nothing
    check("queue", scene, camera_rays(W, h, range(h), False), cnt, centres, cnt[3])


@pytest.mark.parametrize("traits", ["whitted", "queue"])
def test_loop_conventions(traits):
    """Miss values, the strict '<' against far and against the running
    distance (the lowest index wins a tie), INPRIM's result, and the occluder
    position counted over non-lights only."""
    far, result0, miss = R.TRAITS[traits]
    s = R.Scene([R.sphere((0, 0, 50), 1.0, light=True), R.plane((0, 0, -1), 8.0), R.sphere((0, 0, 10), 4.0),
                 R.plane((0, 0, -1), 8.0), R.sphere((0, 0, 0), 9.0)])
    rays = np.array([[0, 0, 0, 0, 0, 1], [0, 0, 0, 1, 0, 0], [0, 0, 20, 0, 0, 1], [0, 5, 0, 0, 1, 0]], F)
    dist, prim, result = R.nearest(s, rays, traits)
    # along z from the origin: inside sphere 4 (exit at 3); the planes and sphere 2 at 8 come later
    assert (dist[0], prim[0], result[0]) == (3.0, 4, -1)
    assert (dist[1], prim[1], result[1]) == (3.0, 4, -1)
    assert (dist[2], prim[2], result[2]) == (29.0, 0, 1)
    assert (dist[3], prim[3], result[3]) == (far, miss, result0)
    s2 = R.Scene([R.sphere((0, 0, 50), 1.0, light=True), R.plane((0, 0, -1), 8.0), R.sphere((0, 0, 10), 4.0),
                  R.plane((0, 0, -1), 8.0)])
    d2, p2, r2 = R.nearest(s2, rays[:1], traits)
    assert (d2[0], p2[0], r2[0]) == (8.0, 1, 1)
    first = R.first_occluder(s2, rays[[0, 0, 0, 3]], np.array([8.0, np.nextafter(F(8), F(9)), np.inf, np.inf], F),
                             traits)
    assert first.tolist() == [R.NONE, 0, 0, R.NONE]
    length, inv = R.light_len_inv(np.array([4.0, 0.0, np.inf], F))
    assert length.tolist() == [2.0, 0.0, np.inf] and inv.tolist() == [0.5, np.inf, 0.0]
