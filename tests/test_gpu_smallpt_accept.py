"""GPU parity of the integer-key accept tests in smallpt's branch-free sphere
loops (csrc/spt_accept.h; smallpt.hip query_bf, shadow_bf): a sphere's two
roots, the "> EPS" tests and the running bound fold into one unsigned minimum
over order-preserving keys.  Everything is compared bit for bit against the
oracle -- HDR colours, pixels, RNG state and, for counted launches, all four
counters -- on each kernel that runs the loops, and on the inputs where keys
and floats could part: shadow rays whose maxt = len - EPS is <= EPS or
negative (limit key 0: nothing is accepted), and spheres so far away that
their roots overflow or exceed the initial bound 1e20."""
import math

import numpy as np
import pytest

import spt_check

pytestmark = pytest.mark.gpu

DIFF, SPEC, REFR = 0, 1, 2
f32 = np.float32
EPS = f32(0.01)


@pytest.fixture(scope="module")
def refs(oracle):
    return spt_check.frame_cache(oracle)


def _scene(rt, rows):
    arr = (rt.Sphere * len(rows))()
    for s, r in zip(arr, rows):
        rt.scenes._sphere(s, *r)
    return arr, len(rows)


def _camera(rt, w, h, orig, target, fov_deg=45.0):
    cam = rt.Camera()
    cam.orig = rt.Vec3(*orig)
    cam.target = rt.Vec3(*target)
    rt.scenes.update_camera(cam, w, h, fov_deg)
    return cam


def _render_and_compare(rt, ref, w, h, spp, counted, scene=None, cam=None):
    S, n = scene if scene else (None, None)
    f = rt.SmallptFrame(w, h, spheres=S, nspheres=n, camera=cam) if scene else rt.SmallptFrame(w, h)
    f.render(spp, counters=counted)
    spt_check.assert_same(f, ref, counted=counted)


# ---------------------------------------------------------------- Cornell, the four kernels
TWO_LIGHTS = (3.0, (30.0, 20.0, 90.0), (6.0, 5.0, 4.0), (0.0, 0.0, 0.0), DIFF)


@pytest.mark.parametrize("kernel", ["two_query", "one_query", "one_query_counted", "counted", "global",
                                    "global_counted"])
def test_cornell_on_each_kernel(rt, refs, monkeypatch, kernel):
    """64x48, 4 spp: the uncounted two-query kernel (query_bf and the ring's
    shadow_bf), the one-query kernel (a second light forces it; its shadow
    queries enter query_bf with the bound len - EPS), the counted kernel
    (query_bf keeps IntersectP's first index) and the global-memory kernel."""
    w, h, spp = 64, 48, 4
    counted = kernel.endswith("counted")
    if kernel.startswith("global"):
        monkeypatch.setenv("RT_SPT_GEO", "global")
    if kernel.startswith("one_query"):
        rows = list(rt.scenes._CORNELL) + [TWO_LIGHTS]
        make = lambda: (_scene(rt, rows), None)                           # noqa: E731
        ref = refs(w, h, [spp], name="cornell+light", make=make)
        _render_and_compare(rt, ref, w, h, spp, counted, scene=_scene(rt, rows))
    else:
        _render_and_compare(rt, refs(w, h, [spp]), w, h, spp, counted)


# ---------------------------------------------------------------- contact: maxt <= EPS
# A 0.004-radius emitter centred on the surface of a unit DIFF sphere, seen
# from 0.1 above it (the camera rays start 0.1 * |rdir| in front of the
# camera's origin), through a 15-degree view so that the emitter's
# surroundings fill the frame.  Light samples land within 2 * EPS of the hit
# points around the emitter, so len - EPS is <= EPS or negative there: the
# replay below counts 199 such rays among the 367 traced at the first vertex,
# 35 of them with a negative maxt (204 of 1082 and 39 with the second light).
CONTACT_W, CONTACT_H, CONTACT_SPP, CONTACT_FOV = 16, 16, 8, 15.0
CONTACT_ROWS = [(1.0, (0.0, 0.0, 0.0), (0, 0, 0), (.75, .75, .75), DIFF),
                (0.004, (0.0, 0.0, 1.0), (40.0, 40.0, 40.0), (0, 0, 0), DIFF)]
CONTACT_FAR_LIGHT = (2.0, (3.0, 4.0, 6.0), (5.0, 5.0, 5.0), (0, 0, 0), DIFF)
CONTACT_ORIG, CONTACT_TARGET = (0.0, 0.0, 1.2), (0.0, 0.0, 0.0)


def _get_random(s):
    """GetRandom (simplernd.h:34-48) on the two-word state s (Python ints)."""
    s[0] = (36969 * (s[0] & 65535) + (s[0] >> 16)) & 0xffffffff
    s[1] = (18000 * (s[1] & 65535) + (s[1] >> 16)) & 0xffffffff
    ires = ((s[0] << 16) + s[1]) & 0xffffffff
    f = np.array([(ires & 0x007fffff) | 0x40000000], np.uint32).view(f32)[0]
    return (f - f32(2)) / f32(2)


def _v(a):
    return np.array([a.x, a.y, a.z], f32)


def _dot(a, b):
    return f32(f32(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])


def _sphere_hit(p, rad, o, d):
    """SphereIntersect (geomfunc.h:32-59) in float32; 0 = miss."""
    op = p - o
    b = _dot(op, d)
    det = f32(f32(b * b - _dot(op, op)) + rad * rad)
    if det < 0:
        return f32(0)
    det = f32(math.sqrt(det))
    t = b - det
    if t > EPS:
        return t
    t = b + det
    return t if t > EPS else f32(0)


def contact_shadow_rays(rows, cam, seeds_per_pass, w, h):
    """Replays, in float32, the first vertex of every sample (camera ray,
    nearest hit, SampleLights' shadow rays, geomfunc.h:112-165) from the RNG
    state the pixel has at the start of each pass.  Returns (shadow rays
    traced, those with maxt = len - EPS <= EPS, those with maxt < 0)."""
    P = [np.array(r[1], f32) for r in rows]
    R = [f32(r[0]) for r in rows]
    lit = [any(v != 0 for v in r[2]) for r in rows]
    cx, cy, cd, co = _v(cam.x), _v(cam.y), _v(cam.dir), _v(cam.orig)
    inv_w, inv_h = f32(1) / f32(w), f32(1) / f32(h)
    traced = contact = negative = 0
    with np.errstate(all="ignore"):
        for seeds in seeds_per_pass:
            for y in range(h):
                for x in range(w):
                    i2 = 2 * ((h - y - 1) * w + x)
                    s = [int(seeds[i2]), int(seeds[i2 + 1])]
                    r1 = _get_random(s) - f32(.5)
                    r2 = _get_random(s) - f32(.5)
                    kcx = (f32(x) + r1) * inv_w - f32(.5)
                    kcy = (f32(y) + r2) * inv_h - f32(.5)
                    rdir = cx * kcx + cy * kcy + cd
                    o = f32(0.1) * rdir + co
                    d = rdir * (f32(1) / f32(math.sqrt(_dot(rdir, rdir))))
                    t, hit_id = f32(1e20), -1
                    for i in range(len(rows) - 1, -1, -1):
                        dist = _sphere_hit(P[i], R[i], o, d)
                        if dist != 0 and dist < t:
                            t, hit_id = dist, i
                    if hit_id < 0 or lit[hit_id] or rows[hit_id][4] != DIFF:
                        continue
                    hp = o + d * t
                    n = hp - P[hit_id]
                    n = n * (f32(1) / f32(math.sqrt(_dot(n, n))))
                    nl = n if _dot(n, d) <= 0 else -n
                    for li in range(len(rows)):
                        if not lit[li]:
                            continue
                        u2 = _get_random(s)                  # the g++ build draws the second argument first
                        u1 = _get_random(s)
                        zz = f32(1) - f32(2) * u1
                        r = f32(math.sqrt(max(f32(0), f32(1) - zz * zz)))
                        phi = f32(2) * f32(math.pi) * u2
                        unit = np.array([f32(float(r) * math.cos(float(phi))), f32(float(r) * math.sin(float(phi))), zz], f32)
                        sp = unit * R[li] + P[li]
                        sd = sp - hp
                        ln = f32(math.sqrt(_dot(sd, sd)))
                        sd = sd * (f32(1) / ln)
                        if _dot(sd, unit) > 0 or not _dot(sd, nl) > 0:
                            continue
                        traced += 1
                        maxt = ln - EPS
                        contact += int(maxt <= EPS)
                        negative += int(maxt < 0)
    return traced, contact, negative


def _contact_reference(rt, oracle, rows):
    """The oracle's frame after CONTACT_SPP single passes, and the seeds each pass started from."""
    w, h = CONTACT_W, CONTACT_H
    S, n = _scene(rt, rows)
    cam = _camera(rt, w, h, CONTACT_ORIG, CONTACT_TARGET, CONTACT_FOV)
    col = np.zeros(3 * w * h, np.float32)
    seeds = oracle.seeds(w, h)
    px = np.zeros(w * h, np.uint32)
    cnt = [0, 0, 0, 0]
    before = []
    for k in range(CONTACT_SPP):
        before.append(seeds.copy())
        c = oracle.smallpt_render(S, n, cam, col, seeds, px, w, h, k, 1)
        cnt = [a + b for a, b in zip(cnt, c)]
    return (S, n), cam, (col, seeds, px, tuple(cnt)), before


@pytest.fixture(scope="module")
def contact(rt, oracle):
    out = {}
    for name, rows in (("one_light", CONTACT_ROWS), ("two_lights", CONTACT_ROWS + [CONTACT_FAR_LIGHT])):
        scene, cam, ref, before = _contact_reference(rt, oracle, rows)
        out[name] = (scene, cam, ref, contact_shadow_rays(rows, cam, before, CONTACT_W, CONTACT_H))
    return out


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("lights", ["one_light", "two_lights"])
def test_contact_shadow_rays_with_maxt_below_eps(rt, contact, lights, counted):
    """one_light: the ring's shadow_bf (uncounted) meets maxt <= EPS;
    two_lights: the one-query kernel's query_bf is entered with t_in <= EPS
    and must return no hit and t_in unchanged.  The replay first shows that
    such rays occur: at least 16, some of them with a negative maxt."""
    scene, cam, ref, (traced, near, negative) = contact[lights]
    print("shadow rays at the first vertex: %d traced, %d with maxt <= EPS, %d with maxt < 0" % (traced, near, negative))
    assert near >= 16 and negative >= 1
    assert traced <= ref[3][1]                # the oracle's IntersectP calls include every first-vertex ray
    _render_and_compare(rt, ref, CONTACT_W, CONTACT_H, CONTACT_SPP, counted, scene=scene, cam=cam)


# ---------------------------------------------------------------- beyond the initial bound
FAR_BASE = [(6.0, (0.0, 30.0, 0.0), (12.0, 12.0, 12.0), (0.0, 0.0, 0.0), DIFF),
            (1000.0, (0.0, -1000.0, 0.0), (0, 0, 0), (.75, .75, .75), DIFF),
            (5.0, (-7.0, 5.0, 0.0), (0, 0, 0), (.75, .25, .25), SPEC)]
FAR_ORIG, FAR_TARGET = (0.0, 8.0, 40.0), (0.0, 8.0, 0.0)                  # looking along -z
FAR = {
    # centred 2e20 down the view direction: b * b overflows, det is NaN, a miss
    "beyond_1e20": (1e19, (0.0, 8.0, -2e20), (0, 0, 0), (.5, .5, .5), DIFF),
    # around the camera, rad * rad overflows: the far root is +inf > 1e20, a miss
    "enclosing_inf_root": (2e19, (0.0, 8.0, 40.0), (0, 0, 0), (.5, .5, .5), DIFF),
    # the farthest a finite root gets: well inside the bound, whatever the oracle makes of it
    "far_inside_bound": (1e18, (0.0, 8.0, -1.5e19), (0, 0, 0), (.5, .5, .5), DIFF),
}


@pytest.mark.parametrize("counted", [False, True])
@pytest.mark.parametrize("far", sorted(FAR))
def test_sphere_beyond_the_initial_bound(rt, refs, far, counted):
    w, h, spp = 16, 16, 4
    rows = FAR_BASE + [FAR[far]]
    cam = _camera(rt, w, h, FAR_ORIG, FAR_TARGET)
    ref = refs(w, h, [spp], name=far, make=lambda: (_scene(rt, rows), cam))
    _render_and_compare(rt, ref, w, h, spp, counted, scene=_scene(rt, rows), cam=cam)
