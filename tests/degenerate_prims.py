"""Whitted and queue-tracer scenes whose primitives hold any floats, any
`type` and any light flag, shared by the CPU pins of the oracle
(tests/test_degenerate_prims.py) and the GPU parity tests
(tests/test_gpu_degenerate_prims.py).

Two sets per tracer:

  * a catalogue of named single-primitive edits (KINDS), each applied to the
    reference scene ("ref-<kind>") and to one lit random scene ("lit-<kind>":
    lit_scenes.whitted_walled(WALLED_DEEP_SEED), lit_scenes.queue_lit(
    QUEUE_EXACT_SEED)).  AIM names the primitive each edit goes to: one the
    camera sees, so that the edit changes the oracle's frame or counters
    against the unedited scene (asserted on the CPU).  NO_OP_KINDS lists the
    kinds (or single cases) that cannot change anything, with the reason;
  * fuzzed lit scenes ("fuzz-<seed>"): fuzz() replaces float words of a lit
    scene with special values.  The listed seeds are those whose oracle frames
    meet lit_scenes.check_lit -- a condition on the reference side alone.

Frames: Whitted 160 x 240 (the lit scenes at their own size), queue tracer
120 x 90 (reference scene) and 96 x 72 (lit scenes).

TEST INFRASTRUCTURE ONLY (imported like lit_scenes)."""
import functools

import numpy as np

import lit_scenes as L
import oracle_lib as O

NAN, INF = float("nan"), float("inf")
WORDS = 24                                   # both primitive records: 96 bytes
WHITTED_SIZE = (160, 240)
QUEUE_SIZE = (120, 90)


def _word(struct, field):
    return getattr(struct, field).offset // 4


def words_of(prims, n):
    """The first n 96-byte records as a writable uint32 [n, 24] copy."""
    return np.frombuffer(bytes(prims)[:96 * n], np.uint32).reshape(n, WORDS).copy()


def prims_of(struct, words):
    """A ctypes array of `struct` holding the uint32 [n, 24] words."""
    return (struct * len(words)).from_buffer_copy(np.ascontiguousarray(words, np.uint32).tobytes())


# ---------------------------------------------------------------- edits
# An edit maps the float32 words of one field of one primitive to new ones.
def _all(v):
    return lambda a: np.full_like(a, v)


def _first(v):
    def f(a):
        a = a.copy()
        a[0] = v
        return a
    return f


def _second(v):
    def f(a):
        a = a.copy()
        a[1] = v
        return a
    return f


def _neg(a):
    return -a


def _times5(a):
    return a * np.float32(5)


def _create_radius(r):
    """(m_SqRadius, m_Radius, m_RRadius) as Primitive_Create (scene.cpp:55-83)
    derives them from radius r."""
    r = np.float32(r)
    return lambda a: np.array([r * r, r, np.float32(1) / r if r > 0 else 0], np.float32)


def _q_radius(r):
    """(radius, sq_radius, r_radius) as scene.c derives them: r, r * r, 1 / r."""
    r = np.float32(r)

    return lambda a: np.array([r, r * r, np.float32(1) / r], np.float32)


# (kind, first field, number of words, edit).  Integer kinds: edit = an int.
_W = O.Primitive
WHITTED_KINDS = [
    # geometry
    ("centre_nan", "m_Centre", 3, _first(NAN)), ("centre_inf", "m_Centre", 3, _first(INF)),
    ("centre_zero", "m_Centre", 3, _all(0)), ("centre_neg", "m_Centre", 3, _neg),
    ("radius_nan", "m_SqRadius", 3, _create_radius(NAN)), ("radius_inf", "m_SqRadius", 3, _create_radius(INF)),
    ("radius_zero", "m_SqRadius", 3, _create_radius(0)), ("radius_sign", "m_Radius", 1, _neg),
    ("rradius_nan", "m_RRadius", 1, _all(NAN)), ("rradius_inf", "m_RRadius", 1, _all(INF)),
    ("rradius_zero", "m_RRadius", 1, _all(0)), ("rradius_neg", "m_RRadius", 1, _neg),
    ("sqradius_nan", "m_SqRadius", 1, _all(NAN)), ("sqradius_inf", "m_SqRadius", 1, _all(INF)),
    ("sqradius_zero", "m_SqRadius", 1, _all(0)), ("sqradius_neg", "m_SqRadius", 1, _neg),
    ("normal_zero", "plane_N", 3, _all(0)), ("normal_nan", "plane_N", 3, _first(NAN)),
    ("normal_times5", "plane_N", 3, _times5), ("plane_d_nan", "plane_D", 1, _all(NAN)),
    # materials
    ("colour_inf", "m_Color", 3, _first(INF)), ("colour_nan", "m_Color", 3, _second(NAN)),
    ("colour_neg", "m_Color", 3, _second(-3.0)), ("colour_huge", "m_Color", 3, _all(3e38)),
    ("rindex_zero", "m_RIndex", 1, _all(0)), ("rindex_nan", "m_RIndex", 1, _all(NAN)),
    ("rindex_neg", "m_RIndex", 1, _neg),
    ("refl_nan", "m_Refl", 1, _all(NAN)), ("refl_inf", "m_Refl", 1, _all(INF)),
    ("refr_nan", "m_Refr", 1, _all(NAN)), ("refr_inf", "m_Refr", 1, _all(INF)),
    ("diff_neg", "m_Diff", 1, _neg),
    ("spec_nan", "m_Spec", 1, _all(NAN)), ("spec_inf", "m_Spec", 1, _all(INF)), ("spec_neg", "m_Spec", 1, _neg),
    # lights and integer fields
    ("light_centre_nan", "m_Centre", 3, _first(NAN)), ("light_centre_inf", "m_Centre", 3, _second(INF)),
    ("light_colour_nan", "m_Color", 3, _first(NAN)),
    ("type_0", "type", 1, 0), ("type_3", "type", 1, 3), ("type_minus7", "type", 1, -7),
    ("light_flag_2", "m_Light", 1, 2), ("light_flag_minus1", "m_Light", 1, -1),
    ("plane_light", "m_Light", 1, 1),
]

_Q = O.QPrimitive
QUEUE_KINDS = [
    ("centre_nan", "center", 3, _first(NAN)), ("centre_inf", "center", 3, _first(INF)),
    ("centre_zero", "center", 3, _all(0)), ("centre_neg", "center", 3, _neg),
    ("radius_nan", "radius", 3, _q_radius(NAN)), ("radius_inf", "radius", 3, _q_radius(INF)),
    ("radius_zero", "radius", 3, _q_radius(0)), ("radius_sign", "radius", 1, _neg),
    ("rradius_nan", "r_radius", 1, _all(NAN)), ("rradius_inf", "r_radius", 1, _all(INF)),
    ("rradius_zero", "r_radius", 1, _all(0)), ("rradius_neg", "r_radius", 1, _neg),
    ("sqradius_nan", "sq_radius", 1, _all(NAN)), ("sqradius_inf", "sq_radius", 1, _all(INF)),
    ("sqradius_zero", "sq_radius", 1, _all(0)), ("sqradius_neg", "sq_radius", 1, _neg),
    ("normal_zero", "normal", 3, _all(0)), ("normal_nan", "normal", 3, _first(NAN)),
    ("normal_times5", "normal", 3, _times5), ("depth_nan", "depth", 1, _all(NAN)),
    ("colour_inf", "m_color", 3, _first(INF)), ("colour_nan", "m_color", 3, _second(NAN)),
    ("colour_neg", "m_color", 3, _second(-3.0)), ("colour_huge", "m_color", 3, _all(3e38)),
    ("rindex_zero", "m_refr_index", 1, _all(0)), ("rindex_nan", "m_refr_index", 1, _all(NAN)),
    ("rindex_neg", "m_refr_index", 1, _neg),
    ("refl_nan", "m_refl", 1, _all(NAN)), ("refl_inf", "m_refl", 1, _all(INF)),
    ("refr_nan", "m_refr", 1, _all(NAN)), ("refr_inf", "m_refr", 1, _all(INF)),
    ("diff_neg", "m_diff", 1, _neg),
    ("spec_nan", "m_spec", 1, _all(NAN)), ("spec_inf", "m_spec", 1, _all(INF)), ("spec_neg", "m_spec", 1, _neg),
    ("light_centre_nan", "center", 3, _first(NAN)), ("light_centre_inf", "center", 3, _second(INF)),
    ("light_colour_nan", "m_color", 3, _first(NAN)),
    ("type_2", "type", 1, 2), ("type_minus7", "type", 1, -7),
    ("light_flag_2", "is_light", 1, 2), ("plane_light", "is_light", 1, 1),
]

# Kinds that leave frame and counters as they were, and why that is right.
# A key is a kind (both base scenes) or a case id ("ref-<kind>": that base only).
NO_OP_KINDS = {
    "whitted": {
        "radius_sign": "Engine_Raytrace reads m_SqRadius and m_RRadius, never m_Radius",
        "light_flag_2": "every test of m_Light is '> 0' or '== 0' (raytracer.cpp:53,73,100): 2 is 1",
    },
    "queue": {
        "radius_sign": "raytrace reads sq_radius and r_radius, never radius",
        "light_flag_2": "is_light is only ever tested for non-zero",
        "ref-refr_inf": "m_refr is only ever tested '> 0.0f'.  On the reference scene's glass spheres inf is 1.0; "
                        "its other non-light primitives have m_refr_index 0, so nn = inf, and with their unit "
                        "sphere normals and plane normals shorter than 1 cosI * cosI <= 1, so cosT2 is -inf or "
                        "NaN: no ray.  (Applied to each of the 17 primitives in turn, only the three lights change "
                        "anything, and that is the count of the reference's undefined reads.)  The lit scene has "
                        "a plane where cosI * cosI > 1 gives cosT2 = +inf: lit-refr_inf is aimed there",
    },
}


def no_op_reason(tracer, case):
    """The reason `case` ("<base>-<kind>") changes nothing, or None."""
    table = NO_OP_KINDS[tracer]
    return table.get(case, table.get(case.partition("-")[2]))


# The primitive each kind is aimed at, per base scene: {kind: index}.
AIM = {
    "whitted": {
        "ref": {
            "centre_nan": 2, "centre_inf": 2, "centre_zero": 2, "centre_neg": 2, "radius_nan": 2,
            "radius_inf": 2, "radius_zero": 2, "radius_sign": 2, "rradius_nan": 2, "rradius_inf": 2,
            "rradius_zero": 2, "rradius_neg": 2, "sqradius_nan": 2, "sqradius_inf": 2,
            "sqradius_zero": 2, "sqradius_neg": 2, "normal_zero": 0, "normal_nan": 0,
            "normal_times5": 0, "plane_d_nan": 0, "colour_inf": 2, "colour_nan": 2, "colour_neg": 13,
            "colour_huge": 2, "rindex_zero": 2, "rindex_nan": 2, "rindex_neg": 2, "refl_nan": 2,
            "refl_inf": 2, "refr_nan": 2, "refr_inf": 4, "diff_neg": 0, "spec_nan": 9, "spec_inf": 0,
            "spec_neg": 9, "light_centre_nan": 1, "light_centre_inf": 1, "light_colour_nan": 1,
            "type_0": 2, "type_3": 2, "type_minus7": 2, "light_flag_2": 1, "light_flag_minus1": 1,
            "plane_light": 0},
        "lit": {
            "centre_nan": 2, "centre_inf": 2, "centre_zero": 0, "centre_neg": 2, "radius_nan": 2,
            "radius_inf": 2, "radius_zero": 2, "radius_sign": 0, "rradius_nan": 2, "rradius_inf": 2,
            "rradius_zero": 2, "rradius_neg": 2, "sqradius_nan": 2, "sqradius_inf": 2,
            "sqradius_zero": 2, "sqradius_neg": 2, "normal_zero": 8, "normal_nan": 8,
            "normal_times5": 8, "plane_d_nan": 8, "colour_inf": 2, "colour_nan": 2, "colour_neg": 53,
            "colour_huge": 2, "rindex_zero": 2, "rindex_nan": 2, "rindex_neg": 2, "refl_nan": 2,
            "refl_inf": 2, "refr_nan": 2, "refr_inf": 9, "diff_neg": 2, "spec_nan": 8, "spec_inf": 2,
            "spec_neg": 8, "light_centre_nan": 18, "light_centre_inf": 18, "light_colour_nan": 18,
            "type_0": 2, "type_3": 2, "type_minus7": 2, "light_flag_2": 18, "light_flag_minus1": 18,
            "plane_light": 8},
    },
    "queue": {
        "ref": {
            "centre_nan": 1, "centre_inf": 1, "centre_zero": 1, "centre_neg": 1, "radius_nan": 1,
            "radius_inf": 1, "radius_zero": 1, "radius_sign": 1, "rradius_nan": 1, "rradius_inf": 1,
            "rradius_zero": 1, "rradius_neg": 1, "sqradius_nan": 1, "sqradius_inf": 1,
            "sqradius_zero": 1, "sqradius_neg": 1, "normal_zero": 0, "normal_nan": 0,
            "normal_times5": 0, "depth_nan": 0, "colour_inf": 1, "colour_nan": 1, "colour_neg": 12,
            "colour_huge": 1, "rindex_zero": 1, "rindex_nan": 1, "rindex_neg": 1, "refl_nan": 1,
            "refl_inf": 1, "refr_nan": 1, "refr_inf": 1, "diff_neg": 0, "spec_nan": 0, "spec_inf": 0,
            "spec_neg": 0, "light_centre_nan": 13, "light_centre_inf": 13, "light_colour_nan": 13,
            "type_2": 1, "type_minus7": 1, "light_flag_2": 13, "plane_light": 0},
        "lit": {
            "centre_nan": 3, "centre_inf": 3, "centre_zero": 0, "centre_neg": 3, "radius_nan": 3,
            "radius_inf": 3, "radius_zero": 3, "radius_sign": 0, "rradius_nan": 3, "rradius_inf": 3,
            "rradius_zero": 3, "rradius_neg": 3, "sqradius_nan": 3, "sqradius_inf": 3,
            "sqradius_zero": 3, "sqradius_neg": 3, "normal_zero": 1, "normal_nan": 1,
            "normal_times5": 1, "depth_nan": 1, "colour_inf": 3, "colour_nan": 3, "colour_neg": 19,
            "colour_huge": 3, "rindex_zero": 3, "rindex_nan": 3, "rindex_neg": 3, "refl_nan": 3,
            "refl_inf": 3, "refr_nan": 3, "refr_inf": 2, "diff_neg": 1, "spec_nan": 2, "spec_inf": 2,
            "spec_neg": 2, "light_centre_nan": 15, "light_centre_inf": 15, "light_colour_nan": 15,
            "type_2": 3, "type_minus7": 3, "light_flag_2": 15, "plane_light": 1},
    },
}

_SPEC = {"whitted": (O.Primitive, WHITTED_KINDS), "queue": (O.QPrimitive, QUEUE_KINDS)}


def apply_kind(tracer, words, kind, index):
    """A copy of the uint32 [n, 24] words with `kind` applied to primitive
    `index`."""
    struct, kinds = _SPEC[tracer]
    _, field, nw, edit = next(k for k in kinds if k[0] == kind)
    out = words.copy()
    if field == "is_light":                                  # a byte; the padding behind it stays
        b = out[index].view(np.uint8)
        b[getattr(struct, field).offset] = edit
        return out
    w0 = _word(struct, field)
    if isinstance(edit, int):
        out[index, w0] = np.array([edit], np.int32).view(np.uint32)[0]
    else:
        with np.errstate(all="ignore"):
            new = np.asarray(edit(out[index, w0:w0 + nw].view(np.float32)), np.float32)
        out[index, w0:w0 + nw] = new.view(np.uint32)
    return out


# ---------------------------------------------------------------- fuzz
FUZZ_VALUES = np.array([0.0, -0.0, INF, -INF, NAN, 1e-30, -1e-30, 3e38, -3e38, 1e-42, -1.0, -0.5, 7.5], np.float32)
# The float words: everything but type, the light flag (and its padding),
# plane_cell / dummy_3.
FUZZ_WORDS = {
    "whitted": [w for w in range(WORDS) if w not in (_word(_W, "type"), _word(_W, "m_Light"))
                and not _word(_W, "plane_cell") <= w < _word(_W, "plane_cell") + 4],
    "queue": [w for w in range(WORDS) if w not in (_word(_Q, "type"), _word(_Q, "is_light"), _word(_Q, "dummy_3"))],
}


def fuzz(tracer, words, seed, rate=0.04):
    """A copy of the words in which each float word was replaced, with
    probability `rate`, by one of FUZZ_VALUES or by its own negation."""
    rng = np.random.default_rng(seed)
    fw = FUZZ_WORDS[tracer]
    out = words.copy()
    hit = rng.random((len(words), len(fw))) < rate
    pick = rng.integers(0, len(FUZZ_VALUES) + 1, size=hit.shape)
    for i, j in zip(*np.nonzero(hit)):
        k = pick[i, j]
        if k == len(FUZZ_VALUES):
            out[i, fw[j]] ^= np.uint32(0x80000000)
        else:
            out[i, fw[j]] = FUZZ_VALUES[k:k + 1].view(np.uint32)[0]
    return out


# Fuzz seed s works on the lit scene of seed WALLED_SEEDS[s % 12] /
# QUEUE_SEEDS[s % 10].  Listed: the seeds whose oracle frames meet
# lit_scenes.check_lit (Whitted: under both semantics).
WHITTED_FUZZ_SEEDS = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11)
QUEUE_FUZZ_SEEDS = (0, 1, 5, 6, 7, 12, 13, 14, 19, 33)
# The two of each list with the most traced rays per primary ray.
WHITTED_FUZZ_DEEP = (6, 1)              # 4.6 and 4.3 traced rays per primary ray
QUEUE_FUZZ_DEEP = (6, 19)               # 24.4 and 23.0


# ---------------------------------------------------------------- cases
def _whitted_base(base):
    if base == "ref":
        P, n = O.whitted_scene()
        return words_of(P, n), WHITTED_SIZE
    P, n, w, h = L.whitted_walled(L.WALLED_DEEP_SEED)
    return words_of(P, n), (w, h)


def _queue_base(base):
    if base == "ref":
        P, n = O.queue_scene()
        return words_of(P, n), QUEUE_SIZE
    P, n, _, _ = L.queue_lit(L.QUEUE_EXACT_SEED)
    return words_of(P, n), (L.QUEUE_W, L.QUEUE_H)


def whitted_words(case):
    """(uint32 [n, 24] words, (w, h)) of a case id: "ref", "lit" (the
    unedited bases), "ref-<kind>", "lit-<kind>" or "fuzz-<seed>"."""
    head, _, tail = case.partition("-")
    if head == "fuzz":
        seed = int(tail)
        P, n, w, h = L.whitted_walled(L.WALLED_SEEDS[seed % len(L.WALLED_SEEDS)])
        return fuzz("whitted", words_of(P, n), seed), (w, h)
    words, size = _whitted_base(head)
    return (apply_kind("whitted", words, tail, AIM["whitted"][head][tail]) if tail else words), size


def queue_words(case):
    head, _, tail = case.partition("-")
    if head == "fuzz":
        seed = int(tail)
        P, n, _, _ = L.queue_lit(L.QUEUE_SEEDS[seed % len(L.QUEUE_SEEDS)])
        return fuzz("queue", words_of(P, n), seed), (L.QUEUE_W, L.QUEUE_H)
    words, size = _queue_base(head)
    return (apply_kind("queue", words, tail, AIM["queue"][head][tail]) if tail else words), size


WHITTED_CATALOGUE = ["%s-%s" % (b, k[0]) for b in ("ref", "lit") for k in WHITTED_KINDS]
QUEUE_CATALOGUE = ["%s-%s" % (b, k[0]) for b in ("ref", "lit") for k in QUEUE_KINDS]
WHITTED_FUZZ = ["fuzz-%d" % s for s in WHITTED_FUZZ_SEEDS]
QUEUE_FUZZ = ["fuzz-%d" % s for s in QUEUE_FUZZ_SEEDS]
WHITTED_CASES = WHITTED_CATALOGUE + WHITTED_FUZZ
QUEUE_CASES = QUEUE_CATALOGUE + QUEUE_FUZZ


@functools.lru_cache(maxsize=None)
def whitted_case(case):
    """(prims, n, w, h, (frame, counters), (frame_ocl, counters_ocl)): the
    case's primitives and the oracle's frames under both semantics, computed
    once, frames read-only."""
    words, (w, h) = whitted_words(case)
    P, n = prims_of(O.Primitive, words), len(words)
    cpu = O.whitted_render(w, h, nthreads=L.NT, prims=P, n=n)
    ocl = O.whitted_render_ocl(w, h, nthreads=L.NT, prims=P, n=n)
    cpu[0].setflags(write=False)
    ocl[0].setflags(write=False)
    return P, n, w, h, cpu, ocl


@functools.lru_cache(maxsize=None)
def queue_case(case):
    """(prims, n, w, h, frame, counters) with the oracle's frame, computed
    once, read-only.  The array holds one zero record before prims[0] (prims
    is a view from its second record on): the reference reads primitives[-1]
    when a ray leaves the scene, and a zero primitive there has no children
    -- the oracle's definition of that read."""
    words, (w, h) = queue_words(case)
    n = len(words)
    store = prims_of(O.QPrimitive, np.concatenate([np.zeros((1, WORDS), np.uint32), words]))
    P = (O.QPrimitive * n).from_buffer(store, 96)
    frame, cnt = O.queue_render(w, h, P, n, nthreads=L.NT)
    frame.setflags(write=False)
    return P, n, w, h, frame, cnt


def whitted_rays_per_primary(case):
    _, _, w, h, (_, cnt), _ = whitted_case(case)
    return L.rays_per_primary(cnt, w, L.whitted_windows(w, h)[0])


def queue_rays_per_primary(case):
    _, _, w, h, _, cnt = queue_case(case)
    return cnt[0] / float(9 * w * h)


def first_difference(ref, got):
    """None, or a message naming the first differing pixel of two frames
    (uint32 [h, w] or uint8 [h, w, 4])."""
    d = ref != got
    if d.ndim == 3:
        d = d.any(-1)
    bad = np.argwhere(d)
    if bad.size == 0:
        return None
    at = tuple(bad[0])
    fmt = (lambda v: "%08x" % int(v)) if ref.ndim == 2 else (lambda v: str(v.tolist()))
    return "%d pixels differ, first at %s (got %s want %s)" % (len(bad), list(at), fmt(got[at]), fmt(ref[at]))
