// accept_key_check.cpp -- CPU proof of csrc/spt_accept.h: the integer-key
// accept tests of smallpt's branch-free sphere loops decide exactly what the
// reference's float comparisons decide.
//
//   1. Every one of the 2^32 bit patterns of a root x, against a fixed set of
//      bounds: candidates (finite, > EPS) have keys below KEY_INF, strictly
//      increasing; everything else has a key >= KEY_INF; unkey(key(x)) is x;
//      and  x > EPS && x < bound  <=>  key(x) < limit_key(bound).
//   2. Root pairs t1 = b - sd, t2 = b + sd from edge and random b and sd
//      (sd >= 0 or NaN, as sqrt_nr returns): min(key(t1), key(t2)) is the
//      key of SphereIntersect's distance (geomfunc.h:32-59) or >= KEY_INF on
//      a miss; nearest_accept / any_accept agree with "d != 0 && d < bound"
//      for every bound, and a taken bound is the distance, bit for bit.
//   3. Whole queries over descending index sequences with repeated pairs
//      (ties): the taken index, the first taken index and the returned t are
//      Intersect's (:71-92), the occluded flag is IntersectP's (:94-110) --
//      including bounds <= EPS and NaN, which accept nothing and come back
//      unchanged.
//
// Usage: accept_key_check [threads [stride]]     exit status 0 iff everything
// holds.  stride > 1 (the sanitizer build's run, which looks for faults of the
// program, not of the keys) sweeps every stride-th block of 2^16 patterns and
// the blocks around the edges.
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "spt_accept.h"

using namespace rt::sptaccept;

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float fbits(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

static std::vector<float> bounds()
{
    return {1e20f, EPS, nextafterf(EPS, INFINITY), nextafterf(EPS, -INFINITY), 0.f, -1.f, 1e-40f, 1.f, FLT_MAX, NAN,
            // beyond the required set
            -0.f, INFINITY, -INFINITY, 0.02f, fbits(0xffc00000u)};
}

// SphereIntersect's result from its two roots (0 = miss).
static float ref_distance(float t1, float t2)
{
    if (t1 > EPS) return t1;
    if (t2 > EPS) return t2;
    return 0.f;
}

static std::atomic<int> failures{0};
#define FAIL(...)                                                  \
    do {                                                           \
        if (failures.fetch_add(1) < 20) { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } \
    } while (0)

// ---- 1: all bit patterns [lo, hi)
static void sweep_report(uint64_t lo, uint64_t hi, const std::vector<float> &B);

// Blocks at or beside +-0, EPS, FLT_MAX, +-inf and the last pattern.
static bool edge_block(uint64_t b0)
{
    for (uint64_t e : {0x0ull, 0x3c23d70aull, 0x7f7fffffull, 0x7f800000ull, 0x80000000ull, 0xff800000ull, 0xffffffffull})
        if (e >> 16 == b0 >> 16 || (e >> 16) + 1 == b0 >> 16 || e >> 16 == (b0 >> 16) + 1) return true;
    return false;
}

// Branch-free over blocks of patterns (the compiler vectorises it); a block
// with any mismatch is gone through again by sweep_report, which names them.
static void sweep(uint64_t lo, uint64_t hi, const std::vector<float> &B, uint64_t stride)
{
    constexpr int MAXB = 32;
    float Bf[MAXB];
    uint32_t L[MAXB];
    const int nb = (int)B.size();
    if (nb > MAXB) abort();
    for (int j = 0; j < nb; j++) {
        Bf[j] = B[j];
        L[j] = limit_key(B[j]);
    }
    const uint64_t BLOCK = 1 << 16;
    for (uint64_t b0 = lo; b0 < hi; b0 += BLOCK) {
        const uint64_t b1 = b0 + BLOCK < hi ? b0 + BLOCK : hi;
        if (stride > 1 && (b0 >> 16) % stride != 0 && !edge_block(b0)) continue;
        uint32_t bad = 0;
        for (uint64_t u64 = b0; u64 < b1; u64++) {
            const uint32_t u = (uint32_t)u64;
            const float x = __builtin_bit_cast(float, u);
            const uint32_t k = key(x);
            const bool cand = x > EPS && x < INFINITY;
            bad |= (uint32_t)(cand != (k < KEY_INF));
            bad |= (uint32_t)(__builtin_bit_cast(uint32_t, unkey(k)) != u);
            const float nx = __builtin_bit_cast(float, u + 1);
            bad |= (uint32_t)(cand & (nx > EPS) & (nx < INFINITY) & !(key(nx) > k));
            for (int j = 0; j < nb; j++) bad |= (uint32_t)(((x > EPS) & (x < Bf[j])) != (k < L[j]));
        }
        if (bad) sweep_report(b0, b1, B);
    }
}

static void sweep_report(uint64_t lo, uint64_t hi, const std::vector<float> &B)
{
    std::vector<uint32_t> L;
    for (float b : B) L.push_back(limit_key(b));
    const size_t nb = B.size();
    for (uint64_t u64 = lo; u64 < hi; u64++) {
        const uint32_t u = (uint32_t)u64;
        const float x = fbits(u);
        const uint32_t k = key(x);
        const bool cand = x > EPS && x < INFINITY;
        if (cand != (k < KEY_INF)) FAIL("candidate/key mismatch at %08x: key %08x", u, k);
        if (bits(unkey(k)) != u) FAIL("unkey(key) != x at %08x", u);
        if (cand) {
            const float nx = fbits(u + 1);
            if (nx > EPS && nx < INFINITY && !(key(nx) > k)) FAIL("key not increasing at %08x", u);
        }
        for (size_t j = 0; j < nb; j++) {
            const bool f = x > EPS && x < B[j];
            if (f != (k < L[j])) FAIL("x %08x bound %08x: float %d key %d", u, bits(B[j]), (int)f, (int)(k < L[j]));
        }
    }
}

struct Rng {
    uint64_t s;
    uint32_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); }
    float unit() { return (next() >> 8) * (1.f / 16777216.f); }
};

struct Pair { float t1, t2; };

// ---- 2: one root pair against every bound
static void check_pair(float b, float sd, const std::vector<float> &B)
{
    const float t1 = b - sd, t2 = b + sd;
    const float d = ref_distance(t1, t2);
    const uint32_t k1 = key(t1), k2 = key(t2), km = k1 < k2 ? k1 : k2;
    const bool hit = d != 0.f && d < INFINITY;
    if (!(t1 <= t2) && (k1 < KEY_INF || k2 < KEY_INF)) FAIL("unordered roots with a candidate: b %a sd %a", b, sd);
    if (hit != (km < KEY_INF)) FAIL("hit/key mismatch: b %a sd %a", b, sd);
    if (hit && bits(unkey(km)) != bits(d)) FAIL("distance mismatch: b %a sd %a", b, sd);
    for (float bound : B) {
        const bool ref = d != 0.f && d < bound;
        uint32_t tb = limit_key(bound);
        const uint32_t tb0 = tb;
        const bool take = nearest_accept(tb, t1, t2);
        if (take != ref) FAIL("take mismatch: b %a sd %a bound %a", b, sd, bound);
        if (take && bits(unkey(tb)) != bits(d)) FAIL("taken bound is not d: b %a sd %a bound %a", b, sd, bound);
        if (!take && tb != tb0) FAIL("bound moved without take: b %a sd %a bound %a", b, sd, bound);
        uint32_t acc = KEY_NONE;
        any_accept(acc, t1, t2);
        if (any_result(acc, bound) != ref) FAIL("any-hit mismatch: b %a sd %a bound %a", b, sd, bound);
    }
}

// ---- 3: one query over pairs[n-1 .. 0]
static void check_query(const Pair *p, int n, float t_in)
{
    float t = t_in;
    int id = -1, first = -1;
    for (int i = n - 1; i >= 0; i--) {
        const float d = ref_distance(p[i].t1, p[i].t2);
        if (d != 0.f && d < t) {
            t = d;
            id = i;
            if (first < 0) first = i;
        }
    }
    uint32_t tb = limit_key(t_in), acc = KEY_NONE;
    int kid = -1, kfirst = -1;
    for (int i = n - 1; i >= 0; i--) {
        const bool take = nearest_accept(tb, p[i].t1, p[i].t2);
        kid = take ? i : kid;
        kfirst = (kfirst < 0 && take) ? i : kfirst;
        any_accept(acc, p[i].t1, p[i].t2);
    }
    const float kt = nearest_result(tb, t_in);
    if (kid != id || kfirst != first || bits(kt) != bits(t))
        FAIL("query mismatch: n %d t_in %a: id %d/%d first %d/%d t %a/%a", n, t_in, kid, id, kfirst, first, kt, t);
    if (any_result(acc, t_in) != (id >= 0)) FAIL("occluded mismatch: n %d maxt %a", n, t_in);
}

int main(int argc, char **argv)
{
    int nthreads = argc > 1 ? atoi(argv[1]) : (int)std::thread::hardware_concurrency();
    if (nthreads < 1) nthreads = 1;
    if (nthreads > 16) nthreads = 16;
    const uint64_t stride = argc > 2 ? strtoull(argv[2], nullptr, 10) : 1;
    const std::vector<float> B = bounds();

    static_assert(KEY_INF == 0x435c28f5u, "KEY_INF");
    if (key(nextafterf(EPS, INFINITY)) != 0u || key(EPS) != 0xffffffffu || key(INFINITY) != KEY_INF) FAIL("key anchors");

    std::vector<std::thread> th;
    const uint64_t total = 1ull << 32, per = (total / nthreads) & ~0xffffull;      // whole blocks
    for (int i = 0; i < nthreads; i++)
        th.emplace_back(sweep, i * per, i == nthreads - 1 ? total : (i + 1) * per, std::cref(B), stride);

    // 2
    Rng rng{0x9e3779b97f4a7c15ull};
    std::vector<float> bs = {0.f, -0.f, EPS, nextafterf(EPS, INFINITY), nextafterf(EPS, -INFINITY), 2 * EPS, 0.005f, 0.02f,
                             1.f, -1.f, 100.f, -100.f, 1e20f, -1e20f, 2e20f, FLT_MAX, -FLT_MAX, INFINITY, -INFINITY, NAN,
                             1e-40f, -1e-40f, FLT_MIN, 1e-30f, 16777216.f};
    std::vector<float> sds = {0.f, NAN, 1e-40f, FLT_MIN, 0x1p-48f, 1e-6f, EPS, nextafterf(EPS, INFINITY), 0.005f, 0.02f, 1.f,
                              50.f, 100.f, 1e20f, FLT_MAX, INFINITY};
    for (int i = 0; i < 1500; i++) {
        const float mag = ldexpf(1.f + rng.unit(), (int)(rng.next() % 80) - 40);
        bs.push_back((rng.next() & 1) ? mag : -mag);
        if (i % 3 == 0) bs.push_back(fbits(rng.next()));                  // any pattern
        sds.push_back(ldexpf(1.f + rng.unit(), (int)(rng.next() % 80) - 40));
        if (i % 3 == 0) sds.push_back(fbits(rng.next() & 0x7fffffffu));   // any non-negative pattern, NaNs too
    }
    // roots close to EPS and to each other
    for (int i = 0; i < 500; i++) {
        bs.push_back(EPS * (0.5f + rng.unit()));
        sds.push_back(EPS * rng.unit());
    }
    size_t npairs = 0;
    for (float b : bs)
        for (float sd : sds) {
            check_pair(b, sd, B);
            npairs++;
        }

    // 3: pools with few distinct pairs, so equal distances meet
    size_t nqueries = 0;
    for (int q = 0; q < 300000; q++) {
        Pair pool[4];
        for (Pair &p : pool) {
            const float b = bs[rng.next() % bs.size()], sd = sds[rng.next() % sds.size()];
            p.t1 = b - sd;
            p.t2 = b + sd;
        }
        if (q % 2) {                                                      // mostly hits, within the scene's scale
            for (Pair &p : pool) {
                const float b = 200.f * rng.unit() - 20.f, sd = 30.f * rng.unit();
                p.t1 = b - sd;
                p.t2 = b + sd;
            }
        }
        Pair seq[12];
        const int n = 1 + (int)(rng.next() % 12);
        for (int i = 0; i < n; i++) seq[i] = pool[rng.next() % 4];
        for (float t_in : B) {
            check_query(seq, n, t_in);
            nqueries++;
        }
        // a bound that is one of the distances (a tie with the bound itself)
        const float d = ref_distance(seq[0].t1, seq[0].t2);
        check_query(seq, n, d);
        nqueries++;
    }

    for (std::thread &t : th) t.join();
    const int f = failures.load();
    printf("accept_key_check: %s patterns x %zu bounds, %zu root pairs, %zu queries: %s (%d failures)\n", stride > 1 ? "sampled" : "2^32", B.size(), npairs,
           nqueries, f ? "FAILED" : "ok", f);
    return f ? 1 : 0;
}
