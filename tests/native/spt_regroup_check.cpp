// spt_regroup_check.cpp -- test-only CPU checks of the hierarchy regroup
// (csrc/spt_regroup.h).  The sections, the containment check and the scalar
// walks are those of spt_refit_check.cpp, which this file includes whole (its
// State and its rfc_* entry points serve the regrouped sections as they
// stand); added here are the per-node topology beside Meta, regroup_host and
// the summed surface area of the binary nodes' boxes.
// tests/regroup_check.py builds this file into a shared library with
// g++ -O2 -std=c++17 -ffp-contract=off -pthread; with -DSPT_REGROUP_MAIN it is
// a stand-alone program (scenes and edits of its own) for a run under
// -fsanitize=address,undefined,float-cast-overflow.
#include "spt_refit_check.cpp"
#include "spt_regroup.h"

namespace {

struct Regroup {
    State *S = nullptr;
    sptregroup::Topo topo;
    ~Regroup() { delete S; }
};

Regroup *rg_create(const rt_sphere *sp, int n, int wide)
{
    Regroup *R = new Regroup();
    R->S = create(sp, n, wide);
    if (!R->S) { delete R; return nullptr; }
    // the builders once more (they are deterministic), as refit_prepare runs them
    std::vector<int> always;
    sptbvh::BvhBuild b;
    sptbvh::partition_and_build(R->S->sp.data(), n, always, b);
    sptregroup::build_topo(b, R->S->meta, R->topo);
    return R;
}

void rg_regroup(Regroup *R, const rt_sphere *sp)
{
    State *S = R->S;
    S->sp.assign(sp, sp + S->n);
    sptregroup::regroup_host(S->meta, R->topo, S->sp.data(), S->nodes.data(), S->geo.data(), S->ids.data(),
                             S->wn ? S->words.data() : nullptr, S->wn ? S->maxid.data() : nullptr, S->nbox);
}

// Summed surface area of the binary nodes' boxes (empty boxes count nothing).
double rg_area(const Regroup *R)
{
    double sum = 0;
    for (int i = 0; i < R->S->nn; i++) {
        const float *o = &R->S->nbox[8 * (size_t)i];
        if (!(o[0] <= o[4] && o[1] <= o[5] && o[2] <= o[6])) continue;
        const double x = (double)o[4] - o[0], y = (double)o[5] - o[1], z = (double)o[6] - o[2];
        sum += 2.0 * (x * y + y * z + z * x);
    }
    return sum;
}

}  // namespace

extern "C" {

void *rgc_create(const rt_sphere *sp, int n, int wide) { return rg_create(sp, n, wide); }
void rgc_destroy(void *r) { delete (Regroup *)r; }
// The State behind a handle, for the rfc_* entry points.
void *rgc_state(void *r) { return ((Regroup *)r)->S; }
void rgc_regroup(void *r, const rt_sphere *sp) { rg_regroup((Regroup *)r, sp); }
double rgc_area(const void *r) { return rg_area((const Regroup *)r); }
// out[0]: levels of the tree  [1]: levels sorted by global passes  [2]: subtree roots of the LDS tier
// (sub_max < 0: the library's default size of that tier)
void rgc_plan(const void *r, int sub_max, long long *out)
{
    const Regroup *R = (const Regroup *)r;
    sptregroup::Plan p;
    sptregroup::build_plan(R->S->meta, R->topo, sub_max < 0 ? sptregroup::SUB_DEFAULT : sub_max, p);
    out[0] = p.levels;
    out[1] = (long long)p.lev_count.size();
    out[2] = (long long)p.sub.size() / 2;
}

}  // extern "C"

#ifdef SPT_REGROUP_MAIN
// Stand-alone run: a small and a larger cloud over a ground sphere; per scene
// a regroup of the scene as built, of a moved scene, of every tree sphere on
// one point, and of ten kinds of degenerate floats (negative, zero and
// non-finite radii and centres), each followed by the containment check, both
// walks against the full scan, and a second regroup that must change nothing.
namespace {
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
double uni()
{
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_rng >> 11) / 9007199254740992.0;
}
std::vector<rt_sphere> scene(int n, float half)
{
    std::vector<rt_sphere> v(n);
    for (int i = 0; i < n; i++) {
        rt_sphere &q = v[i];
        memset(&q, 0, sizeof(q));
        q.rad = (float)pow(10.0, -2.5 + 2.0 * uni());
        q.p.x = (float)((2 * uni() - 1) * half);
        q.p.y = (float)((2 * uni() - 1) * half);
        q.p.z = (float)((2 * uni() - 1) * half);
        q.c.x = q.c.y = q.c.z = 0.5f;
        q.refl = i % 3;
    }
    v[0].rad = 1e4f; v[0].p.x = 0.f; v[0].p.y = -1e4f - half - 2.f; v[0].p.z = 0.f;
    v[1].rad = 3.f; v[1].e.x = v[1].e.y = v[1].e.z = 20.f;
    return v;
}
void degenerate(rt_sphere &q, int k, int j)
{
    float *c = j % 3 == 0 ? &q.p.x : (j % 3 == 1 ? &q.p.y : &q.p.z);
    switch (k) {
    case 0: q.rad *= -4.f; break;
    case 1: q.rad = 0.f; break;
    case 2: q.rad = 1e-40f; break;
    case 3: q.rad = INFINITY; break;
    case 4: q.rad = -INFINITY; break;
    case 5: q.rad = NAN; break;
    case 6: *c = j % 2 ? NAN : -NAN; break;
    case 7: *c = j % 2 ? -INFINITY : INFINITY; break;
    case 8: *c = j % 4 < 2 ? 3.4e38f : -3.4e38f; break;
    case 9: *c = j % 2 ? -0.f : 0.f; break;
    }
}
bool same_sections(const State *A, const State *B)
{
    auto eq = [](const auto &a, const auto &b) { return a.size() == b.size() && !memcmp(a.data(), b.data(), a.size() * sizeof(a[0])); };
    return eq(A->nodes, B->nodes) && eq(A->geo, B->geo) && eq(A->ids, B->ids) && eq(A->words, B->words) && eq(A->maxid, B->maxid);
}
int run(int n, float half, int nrays)
{
    const std::vector<rt_sphere> base = scene(n, half);
    std::vector<float> rays, maxt;
    for (int k = 0; k < nrays; k++) {
        float d[3] = {(float)(2 * uni() - 1), (float)(2 * uni() - 1), (float)(2 * uni() - 1)};
        const float l = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-9f;
        for (int a = 0; a < 3; a++) rays.push_back((float)((2 * uni() - 1) * half));
        for (int a = 0; a < 3; a++) rays.push_back(d[a] / l);
        maxt.push_back((float)(uni() * 2 * half));
    }
    int rc = 0;
    for (int edit = 0; edit < 13; edit++) {
        Regroup *R = rg_create(base.data(), n, 1);
        if (!R) return 1;
        State *S = R->S;
        std::vector<rt_sphere> v = base;
        if (edit == 1)
            for (int i = 2; i < n; i++) {
                v[i].p.x += (float)((2 * uni() - 1) * half);
                v[i].p.z += (float)((2 * uni() - 1) * half);
            }
        if (edit == 2)
            for (int j = 0; j < S->nb; j++) { rt_sphere &q = v[S->ids[j]]; q.p.x = 1.f; q.p.y = 2.f; q.p.z = 3.f; q.rad = 0.25f; }
        if (edit >= 3) {
            int j = 0;
            for (int i = 20; i < n; i += 7, j++) degenerate(v[i], edit - 3, j);
        }
        const std::vector<int> ids0 = S->ids;
        rg_regroup(R, v.data());
        char msg[256] = "";
        const long long bad = check(S, msg, sizeof(msg));
        const long long wrong = walk_check(S, rays.data(), nullptr, nrays, nullptr, nullptr) +
                                walk_check(S, rays.data(), maxt.data(), nrays, nullptr, nullptr);
        std::vector<int> a(ids0.begin(), ids0.begin() + S->nb), c(S->ids.begin(), S->ids.begin() + S->nb);
        std::sort(a.begin(), a.end());
        std::sort(c.begin(), c.end());
        const bool perm = a == c && std::equal(ids0.begin() + S->nb, ids0.end(), S->ids.begin() + S->nb);
        const State before = *S;
        rg_regroup(R, v.data());
        const bool again = same_sections(&before, S);
        printf("n %d edit %d: nodes %d wide %d violations %lld %s walk mismatches %lld permutation %s second regroup %s\n",
               n, edit, S->nn, S->wn, bad, msg, wrong, perm ? "yes" : "NO", again ? "equal" : "DIFFERS");
        // A second regroup changes nothing where no two centres tie along a
        // split (edits 0 and 1) or all of them do (edit 2: every stable sort
        // is then the identity).  The degenerate kinds put several spheres on
        // one coordinate (+-inf, +-3.4e38, +-0): such a tie group may straddle
        // a child boundary, and the deeper sorts reorder it between two calls.
        if (bad || wrong || !perm || (edit <= 2 && !again)) rc = 1;
        delete R;
    }
    return rc;
}
}  // namespace

int main()
{
    const int a = run(300, 5.f, 2000), b = run(3000, 30.f, 500);
    return a | b;
}
#endif
