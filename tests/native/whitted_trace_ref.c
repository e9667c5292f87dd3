/*
 * tests/native/whitted_trace_ref.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference for rtw_trace / rtw_trace_async: one sub-sample of the
 * oracle's render_pixel (oracle/whitted_oracle.c, raytracer.cpp:353-511) per
 * caller ray, over the oracle's own engine_raytrace -- o_Ray = refl_Ray =
 * refr_Ray = the ray as given, input_Rindex = 1, the node arrays reset, the
 * root call, the 62 children in breadth-first order, the back-accumulation.
 * Per ray: tr_Color[0], tr_dist[0] and the root call's return.  Besides the
 * oracle's four counters it reports the TIR nodes (index < 31) by what their
 * stale refraction ray is: an earlier node's, or the caller's own ray.
 * Built on demand by tests/whitted_trace_ref.py with the oracle's CFLAGS.
 */
#include "../../oracle/whitted_oracle.c"

static void trace_one(const or_primitive *P, int n, const float *ray6, int ocl, float *color, float *t_out,
                      int *id_out, wcount *cnt, uint64_t *stale_kind)
{
    ray_t o_ray, refl_ray, refr_ray;
    ray_t tr_refl_ray[NODECOUNT], tr_refr_ray[NODECOUNT];
    float cx[NODECOUNT], cy[NODECOUNT], cz[NODECOUNT];
    float tr_refl[NODECOUNT], tr_refr[NODECOUNT], tr_rindex[NODECOUNT], tr_dist[NODECOUNT];
    int tr_refl_index[NODECOUNT], tr_refr_index[NODECOUNT];
    int wrote_refr = 0;     /* some call so far has written refr_ray */

    for (int i = 0; i < NODECOUNT; i++) {
        cx[i] = cy[i] = cz[i] = 0;
        tr_refl[i] = 0; tr_refl_index[i] = -1; tr_rindex[i] = 1.0f;
        tr_refr[i] = 0; tr_refr_index[i] = -1; tr_dist[i] = 0;
    }
    o_ray.o.x = ray6[0]; o_ray.o.y = ray6[1]; o_ray.o.z = ray6[2];
    o_ray.d.x = ray6[3]; o_ray.d.y = ray6[4]; o_ray.d.z = ray6[5];
    refl_ray = o_ray;
    tr_refl_ray[0] = o_ray;
    refr_ray = o_ray;

    float dist = 0, refl = 0, refr = 0, rin = 1.0f;
    int refl_index = -1, refr_index = -1;
    vec3 acc = {0, 0, 0};
    const int root = engine_raytrace(P, n, &o_ray, &acc, 1, &rin, &dist, &refl, &refl_index, &refl_ray,
                                     &refr, &refr_index, &refr_ray, cnt, ocl);
    cx[0] = acc.x; cy[0] = acc.y; cz[0] = acc.z;
    tr_refl_ray[0] = refl_ray; tr_refl[0] = refl; tr_refl_index[0] = refl_index;
    tr_refr_ray[0] = refr_ray; tr_rindex[0] = rin; tr_refr[0] = refr;
    tr_refr_index[0] = refr_index; tr_dist[0] = dist;
    if (refr_index > -1) wrote_refr = 1;
    if (refr > 0 && refr_index == -1) { cnt->tir++; stale_kind[wrote_refr ? 0 : 1]++; }

    for (int i = 1; i < NODECOUNT; i += 2) {
        int p = (i - 1) / 2;
        for (int side = 0; side < 2; side++) {
            int c = i + side;
            float flag = side == 0 ? tr_refl[p] : tr_refr[p];
            if (flag > 0) {
                o_ray = side == 0 ? tr_refl_ray[p] : tr_refr_ray[p];
                acc.x = cx[c]; acc.y = cy[c]; acc.z = cz[c];
                dist = 0; refl = 0; refr = 0; refl_index = -1; refr_index = -1;
                rin = tr_rindex[p];
                engine_raytrace(P, n, &o_ray, &acc, 1, &rin, &dist, &refl, &refl_index,
                                &refl_ray, &refr, &refr_index, &refr_ray, cnt, ocl);
                cx[c] = acc.x; cy[c] = acc.y; cz[c] = acc.z;
                tr_refl_ray[c] = refl_ray; tr_refl[c] = refl; tr_refl_index[c] = refl_index;
                tr_refr_ray[c] = refr_ray; tr_refr[c] = refr; tr_refr_index[c] = refr_index;
                tr_rindex[c] = rin; tr_dist[c] = dist;
                if (refr_index > -1) wrote_refr = 1;
                if (c < NODECOUNT / 2 && refr > 0 && refr_index == -1) {
                    cnt->tir++;
                    stale_kind[wrote_refr ? 0 : 1]++;
                }
            } else {
                cx[c] = cy[c] = cz[c] = 0;
                tr_refl[c] = 0; tr_refl_index[c] = -1;
                tr_refr[c] = 0; tr_refr_index[c] = -1;
            }
        }
    }

    for (int i = NODECOUNT - 1; i >= 2; i -= 2) {
        int p = (i - 1) / 2;
        for (int k = 0; k < 2; k++) {
            const int refr_side = ocl ? (k == 1) : (k == 0);
            if (refr_side) {
                acc.x = cx[i]; acc.y = cy[i]; acc.z = cz[i];
                if ((tr_refr_index[p] > -1) && (tr_refr[p] > 0)) {
                    const or_primitive *q = &P[tr_refr_index[p]];
                    vec3 ab;
                    ab.x = q->m_Color.x * 0.15f * -tr_dist[p];
                    ab.y = q->m_Color.y * 0.15f * -tr_dist[p];
                    ab.z = q->m_Color.z * 0.15f * -tr_dist[p];
                    acc.x = cx[i] * expf(ab.x);
                    acc.y = cy[i] * expf(ab.y);
                    acc.z = cz[i] * expf(ab.z);
                }
            } else {
                acc.x = cx[i - 1]; acc.y = cy[i - 1]; acc.z = cz[i - 1];
                if ((tr_refl_index[p] > -1) && (tr_refl[p] > 0)) {
                    const or_primitive *q = &P[tr_refl_index[p]];
                    acc.x = cx[i - 1] * q->m_Color.x * tr_refl[p];
                    acc.y = cy[i - 1] * q->m_Color.y * tr_refl[p];
                    acc.z = cz[i - 1] * q->m_Color.z * tr_refl[p];
                }
            }
            cx[p] += acc.x; cy[p] += acc.y; cz[p] += acc.z;
        }
    }
    color[0] = cx[0]; color[1] = cy[0]; color[2] = cz[0];
    *t_out = tr_dist[0];
    *id_out = root;
}

/* rays: 6 floats each.  color [3 nrays], t [nrays], id [nrays]; counters[4]
 * (traced, shadow, tests, tir) and stale[2] (TIR nodes < 31 whose refraction
 * child runs along an earlier node's refraction ray / along the caller's own
 * ray) are set, not accumulated into. */
void wtr_trace(const or_primitive *P, int n, const float *rays, size_t nrays, int ocl, float *color, float *t,
               int *id, uint64_t *counters, uint64_t *stale, int nthreads)
{
    uint64_t t_traced = 0, t_shadow = 0, t_tests = 0, t_tir = 0, s0 = 0, s1 = 0;
    if (nthreads < 1) nthreads = 1;
#pragma omp parallel for schedule(dynamic, 256) num_threads(nthreads) \
    reduction(+ : t_traced, t_shadow, t_tests, t_tir, s0, s1) if (nthreads > 1)
    for (long long r = 0; r < (long long)nrays; r++) {
        wcount c = {0, 0, 0, 0};
        uint64_t sk[2] = {0, 0};
        trace_one(P, n, rays + 6 * r, ocl, color + 3 * r, t + r, id + r, &c, sk);
        t_traced += c.traced; t_shadow += c.shadow; t_tests += c.tests; t_tir += c.tir;
        s0 += sk[0]; s1 += sk[1];
    }
    counters[0] = t_traced; counters[1] = t_shadow; counters[2] = t_tests; counters[3] = t_tir;
    stale[0] = s0; stale[1] = s1;
}
