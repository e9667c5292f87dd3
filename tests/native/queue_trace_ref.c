/*
 * tests/native/queue_trace_ref.c -- TEST INFRASTRUCTURE ONLY.
 *
 * The reference for rtq_trace / rtq_trace_async: the push and drain loop of
 * the oracle's q_pixel (oracle/queue_oracle.c, raytracer_non_OpenCL.c:309-434)
 * over the oracle's own q_raytrace, driven by the caller's rays instead of the
 * camera's.  A chain of `group` consecutive rays is what a pixel's nine
 * primaries are to q_pixel: acc = 0, then for each ray in order a Ray with
 * that origin and direction (weight 1, depth 0, origin_primitive -1, type
 * ORIGIN, r_index 1, transparency 1) is pushed and the FIFO drained, every
 * popped ray's term added to acc by its type, the reflected then the
 * refracted child pushed while depth < 5.  Per chain: acc.  Per ray: the root
 * q_raytrace call's distance and return.  Undefined behaviour as the oracle
 * defines it (no children, counted in counters[3]).
 * Built on demand by tests/queue_trace_ref.py with the oracle's CFLAGS.
 */
#include "../../oracle/queue_oracle.c"

#define QT_PUSH(R) do { if (back >= Q_MAXRAYS) back = 0; q[back++] = (R); nq++; } while (0)

static void trace_chain(const orq_primitive *P, int n, const float *rays, int group, float *color, float *t, int *id,
                        uint64_t *cnt)
{
    qray q[Q_MAXRAYS];
    int nq = 0, front = 0, back = 0;
    orq_f4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < group; k++) {
        const float *ray6 = rays + 6 * k;
        qray r;
        r.o.x = ray6[0]; r.o.y = ray6[1]; r.o.z = ray6[2]; r.o.w = 0.f;
        r.d.x = ray6[3]; r.d.y = ray6[4]; r.d.z = ray6[5]; r.d.w = 0.f;
        r.weight = 1.0f; r.depth = 0;
        r.origin_primitive = -1; r.type = 0; r.r_index = 1.0f;
        r.transparency.x = r.transparency.y = r.transparency.z = 1; r.transparency.w = 0;
        QT_PUSH(r);
        int is_root = 1;
        while (nq > 0) {
            if (front >= Q_MAXRAYS) front = 0;
            const qray cur = q[front++]; nq--;
            orq_f4 rc = {0.f, 0.f, 0.f, 0.f}, pi = {0.f, 0.f, 0.f, 0.f};
            float dist;
            int result = 0;
            cnt[0]++;
            const int prim = q_raytrace(&cur, &rc, &dist, &pi, &result, P, n, cnt);
            if (is_root) {
                if (t) t[k] = dist;
                if (id) id[k] = prim;
                is_root = 0;
            }
            if (cur.type == 0) {
                acc.x += rc.x * cur.weight;
                acc.y += rc.y * cur.weight;
                acc.z += rc.z * cur.weight;
            } else if (cur.type == 1) {
                const orq_f4 oc = P[cur.origin_primitive].m_color;
                acc.x += rc.x * cur.weight * oc.x * cur.transparency.x;
                acc.y += rc.y * cur.weight * oc.y * cur.transparency.y;
                acc.z += rc.z * cur.weight * oc.z * cur.transparency.z;
            } else {
                acc.x += rc.x * cur.weight * cur.transparency.x;
                acc.y += rc.y * cur.weight * cur.transparency.y;
                acc.z += rc.z * cur.weight * cur.transparency.z;
            }
            if (!(cur.depth < Q_TRACEDEPTH)) continue;
            if (prim < 0 || P[prim].is_light) {
                if (prim < 0 || P[prim].m_refl > 0.0f || P[prim].m_refr > 0.0f) cnt[3]++;
                continue;
            }
            const orq_primitive *hp = &P[prim];
            const float refl = hp->m_refl;
            if (refl > 0.0f) {
                const orq_f4 N = q_normal(hp, pi);
                const float td = QDOT(cur.d, N);
                orq_f4 R;
                R.x = cur.d.x - 2.0f * td * N.x;
                R.y = cur.d.y - 2.0f * td * N.y;
                R.z = cur.d.z - 2.0f * td * N.z;
                R.w = 0.f;
                qray nr;
                nr.o.x = pi.x + R.x * Q_EPS;
                nr.o.y = pi.y + R.y * Q_EPS;
                nr.o.z = pi.z + R.z * Q_EPS;
                nr.o.w = 0.f;
                nr.d = R;
                nr.depth = cur.depth + 1;
                nr.weight = refl * cur.weight;
                nr.type = 1;
                nr.origin_primitive = prim;
                nr.r_index = cur.r_index;
                nr.transparency = cur.transparency;
                QT_PUSH(nr);
            }
            const float refr = hp->m_refr;
            if (refr > 0.0f) {
                const float mri = hp->m_refr_index;
                const float nn = cur.r_index / mri;
                const orq_f4 tn = q_normal(hp, pi);
                orq_f4 N;
                N.x = tn.x * (float)result;
                N.y = tn.y * (float)result;
                N.z = tn.z * (float)result;
                const float td = QDOT(N, cur.d);
                const float cosI = -td;
                const float cosT2 = 1.0f - nn * nn * (1.0f - cosI * cosI);
                if (cosT2 > 0.0f) {
                    const float kk = nn * cosI - sqrtf(cosT2);
                    orq_f4 T;
                    T.x = (nn * cur.d.x) + kk * N.x;
                    T.y = (nn * cur.d.y) + kk * N.y;
                    T.z = (nn * cur.d.z) + kk * N.z;
                    T.w = 0.f;
                    qray nr;
                    nr.o.x = pi.x + T.x * Q_EPS;
                    nr.o.y = pi.y + T.y * Q_EPS;
                    nr.o.z = pi.z + T.z * Q_EPS;
                    nr.o.w = 0.f;
                    nr.d = T;
                    nr.depth = cur.depth + 1;
                    nr.weight = cur.weight;
                    nr.type = 2;
                    nr.origin_primitive = prim;
                    nr.r_index = mri;
                    nr.transparency.x = cur.transparency.x * expf(hp->m_color.x * 0.15f * (-dist));
                    nr.transparency.y = cur.transparency.y * expf(hp->m_color.y * 0.15f * (-dist));
                    nr.transparency.z = cur.transparency.z * expf(hp->m_color.z * 0.15f * (-dist));
                    nr.transparency.w = 0.f;
                    QT_PUSH(nr);
                }
            }
        }
    }
    color[0] = acc.x; color[1] = acc.y; color[2] = acc.z;
}

/* rays: 6 floats each, nrays a multiple of group.  color [3 nrays / group],
 * t [nrays], id [nrays] (t and id nullable); counters[4] (rays traced, shadow
 * rays, intersect calls, undefined-behaviour events) are set, not accumulated
 * into. */
void qtr_trace(const orq_primitive *P, int n, const float *rays, size_t nrays, int group, float *color, float *t,
               int *id, uint64_t *counters, int nthreads)
{
    uint64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    const long long nchains = (long long)(nrays / (size_t)group);
    if (nthreads < 1) nthreads = 1;
#pragma omp parallel for schedule(dynamic, 64) num_threads(nthreads) reduction(+ : c0, c1, c2, c3) if (nthreads > 1)
    for (long long c = 0; c < nchains; c++) {
        uint64_t k[4] = {0, 0, 0, 0};
        const long long r0 = c * group;
        trace_chain(P, n, rays + 6 * r0, group, color + 3 * c, t ? t + r0 : 0, id ? id + r0 : 0, k);
        c0 += k[0]; c1 += k[1]; c2 += k[2]; c3 += k[3];
    }
    counters[0] = c0; counters[1] = c1; counters[2] = c2; counters[3] = c3;
}
