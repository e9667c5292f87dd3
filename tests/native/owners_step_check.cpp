// CPU check of the owners' step of a flush pass (render_kernel, DQ): the
// straight-line two-entry form the kernel runs (index arithmetic from
// csrc/spt_policy.h, sq_owners*) against the per-entry loop it replaced,
// restated here.  Every state of one lane is enumerated: npend in {0, 1, 2}
// with npark <= npend, the head at every ring position, the lane's entries at
// distances from the head around 0, 32, 64 and the ring's end (so positions
// cover the ring and its wrap), m in {0, 1, 32, 63, 64}, every combination of
// lit bits, and the parked sample's number in {0, 1, 63}.  The float terms
// are 1, 2^-24 and -1 in an order in which (a + b) + c != a + (b + c), so a
// changed order of additions changes bits.  rad, the parked rad, the colour,
// both pending terms, pidx, npend and npark must come out equal bit for bit.
// Prints the number of states compared; exits non-zero at the first difference.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "spt_policy.h"

using namespace sptpolicy;

struct F3 { float x, y, z; };
static F3 add(F3 a, F3 b) { return F3{a.x + b.x, a.y + b.y, a.z + b.z}; }

// One lane's share of the kernel's state: registers and its LDS slots.
struct Lane {
    int pidx, npend, npark;
    F3 pc0;         // the oldest pending term (registers)
    F3 pend;        // SLOT_PEND: the second pending term
    F3 rad;         // the current sample's radiance (registers)
    F3 prad;        // SLOT_RAD: the parked sample's radiance
    F3 col;         // SLOT_COL: the running average
};

// render_kernel's fold: sample number `current`'s radiance into the average
// (rcp_nr is 1.f / x on its range, tests/test_gpu_math.py)
static void fold(Lane &L, F3 r, int current)
{
    F3 c = r;
    if (current != 0) {
        const float k1 = (float)current;
        const float k2 = 1.f / (k1 + 1.f);
        c.x = (L.col.x * k1 + r.x) * k2;
        c.y = (L.col.y * k1 + r.y) * k2;
        c.z = (L.col.z * k1 + r.z) * k2;
    }
    L.col = c;
}

// The per-entry loop (the kernel before this form).
static void step_loop(Lane &L, int head, int m, unsigned long long unocc, int prev)
{
    while (L.npend > 0) {
        const int rel = sq_rel(L.pidx & 255, head);
        if (rel >= m) break;
        const bool lit = (unocc >> rel) & 1ull;
        if (L.npark > 0) {
            if (lit) L.prad = add(L.prad, L.pc0);
            L.npark--;
            if (L.npark == 0) fold(L, L.prad, prev);
        } else if (lit) {
            L.rad = add(L.rad, L.pc0);
        }
        L.npend--;
        L.pidx >>= 8;
        if (L.npend > 0) L.pc0 = L.pend;
    }
}

// The straight-line form (render_kernel's statements, in its order).
static void step_flat(Lane &L, int head, int m, unsigned long long unocc, int prev)
{
    const SqOwners ow = sq_owners(L.pidx, L.npend, head, m, unocc);
    if (ow.r0) {
        const int nres = sq_owners_resolved(ow), nparked = sq_owners_parked(nres, L.npark);
        F3 pc1 = L.pc0;         // the second term: resolved now, or the oldest from here on
        if (L.npend == 2) pc1 = L.pend;
        if (nparked > 0) {
            F3 pr = L.prad;
            const bool add0 = ow.lit0, add1 = nparked == 2 && ow.lit1;
            if (add0) pr = add(pr, L.pc0);
            if (add1) pr = add(pr, pc1);
            if (add0 || add1) L.prad = pr;
            if (nparked == L.npark) fold(L, pr, prev);
        } else if (ow.lit0) {
            L.rad = add(L.rad, L.pc0);
        }
        if (ow.lit1 && nparked < 2) L.rad = add(L.rad, pc1);
        L.npark -= nparked;
        L.npend -= nres;
        L.pidx = sq_owners_shift(L.pidx, nres);
        L.pc0 = pc1;
    }
}

int main()
{
    const float E = 0x1p-24f;
    const int rels[] = {0, 1, 2, 30, 31, 32, 33, 62, 63, 64, 65, SQ_RING - 2};
    const int gaps[] = {1, 2, 3, 31, 32, 33, 62, 63, 64, SQ_RING - 1};
    const int ms[] = {0, 1, 32, 63, 64};
    const int prevs[] = {0, 1, 63};
    long n = 0;
    // the terms must tell the two orders apart
    if ((1.f + E) + -1.f == 1.f + (E + -1.f)) {
        printf("FAILED: the float terms do not depend on the order of additions\n");
        return 1;
    }
    for (int head = 0; head < SQ_RING; head++)
        for (int rel0 : rels)
            for (int gap : gaps) {
                const int rel1 = rel0 + gap;
                if (rel1 >= SQ_RING) continue;
                const int pos0 = sq_wrap(head + rel0), pos1 = sq_wrap(head + rel1);
                for (int npend = 0; npend <= 2; npend++)
                    for (int npark = 0; npark <= npend; npark++)
                        for (int m : ms)
                            for (int lits = 0; lits < 4; lits++)
                                for (int prev : prevs) {
                                    // bits of the other lanes' entries on, the lane's own as `lits` says
                                    unsigned long long unocc = 0x5a5a5a5aa5a5a5a5ull;
                                    if (rel0 < 64) unocc = (unocc & ~(1ull << rel0)) | ((unsigned long long)(lits & 1) << rel0);
                                    if (rel1 < 64) unocc = (unocc & ~(1ull << rel1)) | ((unsigned long long)(lits >> 1) << rel1);
                                    unocc &= m >= 64 ? ~0ull : (1ull << m) - 1;     // (have: lane < m)
                                    Lane a;
                                    memset(&a, 0, sizeof a);
                                    a.npend = npend;
                                    a.npark = npark;
                                    a.pidx = npend == 0 ? 0 : (npend == 1 ? pos0 : (pos0 | pos1 << 8));
                                    a.rad = F3{1.f, E, -1.f};
                                    a.prad = F3{-1.f, 1.f, E};
                                    a.pc0 = F3{E, -1.f, 1.f};
                                    a.pend = F3{-1.f, 1.f, E};
                                    a.col = F3{0.25f, 0.5f, 0.75f};
                                    Lane b = a;
                                    step_loop(a, head, m, unocc, prev);
                                    step_flat(b, head, m, unocc, prev);
                                    n++;
                                    if (memcmp(&a, &b, sizeof a) != 0) {
                                        printf("FAILED: head %d pos %d %d npend %d npark %d m %d lits %d prev %d:\n"
                                               "  loop pidx %x npend %d npark %d rad %a %a %a prad %a %a %a col %a %a %a pc0 %a %a %a\n"
                                               "  flat pidx %x npend %d npark %d rad %a %a %a prad %a %a %a col %a %a %a pc0 %a %a %a\n",
                                               head, pos0, pos1, npend, npark, m, lits, prev,
                                               a.pidx, a.npend, a.npark, a.rad.x, a.rad.y, a.rad.z, a.prad.x, a.prad.y, a.prad.z,
                                               a.col.x, a.col.y, a.col.z, a.pc0.x, a.pc0.y, a.pc0.z,
                                               b.pidx, b.npend, b.npark, b.rad.x, b.rad.y, b.rad.z, b.prad.x, b.prad.y, b.prad.z,
                                               b.col.x, b.col.y, b.col.z, b.pc0.x, b.pc0.y, b.pc0.z);
                                        return 1;
                                    }
                                }
            }
    printf("owners_step_check ok: %ld\n", n);
    return 0;
}
