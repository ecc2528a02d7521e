/* Host-side check of mp_role() (fiasco_amd/csrc/hip/mp_roles.h), the select chain by which a lane of mp_tables()
 * finds the table entry it computes.  reference_role() below is the mapping as mp_tables() had it before -- nested
 * ifs, first match wins, lanes from om + 12 on without a role -- kept here as the table the selects must reproduce:
 * every lane of the largest workgroup-independent range (tid < 256: the roles end below lane 140), every model size
 * the non-FC_HM builds accept (1 .. 64 DC symbols and symbols per context), contexts 0 .. 4, both kinds of band, the
 * default and the big role set.  Built and run by tests/test_gpu_call_fixed.py; no GPU. */
#include <cstdio>
#include <cstdlib>

#include "mp_roles.h"

static const int MAXED = 5;        /* FC_MAXED, frame_coder.h */

struct Ref { int role, ci, ti, dest, di, leaf; };

static Ref reference_role(int tid, int dcs, int sy, int ctx, int band, int half_nd, int half_dc, int big)
{
    Ref o = { 0, 0, 0, MPD_NONE, 0, 0 };
    const int om = 64 + sy + 12 <= 128 ? 64 + sy : 128;
    if (!(tid < om + 12)) return o;
    const int r = tid - om;
    if (tid < dcs) { o.role = 1; o.ci = tid; o.ti = 0; }
    else if (tid >= 64 && tid < 64 + sy) { o.role = 1; o.ci = dcs + ctx * sy + tid - 64; o.ti = ctx + 1; }
    else if (r == 6) { o.role = 1; o.ci = dcs + ctx * sy - 1; o.ti = ctx + 1; }
    else if (r >= 0 && r < MAXED + 1) { o.role = 2; o.ci = r; }
    else if (!big && (r == 7 || r == 8)) o.role = 3;
    else if (!big && r == 9 && !band) { o.role = 1; o.ci = dcs + ctx * sy + half_nd; o.ti = ctx + 1; }
    else if (!big && r == 10 && !band) { o.role = 1; o.ci = half_dc; o.ti = 0; }
    o.leaf = !big && r == 7;                 /* p = 1 - p: only a tree role ever sits there */
    if (o.role == 1) {
        if (tid < dcs) { o.dest = MPD_LGDC; o.di = tid; }
        else if (r == 6) o.dest = MPD_LGLV_M1;
        else if (!big && r == 9) o.dest = MPD_WB_ND;
        else if (!big && r == 10) o.dest = MPD_WB_DC;
        else { o.dest = MPD_LGLV; o.di = tid - 64; }
    } else if (o.role == 2) { o.dest = MPD_LTAB; o.di = o.ci; }
    else if (o.role == 3) { o.dest = MPD_TB; o.di = r - 7; }
    return o;
}

int main()
{
    long n = 0, bad = 0;
    for (int big = 0; big < 2; big++)
    for (int band = 0; band < 2; band++)
    for (int ctx = 0; ctx < 5; ctx++)
    for (int dcs = 1; dcs <= 64; dcs++)
    for (int sy = 1; sy <= 64; sy++) {
        /* rtob(0.5) of the two formats: any symbol of the context / of the DC model */
        const int half_nd = (sy * 3 + ctx) % sy, half_dc = (dcs * 5 + ctx) % dcs;
        if (mp_role_om(sy) != (64 + sy + 12 <= 128 ? 64 + sy : 128)) { printf("om differs at sy %d\n", sy); return 1; }
        for (int tid = 0; tid < 256; tid++, n++) {
            const Ref e = reference_role(tid, dcs, sy, ctx, band, half_nd, half_dc, big);
            const MpRole g = mp_role(tid, dcs, sy, ctx, band, half_nd, half_dc, MAXED, big);
            bool ok = g.kind == e.role && g.dest == e.dest && g.di == e.di;
            /* the indices count where the role reads them; a lane without such a role reads index 0 (in bounds) */
            if (e.role == 1) ok = ok && g.ci == e.ci && g.ti == e.ti;
            else if (e.role == 2) ok = ok && g.ci == e.ci && g.ti == 0;
            else ok = ok && g.ci == 0 && g.ti == 0;
            /* 1 - p is taken where the old code took it, as far as a role stores anything there */
            if (e.role != 0) ok = ok && g.leaf == e.leaf;
            /* what the kernel reads and writes at these indices without looking at the role */
            ok = ok && g.ci >= 0 && g.ci < dcs + 5 * sy && g.ti >= 0 && g.ti < 16 && g.di >= 0 && g.di < 64;
            if (g.dest == MPD_LTAB) ok = ok && g.di <= MAXED;
            if (g.dest == MPD_TB) ok = ok && g.di < 2;
            if (!ok && bad++ < 10)
                printf("tid %d dcs %d sy %d ctx %d band %d big %d: got kind %d ci %d ti %d dest %d di %d leaf %d, "
                       "expected role %d ci %d ti %d dest %d di %d leaf %d\n", tid, dcs, sy, ctx, band, big,
                       g.kind, g.ci, g.ti, g.dest, g.di, g.leaf, e.role, e.ci, e.ti, e.dest, e.di, e.leaf);
        }
    }
    if (bad) { printf("mp_roles_check: %ld of %ld lanes differ\n", bad, n); return 1; }
    printf("mp_roles_check: ok (%ld lanes)\n", n);
    return 0;
}
