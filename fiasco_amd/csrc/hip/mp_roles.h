/*
 *  mp_roles.h -- which table entry a lane of mp_tables() computes (mp_device.inc): the role of a lane as a
 *  chain of selects, so that every lane of a wave runs the same code whatever its role.
 *
 *  Plain C++ without a dependency: the frame kernel includes it, and so does the host-side check of the
 *  mapping (tests/mp_roles_check.cpp).
 */
#ifndef FIASCO_MP_ROLES_H
#define FIASCO_MP_ROLES_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPR_FN __host__ __device__ inline
#else
#define MPR_FN inline
#endif

/* whose counters the probability is made of */
enum { MPR_NONE = 0, MPR_COEFF = 1, MPR_POOL = 2, MPR_TREE = 3 };
/* where the logarithm goes: as a double (LGDC[di], LGLV[di], LGLV_M1), negated as a float (LTAB[di], TB[di]), through
 * sub_log2() (WB_ND, WB_DC: the placeholder weight prices), or nowhere */
enum { MPD_NONE = 0, MPD_LGDC, MPD_LGLV, MPD_LGLV_M1, MPD_LTAB, MPD_TB, MPD_WB_ND, MPD_WB_DC };

struct MpRole {
    int kind;           /* MPR_* */
    int ci, ti;         /* MPR_COEFF: index of the count / of the total; MPR_POOL: ci = index of the count; else 0 */
    int dest, di;       /* MPD_*, index inside the destination array */
    int leaf;           /* the probability is taken as 1 - p (the tree model's leaf symbol) */
};

/* first lane of the single roles: right behind the level's symbols when they still end in wave 1, else lane 128 */
MPR_FN int mp_role_om(int sy) { return 64 + sy + 12 <= 128 ? 64 + sy : 128; }

/* Lane tid of a call at coefficient context ctx, models of dcs DC symbols and sy symbols per context, `maxed` + 1 edge
 * counts.  big: the builds that price the tree and the placeholder weights elsewhere (no roles om + 7 .. om + 10);
 * band != 0 (chroma): no placeholder prices either.
 *     tid < dcs              DC symbol tid                              lgdc[tid]
 *     64 .. 64 + sy - 1      symbol tid - 64 of the context             lglv[tid - 64]
 *     om .. om + maxed       edge count tid - om                        Ltab[tid - om]
 *     om + 6                 the counter in front of the context        lglv_m1
 *     om + 7, om + 8         tree model, leaf / child                   tb[0], tb[1]
 *     om + 9, om + 10        weight 0.5 in the context / as DC          mp.wb_nd, mp.wb_dc
 * The conditions exclude one another (dcs <= 64 <= om - sy, maxed < 6), so their order does not matter.
 *
 * Shape: every condition is a flag worked out up front with & and |, every alternative a local value, and every
 * choice ONE `flag ? value : previous` -- the form the compiler turns into a select instruction.  A nested ?: or an
 * arm that computes something comes back as a branch, and a wave with several kinds of roles then runs them in turn. */
MPR_FN MpRole mp_role(int tid, int dcs, int sy, int ctx, int band, int half_nd, int half_dc, int maxed, int big)
{
    const int om = mp_role_om(sy), r = tid - om;
    const int base = dcs + ctx * sy;            /* first counter of the context */
    const bool small = !big;
    const bool dc = tid < dcs;
    const bool lv = (tid >= 64) & (tid < 64 + sy);
    const bool m1 = r == 6;
    const bool ed = (r >= 0) & (r <= maxed) & (r != 6);
    const bool tr = small & ((r == 7) | (r == 8));
    const bool wn = small & (band == 0) & (r == 9);
    const bool wd = small & (band == 0) & (r == 10);
    const bool ctxt = lv | m1 | wn;             /* the total is the context's */
    const bool coeff = dc | ctxt | wd, leaf = tr & (r == 7);
    const int ci_lv = base + tid - 64, ci_m1 = base - 1, ci_wn = base + half_nd;
    const int ti_ctx = ctx + 1, di_lv = tid - 64, di_tr = r - 7;
    int kind = MPR_NONE, ci = 0, ti = 0, dest = MPD_NONE, di = 0;
    kind = tr ? MPR_TREE : kind;   kind = ed ? MPR_POOL : kind;   kind = coeff ? MPR_COEFF : kind;
    ci = dc ? tid : ci;   ci = lv ? ci_lv : ci;   ci = m1 ? ci_m1 : ci;   ci = wn ? ci_wn : ci;
    ci = wd ? half_dc : ci;   ci = ed ? r : ci;
    ti = ctxt ? ti_ctx : ti;
    dest = dc ? MPD_LGDC : dest;   dest = lv ? MPD_LGLV : dest;   dest = m1 ? MPD_LGLV_M1 : dest;
    dest = ed ? MPD_LTAB : dest;   dest = tr ? MPD_TB : dest;
    dest = wn ? MPD_WB_ND : dest;  dest = wd ? MPD_WB_DC : dest;
    di = dc ? tid : di;   di = lv ? di_lv : di;   di = ed ? r : di;   di = tr ? di_tr : di;
    MpRole o;
    o.kind = kind; o.ci = ci; o.ti = ti; o.dest = dest; o.di = di; o.leaf = leaf;
    return o;
}

#endif
