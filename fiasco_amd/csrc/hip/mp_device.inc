/*
 *  mp_device.inc -- matching pursuit on the device (included by frame_coder.hip).
 *
 *  approximate_range / matching_pursuit / orthogonalize: reference codec/approx.c:74-699.
 *  Rate terms: rle_bits codec/domain-pool.c:737-793, aac_bits codec/coeff.c:215-240,
 *  rtob/btor lib/rpf.c:59-169, bits_bin_code lib/misc.c:223-244.
 *
 *  Code-shape rule of this file: NO dynamically indexed private arrays (they would live in
 *  scratch memory, one HBM/L2 round trip per access).  Everything per candidate is kept in
 *  registers through compile-time trip counts (templates on the step number n) and
 *  predication; wave-uniform step state is read from LDS once per pass.
 */
#include "mp_roles.h"                 /* which table entry a lane of mp_tables() computes */

/* ---- uniform state of one scan pass, held in scalar registers ----
 *
 * rle_bits (codec/domain-pool.c:737-793) of {kept vectors + candidate d} walks the merged,
 * ascending position list and adds bits_bin_code(x - last, N - 1 - last) per element.  For a
 * candidate that falls between the kept positions p[i-1] < d < p[i] everything before d and
 * everything after p[i] is the same for all candidates of that interval, so lane 0 prices
 * those parts once per step (mp_step_prepare) in the reference's order of float additions:
 *   pre[i]            bits after the elements below d,
 *   last/k/thr[i]     bits_bin_code of d itself is k or k+1 (d - last < thr),
 *   sfx[j], has       the kept elements after p[i] (their predecessor is a kept element),
 *   z0, zy            complete sums for position 0 (never emitted) and for the co-located
 *                     luminance state (left out of the list, domain-pool.c:757-772).
 * Per candidate that leaves one interval select, one compare and ONE data-dependent
 * bits_bin_code (p[i] directly after d).
 */
struct StepCtx {
    int      np;                 /* kept vectors (non-zero weight) of earlier steps */
    int      p[MAXED - 1];       /* their pool positions, ascending */
    float    pre[MAXED];
    int      last[MAXED], k[MAXED], thr[MAXED];
    unsigned cd, has;
    float    sfx[MAXED - 1];
    float    z0, zy;
    int      ypos;
    float    wb_dc, wb_nd;       /* weight bits incl. the 0.5 placeholder (DC / other) */
    float    ab, price, err;
    unsigned N;                  /* rle_model->n */
};

__device__ __forceinline__ int   uni(int v)      { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float unif(float v)   { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__device__ __forceinline__ void load_step_ctx(const MPState &mp, StepCtx &c)
{
    c.np = uni(mp.np);
#pragma unroll
    for (int i = 0; i < MAXED - 1; i++) { c.p[i] = uni(mp.psorted[i]); c.sfx[i] = unif(mp.s1_sfx[i]); }
#pragma unroll
    for (int i = 0; i < MAXED; i++) {
        c.pre[i] = unif(mp.s1_pre[i]); c.last[i] = uni(mp.s1_last[i]);
        c.k[i] = uni(mp.s1_k[i]); c.thr[i] = uni(mp.s1_thr[i]);
    }
    c.cd = (unsigned) uni((int) mp.s1_cd); c.has = (unsigned) uni((int) mp.s1_has);
    c.z0 = unif(mp.s1_z0); c.zy = unif(mp.s1_zy);
    c.ypos = uni(mp.ypos);
    c.wb_dc = unif(mp.wb_dc); c.wb_nd = unif(mp.wb_nd);
    c.ab = unif(mp.ab); c.price = unif(mp.price); c.err = unif(mp.err);
    c.N = (unsigned) uni(mp.N);
}

#define RLE_EMIT(x)                                                                      \
    do {                                                                                 \
        unsigned x_ = (unsigned) (x);                                                    \
        if (x_ && (N - 1 - last)) {                                                      \
            bits += (float) bits_bin_code(x_ - last, N - 1 - last);                      \
            last = x_ + 1;                                                               \
        }                                                                                \
    } while (0)

/* stage-1 estimate of the candidate at pool position d (codec/approx.c:433-462): rle_bits of
 * {kept vectors + d} merged in ascending order, weight bits with placeholder 0.5.
 * MAXNP = largest number of kept vectors the caller can have. */
/* NP >= 0: the caller has branched on the (wave-uniform) number of kept vectors, c.np == NP --
 * the interval selects of the other counts are not generated (NP = 0, the first step of every
 * call: none at all).  Same operations in the same order as the general form. */
/* LBQ: the quotient num^2 / den is replaced by an UPPER bound of it (hardware reciprocal, 1 ulp,
 * times 1 + 2^-21: four instructions instead of the eleven of an IEEE division), i.e. the result
 * is a LOWER bound of the estimate, tight to 5e-7 of the quotient.  For the block minima of the
 * sweep only: the rounds ask them which blocks they may skip, what a block holds is evaluated with
 * the exact estimate (LBQ = false) -- a lower bound in their place changes no result. */
template <int MAXNP, int NP = -1, bool LBQ = false>
__device__ __forceinline__ float stage1(const StepCtx &c, int d, int state, float num, float den)
{
    const int np = NP >= 0 ? NP : c.np;
    float bits = c.pre[0];
    int last = c.last[0], k = c.k[0], thr = c.thr[0], i = 0;
    bool cd = c.cd & 1u;
    int nextp = np > 0 ? c.p[0] : -1;
#pragma unroll
    for (int j = 0; j < MAXNP; j++)
        if (j < np && d > c.p[j]) {
            i = j + 1;
            bits = c.pre[j + 1]; last = c.last[j + 1]; k = c.k[j + 1]; thr = c.thr[j + 1];
            cd = (c.cd >> (j + 1)) & 1u;
            nextp = (j + 1 < MAXED - 1 && j + 1 < np) ? c.p[(j + 1) % (MAXED - 1)] : -1;
        }
    if (cd) bits += (float) ((d - last < thr) ? k : k + 1);
    const unsigned mv = c.N - 2u - (unsigned) d;
    if (nextp >= 0 && mv != 0) {
        bits += (float) bits_bin_code((unsigned) (nextp - d - 1), mv);
#pragma unroll
        for (int j = 1; j < MAXNP; j++)
            if (j > i && j < np && ((c.has >> j) & 1u)) bits += c.sfx[j];
    }
    if (d == 0) bits = c.z0;
    if (d == c.ypos) bits = c.zy;
    float weights_bits = state ? c.wb_nd : c.wb_dc;
    if (LBQ)
        return (bits + weights_bits + c.ab) * c.price + c.err
               - num * num * (__builtin_amdgcn_rcpf(den) * 1.00000047683715820312f);
    return (bits + weights_bits + c.ab) * c.price + c.err - num * num / den;
}

/* ---- coefficient prices that are the host's, bit for bit ----
 *
 * aac_bits (codec/coeff.c:228-236) runs `bits -= log2(count / (float) total)` on a FLOAT bits:
 * bits = (float) ((double) bits - log2(...)).  The reference's log2 is glibc's, the device's is
 * ROCm's ocml; over all floats in (0, 1] the two differ for about 0.1 % of the arguments, never
 * by more than LOG2_MAX_ULP ulps (the launcher's self test measures both, exhaustively).  A
 * difference that small changes the rounded float only if the exact difference lies within it of
 * a rounding boundary of the float grid -- checked here with a margin; in that (rare) case the
 * host's value of the logarithm is taken from the table the launcher built (DevFrame.l2_*). */
__device__ __noinline__ double log2_host(const Sh &sh, float p)
{
    double v = log2((double) p);
    const unsigned *keys = sh.par.l2_keys;
    if (keys) {
        const unsigned k = __float_as_uint(p), mask = sh.par.l2_mask;
        unsigned h = (k * 2654435761u) & mask;
        for (unsigned kk; (kk = keys[h]) != 0; h = (h + 1) & mask)
            if (kk == k) { v = sh.par.l2_vals[h]; break; }
    }
    return v;
}

/* (float) ((double) wb - log2_host(p)) given the device's lg = log2(p); p = count ci / total ti
 * of the active coefficient model, looked at only on the slow path */
__device__ __forceinline__ float sub_log2(const Sh &sh, float wb, double lg, int ci, int ti)
{
    const double r = (double) wb - lg;
    /* The float nearest to r changes under a perturbation of r by less than eps = 2^-46 only if r
     * lies within eps of the midpoint of two floats, i.e. if the 29 mantissa bits the float drops
     * are within eps / ulp(r) of 0x10000000.  With 2^-8 <= |r| < 2^40 (anything else takes the slow
     * path) eps / ulp(r) = 2^(6 - e) <= 2^14: one integer window test instead of two double
     * additions and conversions. */
    const unsigned long long rb = (unsigned long long) __double_as_longlong(r);
    const int e = (int) ((rb >> 52) & 0x7ffu) - 1023;
    const unsigned low = (unsigned) rb & 0x1fffffffu;
    if (e < -8 || e >= 40 || low - (0x10000000u - 0x4000u) <= 0x8000u)
        return (float) ((double) wb - log2_host(sh, sh.cb.cnt[ci] / (float) sh.cb.tot[ti]));
    return (float) r;
}

struct Eval { float costs, m_bits, w_bits, m_err, f[MAXED];
              unsigned symp;     /* out: the symbols of f[0..2] (MPState::symp) */
#if FC_GM
              int qc;            /* in: probability index of the candidate's position (quasi-arithmetic pools) */
#endif
};

/* btor without the normalisation loop (lib/rpf.c:114-169): same bits, clz instead */
__device__ __forceinline__ float btor_fast(int b, int mant, float range)
{
    if (b == -1) return 0.0f;
    int sign = b & 1;
    unsigned m = ((unsigned) b & ((1u << (mant + 1)) - 1)) >> 1;
    m <<= (23 - mant);
    float v;
    if (m == 0)
        v = sign ? -1.0f : 1.0f;
    else {
        int sh_ = __clz((int) m) - 9;              /* bring the top set bit to bit 22 */
        m <<= sh_;
        m <<= 1;
        v = __uint_as_float(((unsigned) sign << 31) | ((unsigned) (126 - sh_) << 23) | (m & 0x7fffffu));
    }
    return v * range;
}

/* full evaluation of the candidate (pool position d, state `state`) at step NN
 * (codec/approx.c:495-591; the self-feeding refresh :554-569 is omitted, SURVEY 7.3) */
/* mp / lglv: the call's state and the log2 table of its level's coefficient context (sh.mp / sh.lglv) */
template <int NN>
__device__ __forceinline__ void full_eval_n(const DevFrame &F, const Sh &sh, const MPState &mp, const double *lglv,
                                            int d, int state,
                                            float num, float den, float ip0, float ip1, float ip2,
                                            float ip3, Eval &ev)
{
    float f[NN + 1], r[NN + 1], nov[NN + 1], ipio[NN + 1], ipd[NN + 1][NN + 1];
    int   v[NN + 1], st[NN + 1], sym[NN + 1];
#pragma unroll
    for (int k = 0; k < NN; k++) {
        nov[k] = mp.norm_ov[k]; ipio[k] = mp.ipio[k];
        f[k] = ipio[k] / nov[k];
        v[k] = mp.indices[k]; st[k] = mp.into[k];
#pragma unroll
        for (int j = 0; j < NN; j++) ipd[k][j] = j < k ? mp.sel_ipdo[k][j] : 0.0f;
    }
    f[NN] = num / den; v[NN] = d; st[NN] = state;
#pragma unroll
    for (int j = 0; j < NN; j++) ipd[NN][j] = j == 0 ? ip0 : j == 1 ? ip1 : j == 2 ? ip2 : ip3;  /* <s_d,o_j> */
    /* back substitution with per-step rounding to the reduced precision format */
#pragma unroll
    for (int l = NN; l >= 0; l--) {
        int mant = st[l] ? sh.par.rpf_mant : sh.par.dc_mant;
        float range = st[l] ? sh.par.rpf_range : sh.par.dc_range;
        sym[l] = rtob_dev(f[l], mant, range);
        r[l] = f[l] = btor_fast(sym[l], mant, range);
#pragma unroll
        for (int k = 0; k < NN; k++)
            if (k < l) f[k] -= f[l] * ipd[l][k] / nov[k];
    }
    {
        unsigned sp = 0;
#pragma unroll
        for (int k = 0; k <= NN && k < 3; k++) sp |= SYMP_PUT(sym[k], k);
        ev.symp = sp;                 /* (weights 3, 4 of a big build: not carried) */
    }
    {   /* rate of the rounded combination: coefficients in selection order, positions of the
         * non-zero ones in ascending order.  rtob(btor(sym)) == sym (the quantised value times
         * range and divided by range again is exact), so the symbols are reused. */
        float wb = 0;
        int nn = 0;
        bool uses0 = false;
        const int ypos = mp.ypos;                   /* priced by the weights only */
#pragma unroll
        for (int k = 0; k <= NN; k++)
            if (sym[k] != -1) {
                wb = st[k] ? sub_log2(sh, wb, lglv[sym[k]],
                                      sh.par.dcs + (mp.level - sh.par.lc_min_opt) * sh.par.sy + sym[k],
                                      mp.level - sh.par.lc_min_opt + 1)
                           : sub_log2(sh, wb, sh.lgdc[sym[k]], sym[k], 0);
                if (v[k] != ypos) {
                    nn++;
                    uses0 = uses0 || v[k] == 0;
                }
            }
#if FC_GM
        if (sh.gm.ck[0] == FC_CK_UNIFORM) {          /* uniform_bits, codec/coeff.c:155-170 */
            wb = 0;
#pragma unroll
            for (int k = 0; k <= NN; k++)
                if (sym[k] != -1) wb += (float) ((st[k] ? sh.par.rpf_mant : sh.par.dc_mant) + 1);
        }
#endif
        ev.w_bits = wb;
        const unsigned N = (unsigned) mp.N;
        float bits = sh.Ltab[nn];
        bits += uses0 ? sh.Q1 : sh.Q0;
        unsigned last = 1;
        int prev = -1;
#pragma unroll
        for (int it = 0; it <= NN; it++) {          /* selection in ascending position order */
            int best = 0x7fffffff;
#pragma unroll
            for (int k = 0; k <= NN; k++)
                if (sym[k] != -1 && v[k] != ypos && v[k] > prev && v[k] < best) best = v[k];
            if (best != 0x7fffffff) { RLE_EMIT(best); prev = best; }
        }
#if FC_GM
        {   /* the other pools: qac_bits (codec/domain-pool.c:364-402), uniform_bits (:592-615), const_bits (:530-536)
             * of the vectors with a non-zero weight, in selection order */
            const int pk = sh.gm.pk[0];
            if (GM_QAC(pk)) {
                bits = sh.gm.base;
#pragma unroll
                for (int k = 0; k <= NN; k++)
                    if (sym[k] != -1) {
                        const int qi = v[k] == ypos ? (int) sh.pool.y_index : (k < NN ? (int) mp.kq[k] : ev.qc);
                        bits -= gm_m0(sh, qi); bits += gm_m1(qi);
                    }
            } else if (pk == FC_PK_UNIFORM) {
                bits = sh.gm.base;
#pragma unroll
                for (int k = 0; k <= NN; k++)
                    if (sym[k] != -1) bits = (float) ((double) bits - sh.gm.lg1);
            } else if (pk == FC_PK_CONSTANT) bits = 0;
        }
#endif
        ev.m_bits = bits;
    }
    nov[NN] = den; ipio[NN] = num;
#pragma unroll
    for (int k = 0; k <= NN; k++)
#pragma unroll
        for (int l = 0; l <= NN; l++)
            if (l > k) r[k] += ipd[l][k] * r[l] / nov[k];
    float m_err = mp.norm;
#pragma unroll
    for (int k = 0; k <= NN; k++) m_err += r[k] * r[k] * nov[k] - 2 * r[k] * ipio[k];
    ev.m_err = m_err;
    ev.costs = (ev.m_bits + ev.w_bits + mp.ab) * mp.price + m_err;
#pragma unroll
    for (int k = 0; k < MAXED; k++) ev.f[k] = k <= NN ? f[k] : 0.0f;
}

/* MAXN = largest step number the caller can reach (max_elements - 1): the unreachable
 * instantiations are not generated, the hot scan stays small in the instruction cache */
template <int MAXN>
__device__ __forceinline__ void full_eval(const DevFrame &F, const Sh &sh, const MPState &mp, const double *lglv,
                                          int n, int d, int state,
                                          float num, float den, float ip0, float ip1, float ip2,
                                          float ip3, Eval &ev)
{
    if (n == 0) full_eval_n<0>(F, sh, mp, lglv, d, state, num, den, ip0, ip1, ip2, ip3, ev);
    else if (n == 1 && MAXN >= 1) full_eval_n<(MAXN >= 1 ? 1 : 0)>(F, sh, mp, lglv, d, state, num, den, ip0, ip1, ip2, ip3, ev);
    else if (n == 2 && MAXN >= 2) full_eval_n<(MAXN >= 2 ? 2 : 0)>(F, sh, mp, lglv, d, state, num, den, ip0, ip1, ip2, ip3, ev);
    else if (n == 3 && MAXN >= 3) full_eval_n<(MAXN >= 3 ? 3 : 0)>(F, sh, mp, lglv, d, state, num, den, ip0, ip1, ip2, ip3, ev);
    else if (MAXN >= 4) full_eval_n<(MAXN >= 4 ? 4 : 0)>(F, sh, mp, lglv, d, state, num, den, ip0, ip1, ip2, ip3, ev);
}

/* log2 tables of the two coefficient contexts and of the edge-count model, and -- default build --
 * everything else of a call's set-up that is a function of the models alone.
 *
 * Pass 1, every lane the SAME code (divergent branches of a wave run one after the other: seven
 * different log2 call sites in one wave cost seven logarithms of time): lane t takes a (numerator,
 * denominator) pair by its role, evaluates log2((double) (num / (float) den)) and stores it where
 * the role says:
 *     t < dcs             lgdc[t]          DC symbols          om .. om + MAXED     Ltab[]  edge counts
 *     64 .. 64 + sy       lglv[]           symbols of the level's context
 *     om + 6              lglv_m1          (see below)
 *     om + 7, om + 8      tb[]             tree model: leaf / child of this level (default build)
 *     om + 9, om + 10     mp.wb_nd, wb_dc  placeholder weight 0.5 on no kept vector (default build)
 * (om = 64 + sy, or 128 when that would reach into the third wave; the mapping itself is mp_role(), mp_roles.h).
 * Pass 2, after a barrier, lane om + 11: the nested domain-0 model and -- default build -- the position
 * pricing of the first step (no kept vector), which mp_step_prepare() would otherwise compute on
 * the serial lane.
 * Out of line where machine LICM runs: the double constants of log2 stay inside (inlined, they are materialised
 * once before the kernel's persistent loop and occupy registers for the whole kernel).  The builds compiled without
 * machine LICM (csrc/Makefile KFLAGS: the ones with FC_SERIAL_LOOP) inline it: a call waits for every memory read in
 * flight, and op_approx has the first reads of the scan in flight across the table pass. */
#if defined(FC_SERIAL_LOOP) && FC_SERIAL_LOOP && !FC_HM
#define MP_TABLES_INLINE 1
#define MP_TABLES_ATTR __forceinline__
#else
#define MP_TABLES_INLINE 0
#define MP_TABLES_ATTR __noinline__
#endif
#if FC_HM
/* the same for models of up to 512 symbols per context (more roles than lanes): lane t takes the roles t,
 * t + B, ... -- DC symbols, the level's symbols, lglv_m1, the edge counts */
__device__ __noinline__ void mp_tables(const DevFrame &F, Sh &sh, int level, int y)
{
    const int tid = threadIdx.x;
    const int ctx = level - sh.par.lc_min_opt, dcs = sh.par.dcs, sy = sh.par.sy;
    const int nrole = dcs + sy + MAXED + 2;
    for (int t = tid; t < nrole; t += B) {
        const int r = t - dcs - sy;                /* 0: lglv_m1 (see below), 1 ..: edge counts */
        int ci, ti = 0;
        const bool coeff = r <= 0;
        if (t < dcs) ci = t;
        else if (r < 0) { ci = dcs + ctx * sy + t - dcs; ti = ctx + 1; }
        else if (r == 0) { ci = dcs + ctx * sy - 1; ti = ctx + 1; }
        else ci = r - 1;
        const float num = coeff ? (float) sh.cb.cnt[ci] : (float) sh.pool.count[ci];
        const float den = coeff ? (float) sh.cb.tot[ti] : (float) sh.pool.total;
        const double lg = log2((double) (num / den));
        if (t < dcs) sh.lgdc[t] = lg;
        else if (r < 0) sh.lglv[t - dcs] = lg;
        else if (r == 0) sh.lglv_m1 = lg;
        else sh.Ltab[ci] = (float) -lg;
    }
    __syncthreads();
    if (tid == 0) {
        const Pool &m = sh.pool;
        float q0 = 0, q1;
        if (m.d0_n && y != 0) q0 += sh.m0tab[qac_shift(m.d0_index)];
        if (y >= 0) q0 += sh.m0tab[qac_shift(m.d0_yindex)];
        q1 = q0;
        if (y == 0) { q1 -= sh.m0tab[qac_shift(m.d0_yindex)]; q1 += (float) qac_shift(m.d0_yindex); }
        else        { q1 -= sh.m0tab[qac_shift(m.d0_index)];  q1 += (float) qac_shift(m.d0_index); }
        sh.Q0 = q0; sh.Q1 = q1;
#if FC_GM
        {   /* what the candidates of this call have in common: the price of the empty list */
            const int k = sh.gm.pk[0];
            sh.gm.base = 0.0f;
            if (GM_QAC(k)) {                        /* qac_bits, codec/domain-pool.c:364-402, without `used' */
                const int16_t *q = GQ_CUR(sh, 0), *list = F.pool_states;
                float bits = 0;
                for (int e = 0; e < (int) m.n; e++)
                    if (list[e] != y) bits += gm_m0(sh, q[e]);
                if (y >= 0) bits += gm_m0(sh, m.y_index);
                sh.gm.base = bits;
            } else if (k == FC_PK_UNIFORM) {
                /* uniform_bits :592-615: `- n * log2 (..)' negates the UNSIGNED n first (reproduced, not repaired);
                 * log2 of the float quotient as the host's libm gives it (log2_host), log2 (1.0 / n) from the host's table */
                const unsigned nn = m.n;
                sh.gm.base = (float) ((double) (0u - nn) * log2_host(sh, (float) (nn - 1) / (float) nn));
                sh.gm.lg1 = F.lginv[nn];
            }
        }
#endif
    }
}
#else
__device__ MP_TABLES_ATTR void mp_tables(const DevFrame &F, Sh &sh, int level, int y)
{
    const int tid = threadIdx.x;
    const int ctx = level - sh.par.lc_min_opt, dcs = sh.par.dcs, sy = sh.par.sy;
    /* everything uniform the role pass needs is asked for here, in one LDS round trip */
    const int band = sh.band, half_nd = sh.par.half_nd, half_dc = sh.par.half_dc;
#if !FC_VARIANT_BIG
    const int ML = sh.par.ML;
#endif
    /* The roles are packed into as few waves as they fit (a wave without a role skips the logarithm
     * altogether, ~250 instructions per call and wave): DC symbols in wave 0, the level's symbols from
     * lane 64 on, the eleven single roles right behind them when that still ends in wave 1 (CLI models:
     * 64 + 16 + 11 lanes, waves 2 and 3 go straight to the barrier), else from lane 128 on. */
    const int om = 64 + sy + 12 <= 128 ? 64 + sy : 128;          /* uniform: first lane of the single roles */
    /* The nested domain-0 prices and the integer part of a first step's position pricing do not depend on the
     * logarithms: a lane of a wave WITHOUT a role (waves 2.. when the roles end in wave 1) works them out while the
     * others are in log2().  What needs the list prices -- three sums -- is left to lane 0's set-up of the call
     * (op_approx), which runs behind the caller's barrier anyway: no barrier and no single-lane tail in here. */
    const int sl = (om + 12 <= 128 && B > 128) ? 128 : om + 11;
    if (tid == sl) {
        /* nested domain-0 model with the usable luminance state y or -1
         * (domain-pool.c:367-402,773-782) */
        const Pool &m = sh.pool;
        float q0 = 0, q1;
        if (m.d0_n && y != 0) q0 += sh.m0tab[qac_shift(m.d0_index)];
        if (y >= 0) q0 += sh.m0tab[qac_shift(m.d0_yindex)];
        q1 = q0;
        if (y == 0) { q1 -= sh.m0tab[qac_shift(m.d0_yindex)]; q1 += (float) qac_shift(m.d0_yindex); }
        else        { q1 -= sh.m0tab[qac_shift(m.d0_index)];  q1 += (float) qac_shift(m.d0_index); }
        sh.Q0 = q0; sh.Q1 = q1;
#if !FC_VARIANT_BIG
        if (!band) {
            /* The first step of the call has no kept vector: what mp_step_prepare() would leave
             * for it depends on the models and the dictionary size only. */
            MPState &mp = sh.mp;
            const unsigned N = (unsigned) sh.pool.n;          /* mp.N of a luminance call */
            mp.s1_last[0] = 1;
            const unsigned mv = N - 2u;
            if (mv != 0) {
                const unsigned kk = 31u - (unsigned) __clz((int) (mv + 1));
                const unsigned r = (mv + 1) - (1u << kk);
                mp.s1_cd = 1u; mp.s1_k[0] = (int) kk; mp.s1_thr[0] = (int) (mv + 1 - 2 * r);
            } else {
                mp.s1_cd = 0u; mp.s1_k[0] = 0; mp.s1_thr[0] = 0;
            }
            mp.s1_has = 0u;
            mp.np = 0;
        }
#endif
    }
    if (tid < om + 12) {
        /* The role as selects (mp_roles.h), then one path for every role: each operand a role can ask for is read
         * whatever the lane's role is (at index 0 where it has none), so the LDS reads are in flight together and
         * a wave that holds several kinds of roles does not walk through one branch -- and one dependent LDS round
         * trip -- per kind.  Each count is converted in its own type, as the reference's float casts do. */
        const MpRole ro = mp_role(tid, dcs, sy, ctx, band, half_nd, half_dc, MAXED, FC_VARIANT_BIG);
        const bool kc = ro.kind == MPR_COEFF, kp = ro.kind == MPR_POOL;
        int pi = 0;                                /* cb.cnt[] holds every index a role gives, pool.count[] only a pool role's */
        pi = kp ? ro.ci : pi;
        const short c_num = sh.cb.cnt[ro.ci], c_den = sh.cb.tot[ro.ti], p_num = sh.pool.count[pi];
        const unsigned short p_den = sh.pool.total;
        const float c_numf = (float) c_num, c_denf = (float) c_den, p_numf = (float) p_num, p_denf = (float) p_den;
        float num = 1.0f, den = 1.0f;
        num = kp ? p_numf : num;   den = kp ? p_denf : den;
        num = kc ? c_numf : num;   den = kc ? c_denf : den;
#if !FC_VARIANT_BIG
        {   /* tree_bits_dev(): prob = counts[level] / (float) total */
            const bool kt = ro.kind == MPR_TREE;
            const float t_numf = (float) sh.tm[level], t_denf = (float) sh.tm[ML + level];
            num = kt ? t_numf : num;   den = kt ? t_denf : den;
        }
#endif
        float p = num / den;
        const float q = 1 - p;
        p = ro.leaf ? q : p;                       /* the leaf symbol */
        const double lg = log2((double) p);        /* one call site for every role */
        const float nlg = (float) -lg;
        /* A weight left over from another run of the same call (full_search, codec/approx.c:439-446) may round to
         * zero in this context's format: rtob() is then RPF_ZERO = -1 and the reference prices it with the counter
         * in FRONT of the context (coeff.c:228), the last symbol of the previous context: lglv_m1. */
        double *const d_dc = &sh.lgdc[ro.di], *const d_lv = &sh.lglv[ro.di], *const d_m1 = &sh.lglv_m1;
        float *const f_lt = &sh.Ltab[ro.di], *const f_tb = &sh.tb[ro.di];
        const bool to_dc = ro.dest == MPD_LGDC, to_lv = ro.dest == MPD_LGLV, to_m1 = ro.dest == MPD_LGLV_M1;
        const bool to_lt = ro.dest == MPD_LTAB, to_tb = ro.dest == MPD_TB;
        double *dd = &sh.sink_d;
        float *df = &sh.sink_f;
        dd = to_dc ? d_dc : dd;   dd = to_lv ? d_lv : dd;   dd = to_m1 ? d_m1 : dd;
        df = to_lt ? f_lt : df;   df = to_tb ? f_tb : df;
        *dd = lg;
        *df = nlg;
#if !FC_VARIANT_BIG
        if (ro.dest == MPD_WB_ND || ro.dest == MPD_WB_DC) {
            const float wb = sub_log2(sh, 0.0f, lg, ro.ci, ro.ti);
            if (ro.dest == MPD_WB_ND) sh.mp.wb_nd = wb; else sh.mp.wb_dc = wb;
        }
#endif
    }
}

#endif

/* serial part of a step start: sorted list of kept vectors, the two stage-1 weight prices */
__device__ void mp_step_prepare(const DevFrame &F, Sh &sh, MPState &mp, const double *lglv, double lglv_m1)
{
    float wb = 0;
    int np = 0;
    for (int k = 0; k < mp.n; k++)
        if (mp.weight[k] != 0) {
            const bool have = SYMP_HAS(mp.symp, k);
            if (mp.into[k]) {
                const int sym = have ? SYMP_GET(mp.symp, k) : rtob_dev(mp.weight[k], sh.par.rpf_mant, sh.par.rpf_range);
                {
                    const int ctx = mp.level - sh.par.lc_min_opt;
                    wb = sub_log2(sh, wb, sym >= 0 ? lglv[sym] : lglv_m1, sh.par.dcs + ctx * sh.par.sy + sym, ctx + 1);
                }
            }
            else {
                /* RPF_ZERO in the DC context reads in FRONT of the reference's counter array
                 * (coeff.c:228 with index -1): undefined there; with glibc that is the upper
                 * half of the malloc chunk header, i.e. a count of 0 -> log2(0) = -inf -> the
                 * kept vectors cost +inf bits and no candidate of the step passes stage 1.
                 * The oracle (same allocator) and this code do the same. */
                const int sym = have ? SYMP_GET(mp.symp, k) : rtob_dev(mp.weight[k], sh.par.dc_mant, sh.par.dc_range);
                wb = sym >= 0 ? sub_log2(sh, wb, sh.lgdc[sym], sym, 0)
                              : (float) ((double) wb + (double) INFINITY);
            }
            if (mp.indices[k] == mp.ypos) continue;
            int j = np++;
            while (j > 0 && mp.psorted[j - 1] > mp.indices[k]) { mp.psorted[j] = mp.psorted[j - 1]; j--; }
            mp.psorted[j] = mp.indices[k];
        }
    mp.np = np;
    {   /* uniform parts of the stage-1 position pricing, see StepCtx */
        const unsigned N = (unsigned) mp.N;
        const short *p = mp.psorted;
        const bool p0zero = np > 0 && p[0] == 0;
        float e[MAXED];
        bool  ev[MAXED];
        for (int j = 0; j < np; j++) {
            if (j == 0) {
                ev[0] = p[0] != 0 && (N - 2) != 0;
                e[0] = ev[0] ? (float) bits_bin_code((unsigned) p[0] - 1, N - 2) : 0.0f;
            } else {
                ev[j] = (unsigned) p[j - 1] != N - 2;
                e[j] = ev[j] ? (float) bits_bin_code((unsigned) (p[j] - p[j - 1] - 1), N - 2 - (unsigned) p[j - 1]) : 0.0f;
            }
        }
        float b = sh.Ltab[np + 1];
        b += p0zero ? sh.Q1 : sh.Q0;
        unsigned cd = 0, has = 0;
        for (int i = 0; i <= np; i++) {
            mp.s1_pre[i] = b;
            unsigned last = i == 0 ? 1u : (unsigned) p[i - 1] + 1;
            unsigned mv = N - 1 - last;
            mp.s1_last[i] = (int) last;
            if (mv != 0) {
                unsigned kk = 31u - (unsigned) __clz((int) (mv + 1));
                unsigned r = (mv + 1) - (1u << kk);
                cd |= 1u << i;
                mp.s1_k[i] = (int) kk; mp.s1_thr[i] = (int) (mv + 1 - 2 * r);
            } else {
                mp.s1_k[i] = 0; mp.s1_thr[i] = 0;
            }
            if (i < np && ev[i]) b += e[i];
        }
        for (int j = 1; j < np; j++) { mp.s1_sfx[j] = e[j]; if (ev[j]) has |= 1u << j; }
        mp.s1_cd = cd; mp.s1_has = has;
        b = sh.Ltab[np + 1]; b += sh.Q1;
        for (int j = 0; j < np; j++) if (ev[j]) b += e[j];
        mp.s1_z0 = b;
        b = sh.Ltab[np]; b += p0zero ? sh.Q1 : sh.Q0;
        for (int j = 0; j < np; j++) if (ev[j]) b += e[j];
        mp.s1_zy = b;
    }
    {
        const int ctx = mp.level - sh.par.lc_min_opt;
        const int s_nd = sh.par.half_nd, s_dc = sh.par.half_dc;      /* rtob(0.5): constants of the model set (Sh::par) */
        mp.wb_nd = sub_log2(sh, wb, lglv[s_nd], sh.par.dcs + ctx * sh.par.sy + s_nd, ctx + 1);
        mp.wb_dc = sub_log2(sh, wb, sh.lgdc[s_dc], s_dc, 0);
    }
#if FC_GM
    {
        /* stage 1 prices {kept vectors with a non-zero weight (selection order), candidate} (codec/approx.c:433-458):
         * the part of the kept vectors once per step */
        const int k = sh.gm.pk[0];
        float b = sh.gm.base;
        if (GM_QAC(k)) {
            for (int i = 0; i < mp.n; i++)
                if (mp.weight[i] != 0) {
                    if (mp.indices[i] == mp.ypos) { b -= gm_m0(sh, sh.pool.y_index); b += gm_m1(sh.pool.y_index); }
                    else { b -= gm_m0(sh, mp.kq[i]); b += gm_m1(mp.kq[i]); }
                }
        } else if (k == FC_PK_UNIFORM) {
            for (int i = 0; i < mp.n; i++)
                if (mp.weight[i] != 0) b = (float) ((double) b - sh.gm.lg1);
        }
        sh.gm.kept = b;
        if (sh.gm.ck[0] == FC_CK_UNIFORM) {          /* uniform_bits, codec/coeff.c:155-170: mantissa bits + 1 per weight */
            float w = 0;
            for (int i = 0; i < mp.n; i++)
                if (mp.weight[i] != 0) w += (float) ((mp.into[i] ? sh.par.rpf_mant : sh.par.dc_mant) + 1);
            mp.wb_nd = w; mp.wb_nd += (float) (sh.par.rpf_mant + 1);
            mp.wb_dc = w; mp.wb_dc += (float) (sh.par.dc_mant + 1);
        }
    }
#endif
#if FC_VARIANT_BIG
    mp.min_costs = F.full_search ? MAXCOSTS : mp.costs;     /* codec/approx.c:420 */
#else
    mp.min_costs = mp.costs;            /* full_search needs the big build */
#endif
}

/* rle_update + aac_update on acceptance (domain-pool.c:795-830, coeff.c:242-267) */
/* symp: the RPF symbols of weight[0..2] (MPState::symp) or SYMP_NONE */
__device__ void models_update(const DevFrame &F, Sh &sh, const short *indices, const short *into,
                              const float *weight, int level, int y, unsigned symp = SYMP_NONE)
{
    Pool &m = sh.pool;
    int state_0 = 0, state_y = 0, edge = 0;
#if FC_GM
    if (GM_QAC(sh.gm.pk[0])) {
        /* qac_update, codec/domain-pool.c:404-446: every index + 1; a used domain: - 1 and halved; clamp at 1020.
         * The used ones first from their old values, the rest 16 bytes at a time. */
        int16_t *q = GQ_CUR(sh, 0);
        const int16_t *list = F.pool_states;
        int used_y = 0, y_is_domain = y >= 0 && F.pos[y] >= 0 && F.pos[y] < (int) m.n;
        short nv[MAXED + 1], np_[MAXED + 1];
        int nu = 0;
        for (int e = 0; indices[e] != NOEDGE; e++) {
            const int p = indices[e];
            if (into[e] == y && y >= 0) {
                if (y_is_domain) { np_[nu] = (short) p; nv[nu] = q[p]; nu++; }      /* + 1 - 1 */
                m.y_index >>= 1;
                used_y = 1;
            } else { np_[nu] = (short) p; nv[nu] = (short) (q[p] >> 1); nu++; }      /* (+ 1 - 1) >> 1 */
        }
        (void) list;
        for (int i = 0; i < ((int) m.n + 7) / 8; i++) {
            uint4 v = ((uint4 *) q)[i];
            unsigned *w = (unsigned *) &v;
            for (int j = 0; j < 4; j++) {
                unsigned lo = (w[j] & 0xffffu) + 1, hi = (w[j] >> 16) + 1;
                if (lo > 1020) lo = 1020;
                if (hi > 1020) hi = 1020;
                w[j] = lo | (hi << 16);
            }
            ((uint4 *) q)[i] = v;
        }
        for (int i = 0; i < nu; i++) q[np_[i]] = nv[i] > 1020 ? (short) 1020 : nv[i];
        if (y >= 0 && !used_y) m.y_index++;
        if (m.y_index > 1020) m.y_index = 1020;
    } else if (!GM_RLE(sh.gm.pk[0])) {
        /* default_update: the constant and the uniform pool have no model */
    } else {
#endif
    for (; indices[edge] != NOEDGE; edge++) {
        if (into[edge] == 0) state_0 = 1;
        else if (into[edge] == y) state_y = 1;
    }
    m.count[edge]++;
    m.total++;
    {   /* nested domain-0 model (qac_update, domain-pool.c:404-446) */
        int used_y = 0, y_is_domain = 0;
        if (m.d0_n) { m.d0_index++; if (y == 0) y_is_domain = 1; }
        if (state_0) {
            if (y == 0) { if (y_is_domain) m.d0_index--; m.d0_yindex >>= 1; used_y = 1; }
            else { m.d0_index--; m.d0_index >>= 1; }
        }
        if (y >= 0 && !used_y) m.d0_yindex++;
        if (m.d0_n && m.d0_index > 1020) m.d0_index = 1020;
        if (m.d0_yindex > 1020) m.d0_yindex = 1020;
    }
    if (state_y) m.y_index >>= 1; else m.y_index++;
    if (m.y_index > 1020) m.y_index = 1020;
#if FC_GM
    }
    if (sh.gm.ck[0] == FC_CK_UNIFORM) return;       /* uniform_update: nothing */
#endif
    int ctx = level - sh.par.lc_min_opt;
    for (int e = 0; into[e] != NOEDGE; e++) {
        const bool have = SYMP_HAS(symp, e);
        if (into[e]) {
            sh.cb.cnt[sh.par.dcs + ctx * sh.par.sy + (have ? SYMP_GET(symp, e) : rtob_dev(weight[e], sh.par.rpf_mant, sh.par.rpf_range))]++;
            sh.cb.tot[ctx + 1]++;
        } else {
            sh.cb.cnt[have ? SYMP_GET(symp, e) : rtob_dev(weight[e], sh.par.dc_mant, sh.par.dc_range)]++;
            sh.cb.tot[0]++;
        }
    }
}

/* minimum over the 64 lanes of a wave on the DPP path (no LDS crossbar): inclusive min-scan
 * inside each row of 16 lanes (row_shr 1,2,4,8: a lane without a source keeps its value), row 0/2
 * totals into rows 1/3 (row_bcast15), rows 0-1 total into rows 2-3 (row_bcast31); LANE 63 then
 * holds the wave minimum.  One v_min_f32 with a DPP source per step (written out: the builtin
 * form costs a constant move, a DPP move, a canonicalisation and the min -- four VALU issues a
 * step, twelve times per scan pass); s_nop 1 = the two wait states between a VALU write and a
 * DPP read of the same register. */
__device__ __forceinline__ float wave_min_l63(float v)
{
    asm volatile(
        "s_nop 1\n\t"
        "v_min_f32_dpp %0, %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_f32_dpp %0, %0, %0 row_shr:2 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_f32_dpp %0, %0, %0 row_shr:4 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_f32_dpp %0, %0, %0 row_shr:8 row_mask:0xf bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
        "s_nop 1\n\t"
        "v_min_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
        "s_nop 1"
        : "+v"(v));
    return v;
}

/* four independent minima at once: the four DPP chains are interleaved, so the two wait states
 * between a VALU write and a DPP read of the same register are filled by the other chains (no
 * s_nop between the steps) */
__device__ __forceinline__ void wave_min4_l63(float &a, float &b, float &c, float &d)
{
#define MIN4_STEP(ctl)                                                     \
        "v_min_f32_dpp %0, %0, %0 " ctl "\n\t"                             \
        "v_min_f32_dpp %1, %1, %1 " ctl "\n\t"                             \
        "v_min_f32_dpp %2, %2, %2 " ctl "\n\t"                             \
        "v_min_f32_dpp %3, %3, %3 " ctl "\n\t"
    asm volatile(
        "s_nop 1\n\t"
        MIN4_STEP("row_shr:1 row_mask:0xf bank_mask:0xf")
        MIN4_STEP("row_shr:2 row_mask:0xf bank_mask:0xf")
        MIN4_STEP("row_shr:4 row_mask:0xf bank_mask:0xf")
        MIN4_STEP("row_shr:8 row_mask:0xf bank_mask:0xf")
        MIN4_STEP("row_bcast:15 row_mask:0xa bank_mask:0xf")
        MIN4_STEP("row_bcast:31 row_mask:0xc bank_mask:0xf")
        "s_nop 1"
        : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
#undef MIN4_STEP
}

__device__ __forceinline__ float wave_min(float v)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_min_l63(v)), 63));
}

#if FC_VARIANT_BIG
#define MP_NUMROW(F, mp)    ((mp).numrow)
/* codec/approx.c:376-377: the positions on the exclude list never become candidates */
__device__ __forceinline__ bool mp_excluded(const MPState &mp, int pos)
{
    bool x = false;
    bool live = true;
#pragma unroll
    for (int i = 0; i < MAXED; i++) {
        live = live && mp.excl[i] != NOEDGE;
        x = x || (live && mp.excl[i] == pos);
    }
    return x;
}
#define MP_EXCLUDED(mp, pos) mp_excluded(mp, pos)
#else
#define MP_NUMROW(F, mp)    (sh.par.ipis + (size_t) (mp).image * sh.par.P)
#define MP_EXCLUDED(mp, pos) false
#endif

/* Barrier for data that is exchanged through LDS only.  __syncthreads() also waits for every
 * outstanding global load of the wave (vmcnt(0)): table reads requested early -- the Gram row of
 * the vector a step has just chosen, the first rows of a call -- would be waited for at the next
 * barrier instead of where they are used.  The hardware barrier itself does not drain them. */
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

#include "mp_step.inc"                /* what every scan does with a candidate: accept rule, record, commit, update */
#include "mp_reg.inc"                 /* register-resident scan and the chroma list scan */

/* general scan: per-candidate scratch in HBM (any number of states, up to MAXEDGES vectors).
 * Out of line on purpose: it is the cold variant (frames with more than KREG*B states or
 * more than 3 vectors) and must not sit between the hot loops in the instruction cache. */
__device__ __noinline__ void mp_steps_global(DevFrame &F, Sh &sh, int q, float size)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = F.P;
    MPState &mp = sh.mp;
    const int S = sh.states;
    const int nblk = (S + 63) >> 6;
    constexpr int U = 4;                 /* candidates per lane per pass: loads of all U in flight */
    unsigned long long tA = 0, tB = 0, tmark = wall_clock64();
    unsigned blockevals = 0;
    for (;;) {
        const int n = mp.n;
        /* ---------------- phase A: Gram-Schmidt update + stage-1 estimate ---------------- */
        {
            const float *Gq = GRAM(F, q);
            const int flim = sh.flim;
            const float *diag = F.diag + (size_t) q * P;
            const float *numrow = MP_NUMROW(F, mp);
            const int nv = n - 1;
            StepCtx ctx;
            load_step_ctx(mp, ctx);
            float novk[MAXED - 1], selk[MAXED - 1], nov_nv = 1, ipio_nv = 0;
#pragma unroll
            for (int k = 0; k < MAXED - 1; k++) {
                novk[k] = k < nv ? mp.norm_ov[k] : 1.0f;
                selk[k] = k < nv ? mp.sel_ipdo[nv < 0 ? 0 : nv][k] : 0.0f;
            }
            if (n) { nov_nv = mp.norm_ov[nv]; ipio_nv = mp.ipio[nv]; }
            for (int base = 0; base < nblk * 64; base += B * U) {
                int dd[U], ps[U];
                bool in[U], us[U];
                float num[U], den[U], g[U], ip[U][MAXED - 1], e[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    dd[u] = base + u * B + tid;
                    ps[u] = dd[u] < S && !DEAD(sh, dd[u]) ? (int) F.pos[dd[u]] : -1;
                    in[u] = ps[u] >= 0;
                    us[u] = (in[u] && n) ? F.used[dd[u]] != 0 : !in[u];
                }
                if (n == 0) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        den[u] = in[u] ? diag[dd[u]] : 1.0f;
                        num[u] = in[u] ? numrow[dd[u]] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (!in[u]) continue;
                        bool uu = den[u] / size < MIN_NORM;
                        if (!uu) uu = fabsf(num[u]) < MIN_NORM;
                        if (MP_EXCLUDED(mp, ps[u])) uu = true;
                        us[u] = uu;
                        F.num[dd[u]] = num[u]; F.den[dd[u]] = den[u]; F.used[dd[u]] = uu;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        bool on = !us[u];
                        num[u] = on ? F.num[dd[u]] : 0.0f;
                        den[u] = on ? F.den[dd[u]] : 1.0f;
                        g[u] = on ? gram_load(Gq, P, mp.row_state, dd[u], flim) : 0.0f;
#pragma unroll
                        for (int k = 0; k < MAXED - 1; k++)
                            ip[u][k] = (on && k < nv) ? F.ipdo[(size_t) k * P + dd[u]] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        if (us[u]) continue;
                        const float t = mp_orthogonalize<MAXED - 1>(g[u], ip[u], novk, selk, nv, nov_nv, ipio_nv, num[u], den[u]);
                        F.ipdo[(size_t) nv * P + dd[u]] = t;
                        if (den[u] / size < MIN_NORM) { us[u] = true; F.used[dd[u]] = 1; }
                        F.num[dd[u]] = num[u]; F.den[dd[u]] = den[u];
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    e[u] = BIGF;
                    if (in[u] && !us[u]) e[u] = stage1<MAXED - 1>(ctx, ps[u], dd[u], num[u], den[u]);
                    if (dd[u] < S) F.est[dd[u]] = e[u];
                    float bm = wave_min(e[u]);
                    int blk = ((base + u * B) >> 6) + wave;
                    if (lane == 0 && blk < NBLOCKMIN) sh.blockmin[blk] = bm;
                }
            }
        }
        __syncthreads();
        if (tid == 0) { unsigned long long t = wall_clock64(); tA += t - tmark; tmark = t; }
        /* ------- phase B: ordered replay + commit of the step, all inside wave 0 ------- */
        if (wave == 0) mp_replay_hbm<false>(F, sh, n, S, blockevals);
        __syncthreads();
        if (tid == 0) { unsigned long long t = wall_clock64(); tB += t - tmark; tmark = t; }
        if (!(mp.n < F.max_elements && mp.index >= 0)) break;
    }
    if (tid == 0) { sh.cnt.t_mpA += tA; sh.cnt.t_mpB += tB; sh.cnt.n_blockevals += blockevals; }
}

#if FC_VARIANT_BIG
/* The general scan over an explicit candidate LIST of any length: the chroma bands with a dictionary of more than
 * 63 states (cfiasco --chroma-dictionary 64 ..; codec/domain-pool.c:707-735,854-879).  Candidate c = list position
 * c, state = list[c] (F.pool_states: the states rle_chroma kept, ascending, + the co-located luminance state);
 * tables are read by state, the scratch of mp_steps_global (num, den, est, ipdo, used) is indexed by position. */
__device__ __noinline__ void mp_steps_list_global(DevFrame &F, Sh &sh, int q, float size, int D)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, P = F.P;
    MPState &mp = sh.mp;
    const int16_t *const list = F.pool_states;
    const int nblk = (D + 63) >> 6;
    unsigned blockevals = 0;
    for (;;) {
        const int n = mp.n;
        {
            const float *Gq = GRAM(F, q);
            const int flim = sh.flim;
            const float *diag = F.diag + (size_t) q * P;
            const float *numrow = MP_NUMROW(F, mp);
            const int nv = n - 1;
            StepCtx ctx;
            load_step_ctx(mp, ctx);
            for (int base = 0; base < nblk * 64; base += B) {
                const int c = base + tid;
                const bool in = c < D;
                const int st = in ? (int) list[c] : 0;
                bool us = in ? (n ? F.used[c] != 0 : false) : true;
                float num = 0.0f, den = 1.0f;
                if (in && n == 0) {                                   /* codec/approx.c:360-377 */
                    den = diag[st]; num = numrow[st];
                    bool uu = den / size < MIN_NORM;
                    if (!uu) uu = fabsf(num) < MIN_NORM;
                    if (MP_EXCLUDED(mp, c)) uu = true;
                    us = uu;
                    F.num[c] = num; F.den[c] = den; F.used[c] = uu;
                } else if (!us) {                                     /* codec/approx.c:676-698 */
                    num = F.num[c]; den = F.den[c];
                    float ip[MAXED - 1];
#pragma unroll
                    for (int k = 0; k < MAXED - 1; k++) ip[k] = k < nv ? F.ipdo[(size_t) k * P + c] : 0.0f;
                    const float t = mp_orthogonalize<MAXED - 1>(gram_load(Gq, P, mp.row_state, st, flim), ip, mp.norm_ov,
                                                                mp.sel_ipdo[nv], nv, mp.norm_ov[nv], mp.ipio[nv], num, den);
                    F.ipdo[(size_t) nv * P + c] = t;
                    if (den / size < MIN_NORM) { us = true; F.used[c] = 1; }
                    F.num[c] = num; F.den[c] = den;
                }
                float e = BIGF;
#if FC_GM
                if (in && !us && !GM_RLE(sh.gm.pk[0])) {
                    /* codec/approx.c:433-462 with the pool's own ->bits: the kept vectors' part is sh.gm.kept */
                    const int pk = sh.gm.pk[0];
                    float bits = sh.gm.kept;
                    if (GM_QAC(pk)) {
                        const int qi = c == mp.ypos ? (int) sh.pool.y_index : (int) GQ_CUR(sh, 0)[c < (int) sh.pool.n ? c : 0];
                        bits -= gm_m0(sh, qi); bits += gm_m1(qi);
                    } else if (pk == FC_PK_UNIFORM) bits = (float) ((double) bits - sh.gm.lg1);
                    else bits = 0;
                    const float wbits = st ? ctx.wb_nd : ctx.wb_dc;
                    e = (bits + wbits + ctx.ab) * ctx.price + ctx.err - num * num / den;
                } else
#endif
                if (in && !us) e = stage1<MAXED - 1>(ctx, c, st, num, den);
                if (in) F.est[c] = e;
                const float bm = wave_min(e);
                const int blk = (base >> 6) + wave;
                if (lane == 0 && blk < NBLOCKMIN) sh.blockmin[blk] = bm;
            }
        }
        __syncthreads();
        if (wave == 0) mp_replay_hbm<true>(F, sh, n, D, blockevals);
        __syncthreads();
        if (!(mp.n < F.max_elements && mp.index >= 0)) break;
    }
    if (tid == 0) sh.cnt.n_blockevals += blockevals;
}
#endif

__device__ __noinline__ void mp_steps_chroma(DevFrame &F, Sh &sh, int q, float size, int D)
{
#if FC_VARIANT_BIG
    if (F.chroma_max > 63) { mp_steps_list_global(F, sh, q, size, D); return; }
#endif
    mp_steps_list<MAXED - 1>(F, sh, q, size, D);
}

/* approximate_range (codec/approx.c:74-271): one matching pursuit, plus in the big variant further ones without vectors
 * of the first (:103-206).  op_approx() at the end is the sequence of the steps below.  What a build does differently is
 * said once, in the step it belongs to, as two whole definitions: FC_GM first, then FC_VARIANT_BIG against the default. */
#ifdef FC_SERIAL_PROFILE
#define APX_CLOCK() unsigned long long tp = wall_clock64()
#define APX_MARK(i) do { if (tid == 0) { unsigned long long t_ = wall_clock64(); sh.tk_apx[i] += t_ - tp; tp = t_; } } while (0)
#else
#define APX_CLOCK() do { } while (0)
#define APX_MARK(i) do { } while (0)
#endif

/* Candidates are walked by STATE id (scratch, diag, Gram row, numerators are all state indexed, so every load of
 * phase A is direct and coalesced); pos[] gives the position in the pool list that the rate model needs, -1 for states
 * outside the pool.  State order == position order, so the 64-state blocks keep the reference's scan order.
 * The register scan takes a luminance search whose states and vectors fit its slots (uniform). */
#define APX_REGSCAN(sh) (!(sh).band && (sh).states <= KREG * B && (sh).par.max_elements <= FC_NIP + 1)

#if FC_GM
/* uniform_generate / const_generate (codec/domain-pool.c:578-590,518-528) know no luminance state */
__device__ __forceinline__ bool gm_no_luma(const Sh &sh)
{
    return sh.gm.pk[0] == FC_PK_UNIFORM || sh.gm.pk[0] == FC_PK_CONSTANT;
}
/* set-up: the ->bits of the active pool for the empty list */
__device__ __forceinline__ float apx_empty_list_bits(const Sh &sh)
{
    if (!GM_RLE(sh.gm.pk[0])) return sh.gm.pk[0] == FC_PK_CONSTANT ? 0.0f : sh.gm.base;
    return sh.Ltab[0] + sh.Q0;
}
#else
__device__ __forceinline__ bool gm_no_luma(const Sh &sh) { return false; }
/* set-up: rle_bits of the empty list */
__device__ __forceinline__ float apx_empty_list_bits(const Sh &sh) { return sh.Ltab[0] + sh.Q0; }
#endif

#if FC_VARIANT_BIG
/* ---------------- the big builds ---------------- */

/* set-up: the range's inputs -- its norm, its row of <range, state> numerators, the bits it costs besides the
 * combination */
__device__ __forceinline__ void apx_range_inputs(const DevFrame &F, Sh &sh, SFrame &fr, int level)
{
    MPState &mp = sh.mp;
    const int P = sh.par.P;
    if (level > sh.par.images_level) {
        mp.norm = sh.norms[mp.image];
        mp.numrow = sh.par.ipis + (size_t) mp.image * P;
    } else {
        /* block not larger than a state image: direct dots (codec/ip.c:46-70,268-295),
         * tables d5 / d4 of the current pixel block; norm as codec/approx.c:388-389 */
        const int npx = 1 << level;
        const float *px = sh.pixels + mp.address * npx;
        float nrm = 0;
        for (int k = 0; k < npx; k++) nrm += px[k] * px[k];
        mp.norm = nrm;
        mp.numrow = (level == sh.par.images_level ? ACT_D5(F, sh) : ACT_D4(F, sh)) + (size_t) mp.address * P;
    }
    /* additional_bits, codec/approx.c:391-393 */
    mp.ab = fr.lrange.tree_bits + fr.lrange.mv_tree_bits + fr.lrange.mv_coord_bits + fr.lrange.nd_tree_bits
            + fr.lrange.nd_weights_bits;
}

/* The register scan: its first reads take the row of numerators that the set-up has chosen, so they are requested
 * here.  Then by (uniform) instance: a half / a quarter of the register slots hold every state (a frame starts
 * with a handful).  (The default builds keep ONE instance: a second one inlined beside it costs them more in spilled
 * registers -- 128 VGPRs, four frames per CU -- than the shorter slot loops save: 545 against 556 frames/s.) */
__device__ __forceinline__ void apx_steps_reg(DevFrame &F, Sh &sh, int q, float size, Step0 &pre)
{
    mp_step0_issue(sh, q, MP_NUMROW(F, sh.mp), pre);
    const int kslots = (sh.states + B - 1) / B;
    /* at most three vectors per block (the CLI's default, BASELINE config 5): the scan of the default builds --
     * one kept projection per register slot instead of three, shorter fixed-trip loops in the estimate */
    if (sh.par.max_elements <= 3) {
        if (kslots <= KREG / 4) mp_steps_reg<2, KREG / 4>(F, sh, q, size, pre);
        else if (kslots <= KREG / 2) mp_steps_reg<2, KREG / 2>(F, sh, q, size, pre);
        else mp_steps_reg<2>(F, sh, q, size, pre);
    } else if (kslots <= KREG / 4) mp_steps_reg<FC_NIP, KREG / 4>(F, sh, q, size, pre);
    else if (kslots <= KREG / 2) mp_steps_reg<FC_NIP, KREG / 2>(F, sh, q, size, pre);
    else mp_steps_reg<FC_NIP>(F, sh, q, size, pre);
}

/* Retries of approximate_range (codec/approx.c:103-206): second domain block, then removal of vectors whose weight
 * rounded to zero (underflow) or to the extreme value (overflow); sh.mp is the reference's working copy t, sh.mp_keep
 * its best result so far.  apx_retry_begin: does the frame ask for any; apx_retry_next, behind a search: keep the
 * better result and say whether another search follows (its exclude list is then in sh.mp). */
__device__ __forceinline__ bool apx_retry_begin(const DevFrame &F, Sh &sh)
{
    if (threadIdx.x == 0) {
        sh.apx_stage = 0; sh.apx_it = -1;
        sh.mp.excl[0] = NOEDGE;
        for (int k = 0; k < MAXED; k++) sh.mp.weight[k] = 0;     /* mp_t starts zeroed */
    }
    return F.second_domain_block || F.check_underflow || F.check_overflow;
}
__device__ __forceinline__ bool apx_retry_next(const DevFrame &F, Sh &sh, bool retries)
{
    if (!retries) return false;
    __syncthreads();
    if (threadIdx.x == 0) {
        MPState &mp = sh.mp, &best = sh.mp_keep;
        mp.indices[mp.best_n] = NOEDGE;                       /* codec/approx.c:636-640 */
        mp.costs = (mp.matrix_bits + mp.weights_bits + mp.ab) * mp.price + mp.err;
        if (sh.apx_stage == 0) best = mp;
        else if (mp.costs < best.costs) best = mp;            /* :114-115,146-147,196-197 */
        int more = 0;
        while (!more && sh.apx_stage < 4) {
            if (sh.apx_stage == 0) {                          /* second domain block, :103-118 */
                sh.apx_stage = 1;
                if (F.second_domain_block && (best.indices[0] != NOEDGE || F.full_search)) {
                    /* t = mp is what `mp` already holds.  Without a first vector the second
                     * search repeats the first -- except under full_search, where the
                     * weights left by the first run enter the stage-1 pricing of the second */
                    mp.excl[0] = best.indices[0]; mp.excl[1] = NOEDGE;
                    more = 1;
                }
            } else if (sh.apx_stage == 1 || sh.apx_stage == 2) {
                /* stage 1: underflow loop (:119-161), stage 2: overflow loop (:162-206) */
                const bool on = sh.apx_stage == 1 ? F.check_underflow != 0 : F.check_overflow != 0;
                if (!on) { sh.apx_stage++; sh.apx_it = -1; continue; }
                if (sh.apx_it < 0) mp = best;                 /* t = mp on entry */
                else if (!(sh.apx_it < MAXED - 1)) { sh.apx_stage++; sh.apx_it = -1; continue; }
                const int it = ++sh.apx_it;
                mp.excl[it] = NOEDGE;
                for (int i = 0; mp.indices[i] != NOEDGE; i++) {
                    bool hit;
                    if (sh.apx_stage == 1) hit = mp.weight[i] == 0;
                    else {
                        const int mant = mp.indices[i] ? sh.par.rpf_mant : sh.par.dc_mant;
                        const float range = mp.indices[i] ? sh.par.rpf_range : sh.par.dc_range;
                        hit = mp.weight[i] == btor_fast(rtob_dev(200.0f, mant, range), mant, range)
                              || mp.weight[i] == btor_fast(rtob_dev(-200.0f, mant, range), mant, range);
                    }
                    if (hit) { mp.excl[it] = mp.indices[i]; break; }
                }
                if (mp.excl[it] != NOEDGE) { mp.excl[it + 1] = NOEDGE; more = 1; }
                else { sh.apx_stage++; sh.apx_it = -1; }
            } else sh.apx_stage = 4;
        }
        if (!more) mp = best;
        sh.apx_more = more;
    }
    __syncthreads();
    return sh.apx_more;
}

#else
/* ---------------- the builds of the default geometry ---------------- */

/* set-up: the range's inputs -- its norm (its numerators are the image's row of the table, MP_NUMROW) and the bits
 * it costs besides the combination: the tree bits of this level, which mp_tables left in sh.tb */
__device__ __forceinline__ void apx_range_inputs(const DevFrame &F, Sh &sh, SFrame &fr, int level)
{
    sh.mp.norm = sh.norms[sh.mp.image];
    fr.lrange.tree_bits = sh.tb[0];
    sh.mp.ab = sh.tb[0];
}

__device__ __forceinline__ void apx_steps_reg(DevFrame &F, Sh &sh, int q, float size, Step0 &pre)
{
    mp_steps_reg<FC_NIP>(F, sh, q, size, pre);
}

/* no retries: full_search, second_domain_block and the weight checks need a big build */
__device__ __forceinline__ bool apx_retry_begin(const DevFrame &F, Sh &sh) { return false; }
__device__ __forceinline__ bool apx_retry_next(const DevFrame &F, Sh &sh, bool retries) { return false; }
#endif

/* Default builds: the first reads of the register scan depend on nothing the call computes.  They are requested in
 * front of the table pass and cross it and lane 0's set-up in flight (MP_TABLES_INLINE; a call of the out-of-line
 * mp_tables waits for them) */
__device__ __forceinline__ void apx_issue_early(const Sh &sh, const SFrame &fr, int q, bool regscan, Step0 &pre)
{
    /* vmcnt(0), as the call of the out-of-line mp_tables had it at this point: nothing an earlier operation requested
     * is in flight here, but the compiler cannot tell (the barrier at the head of the operation loop does not wait for
     * memory reads) and would otherwise wait for "them" -- in fact for the reads requested below -- in the middle of
     * the table pass and of the set-up, wherever it reuses a register such a read once went to */
    if (MP_TABLES_INLINE) __builtin_amdgcn_s_waitcnt(0x0f70);
    if (regscan) mp_step0_issue(sh, q, sh.par.ipis + (size_t) fr.lrange.image * sh.par.P, pre);
}

/* set-up, chroma: the list is the chroma pool (constant) plus the luminance state y unless present: y's position in
 * it, where it is appended if need be (mp.D grows); -1 without y */
__device__ __forceinline__ int apx_ypos(DevFrame &F, Sh &sh, int y, int D)
{
    int ypos = -1;
    if (y < 0 || gm_no_luma(sh)) return ypos;
    if (FC_VARIANT_BIG && (FC_GM || F.chroma_max > 63)) {    /* long list in F.pool_states; F.pos is its inverse */
        ypos = F.pos[y];                                     /* (op_chroma_pool) */
        if (ypos < 0 || ypos >= D) { F.pool_states[D] = (short) y; ypos = D; sh.mp.D = D + 1; }
    } else {                                                 /* at most 64, kept in sh.dl */
        for (int i = 0; i < D; i++) if (sh.dl[i] == y) ypos = i;
        if (ypos < 0) { sh.dl[D] = (short) y; ypos = D; sh.mp.D = D + 1; }
    }
    return ypos;
}

/* per-search set-up, lane 0: the call's state in sh.mp before the first step */
__device__ __forceinline__ void apx_setup(DevFrame &F, Sh &sh, SFrame &fr, int level, int y, int D)
{
    MPState &mp = sh.mp;
    mp.n = 0; mp.best_n = 0; mp.symp = SYMP_NONE;
    mp.D = D; mp.N = D;
    mp.y_state = y;
    mp.ypos = sh.band ? apx_ypos(F, sh, y, D) : -1;
    mp.level = level; mp.image = fr.lrange.image; mp.address = fr.lrange.address;
    apx_range_inputs(F, sh, fr, level);
    mp.price = fr.price;
    mp.err = mp.norm;
    mp.weights_bits = 0;
    mp.matrix_bits = apx_empty_list_bits(sh);
    mp.costs = (mp.matrix_bits + mp.weights_bits + mp.ab) * mp.price + mp.err;
    mp.index = -1;
    /* the prices of the first step.  A luminance search of a default build has no kept vector: mp_tables left the
     * integers, the three list prices are added up here.  (Big builds: weights of an earlier run may enter them.) */
    if (FC_VARIANT_BIG || sh.band) mp_step_prepare(F, sh, mp, sh.lglv, sh.lglv_m1);
    else {
        const float L0 = sh.Ltab[0], L1 = sh.Ltab[1], q0 = sh.Q0, q1 = sh.Q1;
        float b = L1; b += q0; mp.s1_pre[0] = b;
        b = L1; b += q1; mp.s1_z0 = b;
        b = L0; b += q0; mp.s1_zy = b;                 /* also rle_bits of the empty list */
        mp.min_costs = mp.costs;
    }
}

/* the choice of scan (uniform) */
#if FC_GM
/* every search of this build: the list scan with scratch in HBM and the ->bits of the active pool */
__device__ __forceinline__ void apx_scan(DevFrame &F, Sh &sh, int q, float size, bool regscan, Step0 &pre)
{
    mp_steps_list_global(F, sh, q, size, sh.mp.D);
}
#else
__device__ __forceinline__ void apx_scan(DevFrame &F, Sh &sh, int q, float size, bool regscan, Step0 &pre)
{
    if (sh.band) mp_steps_chroma(F, sh, q, size, sh.mp.D);   /* chroma bands: explicit candidate list */
    else if (regscan) apx_steps_reg(F, sh, q, size, pre);    /* per-candidate scratch in registers (mp_reg.inc) */
    else mp_steps_global(F, sh, q, size);
}
#endif

/* acceptance, lane 0: the combination found becomes the range's approximation if it costs less than max_costs --
 * without the vectors whose weight is zero, and the models learn it.  Returns its costs, MAXCOSTS if it is not taken. */
__device__ __forceinline__ float apx_take(const DevFrame &F, Sh &sh, SFrame &fr, int level)
{
    MPState &mp = sh.mp;
    Range &lr = fr.lrange;
    mp.indices[mp.best_n] = NOEDGE;
    float costs = (mp.matrix_bits + mp.weights_bits + mp.ab) * mp.price + mp.err;
    if (costs < fr.max_costs) {
        int ni = 0;
        unsigned sp = 0;                 /* the symbols move with their weights */
        for (int oi = 0; mp.indices[oi] != NOEDGE; oi++)
            if (mp.weight[oi] != 0) {
                mp.indices[ni] = mp.indices[oi]; mp.into[ni] = mp.into[oi];
                mp.weight[ni] = mp.weight[oi];
                if (oi < 3) sp |= ((mp.symp >> (10 * oi)) & 1023u) << (10 * ni);      /* (ni <= oi) */
                ni++;
            }
        mp.indices[ni] = NOEDGE; mp.into[ni] = NOEDGE;
        models_update(F, sh, mp.indices, mp.into, mp.weight, level, mp.y_state, sp);
        int e = 0;
        for (; mp.indices[e] != NOEDGE; e++) { lr.into[e] = mp.into[e]; lr.weight[e] = mp.weight[e]; }
        lr.into[e] = NOEDGE;
        lr.matrix_bits = mp.matrix_bits; lr.weights_bits = mp.weights_bits; lr.err = mp.err;
    } else {
        lr.into[0] = NOEDGE;
        costs = MAXCOSTS;
    }
    fr.lincomb = costs;
    return costs;
}

/* acceptance, lane 0, FC_SPEC: a block with a checkpoint (chain): guess that its combination wins -- its verifier
 * searches the block, the chain goes on (fr.ckpt = 3) -- or search the block here: after a wrong guess about it, or
 * when the costs of the combination say that it will hardly win (SpecLocal.mlc) */
#if FC_SPEC
__device__ __forceinline__ void apx_spec_checkpoint(Sh &sh, SFrame &fr, float costs)
{
    if (fr.ckpt == 2 && sh.sl.role == 0) {
        Sh::SpecLocal &sl = sh.sl;
        const unsigned slot = (sl.head - 1) % FC_SPEC_W;      /* this block's checkpoint */
        if (sl.nospec) { sl.nospec = 0; sl.n_inline++; }
        else if (costs < (sl.nlc >= 8 ? SPEC_THR * sl.mlc : MAXCOSTS) && !sh.failed) {
            sl.spec_mask |= 1u << slot;
            sl.lin[slot] = costs;
            fr.ckpt = 3;
        } else sl.n_inline++;
    }
}
#else
__device__ __forceinline__ void apx_spec_checkpoint(Sh &sh, SFrame &fr, float costs) { }
#endif

/* acceptance, lane 0: the call's record for the trace (tests: every call's result against the oracle's) */
__device__ __forceinline__ void apx_trace(DevFrame &F, const Sh &sh, const SFrame &fr, int level, int D, float costs)
{
    if (sh.par.trace_on && F.trace_n < F.trace_cap) {
        const MPState &mp = sh.mp;
        const Range &lr = fr.lrange;
        FcTrace &t = F.trace[F.trace_n];
        t.seq = F.trace_n; t.level = level; t.image = mp.image; t.D = D; t.states = sh.states;
        t.cost = costs; t.err = mp.err; t.mbits = mp.matrix_bits; t.wbits = mp.weights_bits;
        int e = 0;
        for (; e < 6; e++) { t.into[e] = -1; if (e < 5) t.w[e] = 0; }
        for (e = 0; costs < MAXCOSTS && lr.into[e] != NOEDGE; e++) { t.into[e] = lr.into[e]; t.w[e] = lr.weight[e]; }
        t.nedges = e;
        F.trace_n++;
    }
}

/* the roofline counters of a call (mp.n is final) */
__device__ __forceinline__ void apx_count(Sh &sh, int level, int D)
{
    sh.cnt.bytes_mp += 4ull * D * (2 + sh.mp.n) + 4ull * (1u << level);
    sh.cnt.n_mp++; sh.cnt.n_steps += sh.mp.n;
}

__device__ __forceinline__ void op_approx(DevFrame &F, Sh &sh)
{
    const int tid = threadIdx.x;
    SFrame &fr = sh.st[sh.sp];
    const int level = fr.lrange.level;
    const float size = (float) (1u << level);
    const int q = level - sh.par.gl0;                    /* Gram table index of this level */
    const int D = sh.pool.n;
    int y = fr.y_state;                                  /* rle_generate, domain-pool.c:716-719 */
    if (y >= 0 && !(F.domain_type[y] & 2)) y = -1;
    APX_CLOCK();
    if (fr.coop) snap_coop_before(sh, fr, sh.sp, sh.par.ML);
    const bool regscan = APX_REGSCAN(sh);
    Step0 pre;
    if (!FC_VARIANT_BIG) apx_issue_early(sh, fr, q, regscan, pre);
    mp_tables(F, sh, level, y);
    if (MP_TABLES_INLINE && !FC_VARIANT_BIG) lds_barrier();      /* the tables live in LDS */
    else __syncthreads();
    APX_MARK(0);
    const bool retries = apx_retry_begin(F, sh);
    do {
        if (tid == 0) apx_setup(F, sh, fr, level, y, D);
        lds_barrier();                   /* the set-up lives in LDS; the scan's first reads stay in flight */
        APX_MARK(1);
        apx_scan(F, sh, q, size, regscan, pre);
        APX_MARK(2);
    } while (apx_retry_next(F, sh, retries));
    /* looked up again: kept across the scan, its address is spilled and reloaded on the serial lane (0.5 % slower) */
    SFrame &fr_behind_scan = sh.st[sh.sp];
    if (tid == 0) {
        const float costs = apx_take(F, sh, fr_behind_scan, level);
        apx_spec_checkpoint(sh, fr_behind_scan, costs);
        apx_trace(F, sh, fr_behind_scan, level, D, costs);
        if (FC_VARIANT_BIG) apx_count(sh, level, D);
    } else if (!FC_VARIANT_BIG && tid == 64) apx_count(sh, level, D);    /* default builds: off the serial lane */
    if (fr_behind_scan.coop) {           /* uniform */
        __syncthreads();                 /* the models as the accepted combination left them */
        snap_coop_after(sh, fr_behind_scan, sh.sp);
    }
    APX_MARK(3);
}
#undef APX_CLOCK
#undef APX_MARK
