/*
 *  mp_step.inc -- what every scan of the matching pursuit does with a candidate, written once (included by
 *  mp_device.inc in front of the scans): clearing an Eval, the accept rule, the winner's record, the commit of a step,
 *  the Gram-Schmidt update of one candidate, and phase B of the two scans that keep their scratch in HBM.  The scans
 *  differ in where a candidate's num / den / projections live and in how the candidates are spread over the lanes.
 *  Code-shape rule as in mp_device.inc: compile-time trip counts, no dynamically indexed private arrays.
 */

/* an Eval no full_eval has filled in (under FC_GM the caller sets qc) */
__device__ __forceinline__ void eval_clear(Eval &ev)
{
    ev.costs = BIGF; ev.m_bits = ev.w_bits = ev.m_err = 0; ev.symp = SYMP_NONE;
#pragma unroll
    for (int k = 0; k < MAXED; k++) ev.f[k] = 0;
}

/* The accept rule of the reference's scan (strict '<' against the running minimum, codec/approx.c:459-462,592)
 * replayed in index order over the 64 candidates of a wave: `pass' = the lane evaluated its candidate, e its
 * estimate, cost its true cost.  Returns the lane whose candidate is the minimum now, -1 if m stands; m follows. */
__device__ __forceinline__ int mp_accept(bool pass, float e, float cost, int lane, float &m)
{
    int last = -1, win = -1;
    for (;;) {
        unsigned long long ok = __ballot(pass && lane > last && e < m && cost < m);
        if (!ok) break;
        int j = __ffsll((long long) ok) - 1;
        last = j; win = j;
        m = __shfl(cost, j);
    }
    return win;
}

/* the winner's record (RoundBox, fc_lds.inc): what mp_commit() needs of the candidate that won.  idx = its pool
 * position (no pos[] read at commit); ip = its projections <state, o_j>, NP of them */
template <int NP>
__device__ __forceinline__ void mp_record(RoundBox &w, int state, int idx, const Eval &ev, float num, float den,
                                          const float (&ip)[NP])
{
    w.state = state; w.idx = idx;
    w.cost = ev.costs; w.mbits = ev.m_bits; w.wbits = ev.w_bits; w.err = ev.m_err; w.symp = ev.symp;
#pragma unroll
    for (int k = 0; k < MAXED; k++) w.f[k] = ev.f[k];
    w.num = num; w.den = den;
#pragma unroll
    for (int j = 0; j < MAXED - 1; j++) w.ip[j] = j < NP ? ip[j % NP] : 0.0f;
}

#if FC_GM
/* probability index of list position pos in the active quasi-arithmetic pool (0 where there is none) */
__device__ __forceinline__ short gm_qidx(const Sh &sh, int pos)
{
    return GM_QAC(sh.gm.pk[0]) && pos < (int) sh.pool.n ? GQ_CUR(sh, 0)[pos] : (short) 0;
}
#endif

/* Commit of step n, lane 0: the winner w (w.state < 0: no candidate beat the minimum) becomes vector n of the
 * combination and, if it is the cheapest so far, the call's result; then the serial set-up of the next step.
 * Returns what it leaves in mp.index: the winner's pool position or -1. */
__device__ __forceinline__ int mp_commit(const DevFrame &F, Sh &sh, int n, const RoundBox &w)
{
    MPState &mp = sh.mp;
    const int bstate = w.state;
    const int index = bstate >= 0 ? w.idx : -1;
    if (index >= 0) {
        if (w.cost < mp.costs) {
            mp.costs = w.cost; mp.err = w.err;
            mp.matrix_bits = w.mbits; mp.weights_bits = w.wbits;
#pragma unroll
            for (int k = 0; k < MAXED; k++) if (k <= n) mp.weight[k] = w.f[k];
            mp.symp = w.symp;
            mp.best_n = n + 1;
        }
        mp.indices[n] = (short) index;
        mp.into[n] = (short) bstate;
#if FC_GM
        mp.kq[n] = gm_qidx(sh, index);
#endif
        mp.norm_ov[n] = w.den;
        mp.ipio[n] = w.num;
#pragma unroll
        for (int k = 0; k < MAXED - 1; k++) if (k < n) mp.sel_ipdo[n][k] = w.ip[k];
        mp.row_state = bstate;
        mp.n = n + 1;
        if (mp.n < sh.par.max_elements) mp_step_prepare(F, sh, mp, sh.lglv, sh.lglv_m1);
    }
    mp.index = index;
    return index;
}

/* Gram-Schmidt update of one candidate against o_nv, the vector chosen in the step before (codec/approx.c:676-698):
 * g = <candidate, chosen state>, ip[j] = <candidate, o_j>, nov[j] = |o_j|^2 and sel[j] = <chosen state, o_j> for
 * j < nv (the entries from nv on are not looked at), ipio_nv = <range, o_nv>.  mp_project() is <candidate, o_nv>;
 * mp_orthogonalize() returns it, the caller keeps it where it keeps its projections.  The order of operations is the
 * reference's. */
template <int NJ, int NI, int NV, int NS>
__device__ __forceinline__ float mp_project(float g, const float (&ip)[NI], const float (&nov)[NV], const float (&sel)[NS], int nv)
{
    static_assert(NJ <= NI && NJ <= NV && NJ <= NS, "an array is shorter than the number of kept vectors");
    float t = g;
#pragma unroll
    for (int j = 0; j < NJ; j++)
        if (j < nv) t -= ip[j] / nov[j] * sel[j];
    return t;
}
template <int NJ, int NI, int NV, int NS>
__device__ __forceinline__ float mp_orthogonalize(float g, const float (&ip)[NI], const float (&nov)[NV], const float (&sel)[NS],
                                                  int nv, float nov_nv, float ipio_nv, float &num, float &den)
{
    const float t = mp_project<NJ>(g, ip, nov, sel, nv);
    den -= t * t / nov_nv;
    num -= ipio_nv / nov_nv * t;
    return t;
}

/* Phase B of the scans with scratch in HBM (F.num, F.den, F.est, F.ipdo, F.used: indexed by candidate number), inside
 * wave 0: the ordered replay over the block minima phase A left in sh.blockmin (NC candidates), then the commit.
 * LIST: candidate c is position c of the list F.pool_states (mp_steps_list_global); else it is state c, at position
 * F.pos[c] (mp_steps_global).  The best candidate lives in wave-uniform registers; its symbols are not carried. */
#define CAND_STATE(c) (LIST ? (int) F.pool_states[c] : (c))
#define CAND_POS(c)   (LIST ? (c) : (int) F.pos[c])
template <bool LIST>
__device__ __forceinline__ void mp_replay_hbm(DevFrame &F, Sh &sh, int n, int NC, unsigned &blockevals)
{
    const int lane = threadIdx.x & 63, P = F.P;
    MPState &mp = sh.mp;
    const int nblk = (NC + 63) >> 6;
    float m = mp.min_costs;
    unsigned evals = 0;
    int b_c = -1;                        /* the best candidate of the step (wave-uniform copies) */
    float b_cost = 0, b_mbits = 0, b_wbits = 0, b_err = 0, b_f[MAXED];
#pragma unroll
    for (int k = 0; k < MAXED; k++) b_f[k] = 0;
    for (int bb = 0; bb < nblk; bb += 64) {
        float bm = (bb + lane < nblk) ? sh.blockmin[bb + lane] : BIGF;
        int lastb = -1;
        for (;;) {
            unsigned long long mask = __ballot(bm < m && lane > lastb);
            if (!mask) break;
            int jb = __ffsll((long long) mask) - 1;
            lastb = jb;
            const int c = ((bb + jb) << 6) + lane;
            float e = (c < NC) ? F.est[c] : BIGF;
            bool pass = e < m;
            Eval ev;
            eval_clear(ev);
            if (pass) {
                float i0 = n > 0 ? F.ipdo[c] : 0.0f, i1 = n > 1 ? F.ipdo[(size_t) P + c] : 0.0f;
                float i2 = n > 2 ? F.ipdo[(size_t) 2 * P + c] : 0.0f, i3 = n > 3 ? F.ipdo[(size_t) 3 * P + c] : 0.0f;
#if FC_GM
                ev.qc = gm_qidx(sh, CAND_POS(c));
#endif
                full_eval<MAXED - 1>(F, sh, mp, sh.lglv, n, CAND_POS(c), CAND_STATE(c), F.num[c], F.den[c], i0, i1, i2, i3, ev);
            }
            evals += (unsigned) __popcll(__ballot(pass));
            blockevals++;
            const int win = mp_accept(pass, e, ev.costs, lane, m);
            if (win >= 0) {                 /* wave-uniform */
                b_c = ((bb + jb) << 6) + win;
                b_cost = __shfl(ev.costs, win); b_mbits = __shfl(ev.m_bits, win);
                b_wbits = __shfl(ev.w_bits, win); b_err = __shfl(ev.m_err, win);
#pragma unroll
                for (int k = 0; k < MAXED; k++) b_f[k] = __shfl(ev.f[k], win);
            }
        }
    }
    if (lane == 0) {
        sh.cnt.n_fulleval += evals;
        RoundBox w;
        w.state = -1;
        if (b_c >= 0) {
            w.state = CAND_STATE(b_c); w.idx = CAND_POS(b_c);
            w.cost = b_cost; w.mbits = b_mbits; w.wbits = b_wbits; w.err = b_err; w.symp = SYMP_NONE;
#pragma unroll
            for (int k = 0; k < MAXED; k++) w.f[k] = b_f[k];
            w.num = F.num[b_c]; w.den = F.den[b_c];
#pragma unroll
            for (int k = 0; k < MAXED - 1; k++) w.ip[k] = k < n ? F.ipdo[(size_t) k * P + b_c] : 0.0f;
        }
        if (mp_commit(F, sh, n, w) >= 0) F.used[b_c] = 1;
    }
}
#undef CAND_STATE
#undef CAND_POS
