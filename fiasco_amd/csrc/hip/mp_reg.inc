/*
 *  mp_reg.inc -- the matching-pursuit step loop with REGISTER-RESIDENT scratch.
 *
 *  The reference keeps rem_numerator / rem_denominator / used / ip_domain_ortho_vector in
 *  static arrays (codec/approx.c:279-305).  Here lane t of the workgroup owns the candidate
 *  states t, t+256, t+512, ... (up to KREG of them) and keeps exactly those entries in VGPRs
 *  for the whole call: after the three coalesced table reads of step 0 (pool position, Gram
 *  diagonal, <range,state> numerators) a step costs ONE coalesced read of the chosen vector's
 *  Gram row and no stores at all.
 *
 *  The ordered scan (codec/approx.c:422-603) runs in rounds: every wave finds, from the
 *  per-block minima in LDS, the next 64-state block that can still beat the running minimum;
 *  the wave that owns that block evaluates its survivors' true costs from its registers,
 *  replays the accept rule in index order (ballot/ffs) and publishes the new minimum and the
 *  winner's record in LDS; one barrier per round.  Block j is owned by wave j % NWAVES,
 *  register slot j / NWAVES.  The accept rule, the record and the commit are mp_step.inc's, shared with
 *  the other scans (mp_steps_list below, the HBM scans); the slot loop of the update is this scan's own.
 */

#define KREG FC_KREG                 /* register slots per lane: S <= KREG * B states */
#define NWAVES (B / 64)

/* Step-0 inputs of the register scan as they come out of memory: three coalesced reads per
 * slot (pool position, Gram diagonal, <range, state> row), all in flight together and NOT looked
 * at here, so that the caller can issue them before lane 0's per-call set-up and its barrier
 * (the set-up and the memory round trip overlap). */
struct Step0 { unsigned praw[KREG]; float draw[KREG], nraw[KREG]; };

/* FC_SPEC, verifier: the candidates are the states below sh.gap_lo and those from sh.gap_hi on; the
 * ids in between are the chain's (fc_lds.inc, Sh).  Slots that lie inside the gap are not
 * read at all, lanes inside it never become candidates. */
#if FC_SPEC
#define SPEC_DEADMASK(sh) const unsigned deadmask_ = (unsigned) __builtin_amdgcn_readfirstlane((int) (sh).deadmask);
#define SLOT_LIVE(k)      (!((deadmask_ >> (k)) & 1u))
#else
#define SPEC_DEADMASK(sh)
#define SLOT_LIVE(k)      true
#endif

__device__ __forceinline__ void mp_step0_issue(const Sh &sh, int q, const float *numrow, Step0 &o)
{
    unsigned utid = threadIdx.x;
    asm volatile("" : "+v"(utid));                   /* see mp_steps_reg */
    const int P = sh.par.P, S = sh.states, K = (S + B - 1) / B;
    const float *diag = sh.par.diag + (size_t) q * P;
    const unsigned short *pos = (const unsigned short *) sh.par.pos;
    SPEC_DEADMASK(sh)
#pragma unroll
    for (int k = 0; k < KREG; k++) {
        /* utid + constant: one 32-bit lane offset, slot offsets fold into the instruction.
         * The loads of a slot in use are unconditional (a per-lane guard costs a branch and a
         * wait per load): lanes past the last state read the neighbouring table of the
         * frame's slab and drop the value */
        o.praw[k] = 0xffffu; o.draw[k] = 1.0f; o.nraw[k] = 0.0f;
        if (k < K && SLOT_LIVE(k)) {                          /* uniform */
            o.praw[k] = (pos + k * B)[utid];
            o.draw[k] = (diag + k * B)[utid];
            o.nraw[k] = (numrow + k * B)[utid];
        }
    }
}

/* KR: register slots per lane this instance carries (S <= KR * B): every slot loop runs KR times whatever the
 * number of states, so a frame with few states per lane takes the instance with few slots */
template <int NIP, int KR = KREG>
__device__ __forceinline__ void mp_steps_reg(DevFrame &F, Sh &sh, int q, float size, const Step0 &pre)
{
    /* opaque copy of the thread index: what the slot loops derive from it (k * B + tid as
     * 64-bit indices, twelve of them) is otherwise hoisted out of the kernel's persistent loop
     * and held in -- or spilled from -- registers for the whole kernel */
    unsigned utid = threadIdx.x;
    asm volatile("" : "+v"(utid));
    const int tid = (int) utid, lane = tid & 63, wave = tid >> 6, P = sh.par.P;
    MPState &mp = sh.mp;
    RoundBox &rb = sh.rb;
    const int S = sh.states, K = (S + B - 1) / B, nblk = (S + 63) >> 6;
    /* size = 2^level: x / size and x * (1 / size) are the same correctly rounded value (scaling
     * by a power of two), and the product is one instruction instead of a division sequence */
    const float rsize = 1.0f / size;
    SPEC_DEADMASK(sh)

    /* pool positions two per register (positions < 32768, -1 = no candidate); the stage-1
     * estimates are not kept: the owner of a block recomputes them in phase B (one more
     * evaluation per round instead of KR registers for the whole call) */
    unsigned ps2[(KR + 1) / 2];
#define PS(k) ((int) (short) (ps2[(k) >> 1] >> (((k) & 1) * 16)))
    /* <state, o_j> of the kept vectors: NIP - 1 per slot.  The projection onto the LAST vector a
     * call can keep (step NIP) is used by that step's full evaluations only: the owner of a block
     * recomputes it there from one more read of the Gram row instead of every lane holding it in
     * a register for the whole call */
    constexpr int NKEEP = NIP > 1 ? NIP - 1 : 1;
    float    num[KR], den[KR], ip[KR][NKEEP];
    unsigned usmask = 0;             /* bit k: slot k is not (or no longer) a candidate */

#pragma unroll
    for (int k = 0; k < KR; k++) {
        const bool ok = k < K && k * B + tid < S && !DEAD(sh, k * B + tid);
        const unsigned pk = ok ? pre.praw[k] : 0xffffu;
        den[k] = ok ? pre.draw[k] : 1.0f;
        num[k] = ok ? pre.nraw[k] : 0.0f;
        if (k & 1) ps2[k >> 1] |= pk << 16; else ps2[k >> 1] = pk;
#pragma unroll
        for (int j = 0; j < NKEEP; j++) ip[k][j] = 0.0f;
    }
    if (tid == 0) { rb.evals = 0; rb.blockevals = 0; }
    unsigned long long tA = 0, tB = 0, tmark = wall_clock64();   /* includes the wait for the step-0 loads */

    for (;;) {
        const int n = mp.n;
        StepCtx ctx;
        load_step_ctx(mp, ctx);
        /* the packed positions stay packed: without this the unpacking is hoisted out of the
         * step loop and the twelve positions occupy twelve registers again */
#pragma unroll
        for (int i = 0; i < (KR + 1) / 2; i++) asm volatile("" : "+v"(ps2[i]));
        /* ---------------- phase A ---------------- */
        if (n == 0) {
#pragma unroll
            for (int k = 0; k < KR; k++) {
                bool uu = PS(k) < 0 || MP_EXCLUDED(mp, PS(k));
                if (!uu) {                                    /* codec/approx.c:360-374 */
                    uu = den[k] * rsize < MIN_NORM;
                    if (!uu) uu = fabsf(num[k]) < MIN_NORM;
                }
                usmask |= uu ? (1u << k) : 0u;
            }
        } else {
            const int nv = n - 1, row = mp.row_state;
#if FC_GRAM_TRI
            const float *Gq = PGRAM(sh, q);
            float g[KR];
            if (tid == (row & (B - 1))) usmask |= 1u << (row / B);   /* the vector chosen last step */
            {   /* <candidate, chosen state>: the chosen state's row up to the diagonal, its column
                 * behind it (one 4-byte gather per candidate there).  Every lane loads (uniform
                 * guard); a lane past the last state reads the entry of the last one and drops it. */
                const unsigned urow = (unsigned) row, rowoff = TRI(row), last = (unsigned) (S - 1);
                if (row < FC_TRI_HOT) {                       /* uniform */
                    /* one of the first states: its column is also kept as a row (DevFrame.gcol) -- one
                     * coalesced read instead of a gather per candidate */
                    const float *Cq = sh.par.gcol + ((size_t) q * FC_TRI_HOT + urow) * P;
#pragma unroll
                    for (int k = 0; k < KR; k++) {
                        g[k] = 0.0f;
                        if (k < K) {
                            unsigned d = (unsigned) (k * B) + utid;
                            d = d < last ? d : last;
                            g[k] = d <= urow ? Gq[rowoff + d] : Cq[d];
                        }
                    }
                } else {
#pragma unroll
                for (int k = 0; k < KR; k++) {
                    g[k] = 0.0f;
                    if (k < K) {
                        unsigned d = (unsigned) (k * B) + utid;
                        d = d < last ? d : last;
                        g[k] = Gq[d <= urow ? rowoff + d : TRI(d) + urow];
                    }
                }
                }
            }
#else
            const float *Grow = PGRAM(sh, q) + (size_t) row * P;
            float g[KR];
            if (tid == (row & (B - 1))) usmask |= 1u << (row / B);   /* the vector chosen last step */
#pragma unroll
            for (int k = 0; k < KR; k++) {
                g[k] = 0.0f;
                if (k < K && SLOT_LIVE(k)) g[k] = (Grow + k * B)[utid];      /* uniform guard, every lane loads */
            }
            {   /* the newest (< 32 + auxiliary) states have no mirrored entries in older rows
                 * yet (gram_flush): their lanes read the entry from the candidate's own row */
                const int flim = sh.flim;
                if (S > flim && S - 1 > row) {               /* uniform, short-lived state */
                    const float *Gcol = PGRAM(sh, q) + row;
                    unsigned ut = utid;                      /* see above: nothing of this rare */
                    asm volatile("" : "+v"(ut));             /* path is precomputed per slot    */
#pragma unroll
                    for (int k = 0; k < KR; k++) {
                        const int d = k * B + (int) ut;
                        if ((k + 1) * B > flim && k < K && d > row && d >= flim && !((usmask >> k) & 1u))
                            g[k] = Gcol[(size_t) d * P];
                    }
                }
            }
#endif
            float novk[NIP], selk[NIP];
#pragma unroll
            for (int j = 0; j < NIP; j++) {
                novk[j] = j < nv ? mp.norm_ov[j] : 1.0f;
                selk[j] = j < nv ? mp.sel_ipdo[nv][j] : 0.0f;
            }
            const float nov_nv = mp.norm_ov[nv], ipio_nv = mp.ipio[nv];
#pragma unroll
            /* mp_orthogonalize() written out: through the helper the (uniform) branch round the division of a slot
             * becomes a select and the division runs in every step (wide builds: 1 % of the 4K frame rate) */
            for (int k = 0; k < KR; k++) {                  /* codec/approx.c:676-698 */
                if ((usmask >> k) & 1u) continue;
                float t = g[k];
#pragma unroll
                for (int j = 0; j < NIP - 1; j++)
                    if (j < nv) t -= ip[k][j] / novk[j] * selk[j];
#pragma unroll
                for (int j = 0; j < NIP - 1; j++)
                    if (j == nv) ip[k][j] = t;
                den[k] -= t * t / nov_nv;
                num[k] -= ipio_nv / nov_nv * t;
                if (den[k] * rsize < MIN_NORM) usmask |= 1u << k;
            }
        }
        /* the estimates, one form per number of kept vectors (wave-uniform branch: the first
         * step of a call has none and prices a candidate without any interval select); lane 63
         * ends up with the block minimum and stores it */
        /* four slots at a time: the estimates of four blocks, then their minima with interleaved
         * DPP chains (wave_min4_l63) */
#define EST_ONE(NPV, k, ek)                                                                      \
        float ek = BIGF;                                                                         \
        if ((k) < K && !((usmask >> (k)) & 1u))                                                  \
            ek = stage1<NIP, NPV, true>(ctx, PS(k), (k) * B + tid, num[k], den[k]);
#define EST_PASS(NPV)                                                                            \
        _Pragma("unroll")                                                                        \
        for (int k4 = 0; k4 + 4 <= KR; k4 += 4) {                                              \
            if (k4 < K) {                                    /* uniform: skip unused groups */   \
                EST_ONE(NPV, k4, e0) EST_ONE(NPV, k4 + 1, e1) EST_ONE(NPV, k4 + 2, e2) EST_ONE(NPV, k4 + 3, e3) \
                wave_min4_l63(e0, e1, e2, e3);                                                   \
                if (lane == 63) {                                                                \
                    sh.blockmin[NWAVES * k4 + wave] = e0;                                        \
                    if (k4 + 1 < K) sh.blockmin[NWAVES * (k4 + 1) + wave] = e1;                  \
                    if (k4 + 2 < K) sh.blockmin[NWAVES * (k4 + 2) + wave] = e2;                  \
                    if (k4 + 3 < K) sh.blockmin[NWAVES * (k4 + 3) + wave] = e3;                  \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
        _Pragma("unroll")                                                                        \
        for (int k = KR / 4 * 4; k < KR; k++) {                                              \
            if (k < K) {                                                                         \
                EST_ONE(NPV, k, ek)                                                              \
                ek = wave_min_l63(ek);                                                           \
                if (lane == 63) sh.blockmin[NWAVES * k + wave] = ek;                             \
            }                                                                                    \
        }
        if (ctx.np == 0)      { EST_PASS(0) }
        else if (ctx.np == 1) { EST_PASS(1) }
        else                  { EST_PASS(-1) }
#undef EST_PASS
#undef EST_ONE
        if (tid == 0) { rb.m2[1] = mp.min_costs; rb.state = -1; }   /* "round -1" */
        __syncthreads();
        if (tid == 0) { unsigned long long t = wall_clock64(); tA += t - tmark; tmark = t; }

        /* ---------------- phase B: rounds ---------------- */
        float m = rb.m2[1];
        int round = 0;
        int cursor = -1;
        for (;;) {
            int jb = -1;
            for (int bb = 0; bb < nblk && jb < 0; bb += 64) {
                float bmv = (bb + lane < nblk) ? sh.blockmin[bb + lane] : BIGF;
                unsigned long long mask = __ballot(bmv < m && bb + lane > cursor);
                if (mask) jb = bb + __ffsll((long long) mask) - 1;
            }
            if (jb < 0) break;                               /* uniform over the workgroup */
            cursor = jb;
            if (jb % NWAVES == wave) {
                const int kk = jb / NWAVES;
                float numk = 0, denk = 1, ipk[NIP];
                int psk = -1;
#pragma unroll
                for (int j = 0; j < NIP; j++) ipk[j] = 0;
#pragma unroll
                for (int k = 0; k < KR; k++)
                    if (k == kk) {
                        numk = num[k]; denk = den[k]; psk = PS(k);
#pragma unroll
                        for (int j = 0; j < NIP - 1; j++) ipk[j] = ip[k][j];
                    }
                const int state = kk * B + tid;
                /* the last step: <state, o_(NIP-1)> again, as phase A computed it (same inputs, same operations) */
                if (n == NIP && !((usmask >> kk) & 1u))
                    ipk[NIP - 1] = mp_project<NIP - 1>(gram_load(PGRAM(sh, q), P, mp.row_state, state, sh.flim), ipk,
                                                       mp.norm_ov, mp.sel_ipdo[NIP - 1], NIP - 1);
                /* the estimate of phase A again (same inputs, same value) */
                const float ek = ((usmask >> kk) & 1u) ? BIGF : stage1<NIP>(ctx, psk, state, numk, denk);
                bool pass = ek < m;
                Eval ev;
                eval_clear(ev);
                const float i0 = ipk[0], i1 = NIP > 1 ? ipk[1 % NIP] : 0.0f;
                const float i2 = NIP > 2 ? ipk[2 % NIP] : 0.0f, i3 = NIP > 3 ? ipk[3 % NIP] : 0.0f;
                if (pass) full_eval<NIP>(F, sh, mp, sh.lglv, n, psk, state, numk, denk, i0, i1, i2, i3, ev);
                unsigned npass = (unsigned) __popcll(__ballot(pass));
                const int win = mp_accept(pass, ek, ev.costs, lane, m);
                if (lane == win) mp_record(rb, state, psk, ev, numk, denk, ipk);      /* at most one lane */
                if (lane == 0) { rb.m2[round & 1] = m; rb.evals += npass; rb.blockevals++; }
            }
            __syncthreads();
            m = rb.m2[round & 1];
            round++;
        }
        /* ---------------- commit (lane 0) ---------------- */
        if (tid == 0) mp_commit(F, sh, n, rb);
        __syncthreads();
        if (tid == 0) { unsigned long long t = wall_clock64(); tB += t - tmark; tmark = t; }
        if (!(mp.n < sh.par.max_elements && mp.index >= 0)) break;
    }
    if (tid == 0) {
        sh.cnt.n_fulleval += rb.evals; sh.cnt.n_blockevals += rb.blockevals;
        sh.cnt.t_mpA += tA; sh.cnt.t_mpB += tB;
    }
}
#undef PS

/*
 *  The same step loop over a short explicit candidate LIST: the chroma bands search the <= 40
 *  states kept by rle_chroma plus the co-located luminance state (codec/domain-pool.c:707-735,
 *  854-879; D <= 64).  Candidate c = lane c of wave 0, list position == c, state = sh.dl[c];
 *  the Gram row read becomes a gather.  One block, so the ordered replay is a single ballot
 *  loop.
 */
template <int NIP>
__device__ __forceinline__ void mp_steps_list(DevFrame &F, Sh &sh, int q, float size, int D)
{
    const int tid = threadIdx.x, P = sh.par.P;
    MPState &mp = sh.mp;
    RoundBox &rb = sh.rb;
    const bool ok = tid < D;
    const int st = ok ? (int) sh.dl[tid] : 0;
    float den = ok ? sh.par.diag[(size_t) q * P + st] : 1.0f;
    float num = ok ? MP_NUMROW(F, mp)[st] : 0.0f;
    float ip[NIP];
#pragma unroll
    for (int j = 0; j < NIP; j++) ip[j] = 0.0f;
    bool used = !ok;
    unsigned evals = 0, steps = 0;

    for (;;) {
        const int n = mp.n;
        StepCtx ctx;
        load_step_ctx(mp, ctx);
        if (n == 0) {
            if (ok) {                                         /* codec/approx.c:360-374 */
                bool uu = den / size < MIN_NORM;
                if (!uu) uu = fabsf(num) < MIN_NORM;
                used = uu || MP_EXCLUDED(mp, tid);
            }
        } else {
            const int nv = n - 1;
            if (tid == (int) mp.indices[nv]) used = true;     /* the vector chosen last step */
            if (!used) {                                      /* codec/approx.c:676-698 */
                const float t = mp_orthogonalize<NIP>(gram_load(PGRAM(sh, q), P, mp.row_state, st, sh.flim), ip, mp.norm_ov,
                                                      mp.sel_ipdo[nv], nv, mp.norm_ov[nv], mp.ipio[nv], num, den);
#pragma unroll
                for (int j = 0; j < NIP; j++)
                    if (j == nv) ip[j] = t;
                if (den / size < MIN_NORM) used = true;
            }
        }
        if (tid < 64) {                                       /* wave 0 holds the whole list */
            const int lane = tid;
            float e = used ? BIGF : stage1<NIP>(ctx, tid, st, num, den);
            float m = mp.min_costs;
            bool pass = e < m;
            Eval ev;
            eval_clear(ev);
            if (pass)
                full_eval<NIP>(F, sh, mp, sh.lglv, n, tid, st, num, den, ip[0], NIP > 1 ? ip[1 % NIP] : 0.0f,
                          NIP > 2 ? ip[2 % NIP] : 0.0f, NIP > 3 ? ip[3 % NIP] : 0.0f, ev);
            evals += (unsigned) __popcll(__ballot(pass));
            const int win = mp_accept(pass, e, ev.costs, lane, m);
            if (lane == 0) rb.state = -1;
            if (lane == win) mp_record(rb, st, tid, ev, num, den, ip);        /* at most one lane */
        }
        __syncthreads();
        if (tid == 0) mp_commit(F, sh, n, rb);
        steps++;
        __syncthreads();
        if (!(mp.n < sh.par.max_elements && mp.index >= 0)) break;
    }
    if (tid == 0) { sh.cnt.n_fulleval += evals; sh.cnt.n_blockevals += steps; }
}
