/*
 *  fc_serial.inc -- the partition search as a serial state machine on lane 0: the tree model,
 *  snapshots, store_new_state, the bands of a colour frame (band_advance), the chain's side of
 *  speculation (spec_poll, spec_luminance_done), serial_step and serial_advance.
 *
 *  Reference: partition search codec/subdivide.c:60-502; bands codec/coder.c:738-833; rate
 *  models codec/bintree.c:35-73.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

/* ------------------------------------------------------------------ serial state machine */

__device__ float tree_bits_dev(const Sh &sh, int ML, int child, int level, int which)
{
    const unsigned *counts = sh.tm + which * 2 * ML;
    float prob = counts[level] / (float) counts[ML + level];
    return child ? (float) -log2((double) prob) : (float) -log2((double) (1 - prob));
}

__device__ void tree_update_dev(Sh &sh, int ML, int child, int level, int which)
{
    unsigned *counts = sh.tm + which * 2 * ML;
    if (child) counts[level]++;
    counts[ML + level]++;
}

/* model snapshots: short runs of 128-bit LDS copies (lane 0) */
__device__ __forceinline__ void copy16(uint4 *dst, const uint4 *src, int n)
{
    /* 8 independent 128-bit LDS reads in flight, then 8 writes: a dependent read->write
     * chain per element would cost one LDS latency (~64 cycles) each */
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        /* named temporaries: an indexed local array ends up in scratch memory */
        uint4 t0 = src[i], t1 = src[i + 1], t2 = src[i + 2], t3 = src[i + 3];
        uint4 t4 = src[i + 4], t5 = src[i + 5], t6 = src[i + 6], t7 = src[i + 7];
        dst[i] = t0; dst[i + 1] = t1; dst[i + 2] = t2; dst[i + 3] = t3;
        dst[i + 4] = t4; dst[i + 5] = t5; dst[i + 6] = t6; dst[i + 7] = t7;
    }
    for (; i < n; i++) dst[i] = src[i];
}

__device__ void snap_save(const DevFrame &F, Sh &sh, int depth, int which)
{
    copy16(SNAP_AT(sh, depth, which), (const uint4 *) &sh.cb, sh.n16);
}

__device__ void snap_load(const DevFrame &F, Sh &sh, int depth, int which)
{
    copy16((uint4 *) &sh.cb, SNAP_AT(sh, depth, which), sh.n16);
}

#if FC_VARIANT_BIG
/* the resting coefficient model (sh.dcb) */
__device__ void snap_save_d(Sh &sh, int depth, int which)
{
    copy16(SNAP_AT(sh, depth, which), (const uint4 *) &sh.dcb, sh.n16);
}

__device__ void snap_load_d(Sh &sh, int depth, int which)
{
    copy16((uint4 *) &sh.dcb, SNAP_AT(sh, depth, which), sh.n16);
}
#endif

__device__ __forceinline__ void tm_save(Sh &sh, int depth, int ML, int which = 0)
{
    copy16(TM_AT(sh, depth, which, ML), (const uint4 *) sh.tm, TM_N16(ML));
}

__device__ __forceinline__ void tm_load(Sh &sh, int depth, int ML, int which = 0)
{
    copy16((uint4 *) sh.tm, TM_AT(sh, depth, which, ML), TM_N16(ML));
}

/* wfalib.c:152-180 */
__device__ float final_distribution_dev(const DevFrame &F, int s)
{
    float f = 0;
    int dom;
    for (int l = 0; l < 2; l++) {
        if ((dom = TREE(F, s, l)) != RANGE_) f += F.final_d[dom];
        for (int e = 0; (dom = INTO(F, s, l, e)) != NOEDGE; e++)
            f += WEIGHT(F, s, l, e) * F.final_d[dom];
    }
    return f / 2;
}

/* init_new_state (codec/subdivide.c:549-610): store the new state's rows; edge lists are
 * kept sorted by target like append_edge (codec/wfalib.c:233-275) */
#if !FC_VARIANT_BIG
/* The default build's form (<= 3 edges per label): table bases from LDS as global pointers, the
 * edge lists sorted in registers (a dynamically indexed private array lives in scratch memory),
 * the final distribution from the values at hand -- the terms' entries are read in one batch, not
 * found again one dependent read at a time through the rows just stored. */
__device__ void store_new_state(DevFrame &__restrict__ F, Sh &sh, SFrame &fr, int aux)
{
    const int s = sh.states, PA = sh.par.PA;
    GLOBAL_AS int16_t *const tree = (GLOBAL_AS int16_t *) sh.par.at_tree, *const into = (GLOBAL_AS int16_t *) sh.par.at_into;
    GLOBAL_AS int16_t *const posv = (GLOBAL_AS int16_t *) sh.par.pos, *const pool = (GLOBAL_AS int16_t *) sh.par.at_pool;
    GLOBAL_AS float *const weight = (GLOBAL_AS float *) sh.par.at_weight, *const fin = (GLOBAL_AS float *) sh.par.at_final;
    GLOBAL_AS uint16_t *const xs = (GLOBAL_AS uint16_t *) sh.par.at_x, *const ys = (GLOBAL_AS uint16_t *) sh.par.at_y;
    short p = -1;
    if (!aux && sh.pool.n < sh.pool.max_domains) {
        p = (short) sh.pool.n;
        pool[sh.pool.n++] = (short) s;
    }
    posv[s] = p;
    fr.rrange.into[0] = NOEDGE;
    fr.rrange.tree = s;
    int   tr[2], i[2][3];
    float w[2][3], fd_t[2], fd_e[2][3];
#pragma unroll
    for (int l = 0; l < 2; l++) {
        const Range &ch = fr.child[l];
        tr[l] = ch.tree;
        bool live = true;
#pragma unroll
        for (int e = 0; e < 3; e++) {                     /* NOEDGE terminated; missing: sorts last */
            live = live && ch.into[e] != NOEDGE;
            i[l][e] = live ? (int) ch.into[e] : 0x7fff;
            w[l][e] = live ? ch.weight[e] : 0.0f;
        }
        /* ascending by target (append_edge, codec/wfalib.c:233-275; targets are distinct) */
#define CSWAP(a, b) if (i[l][a] > i[l][b]) { int ti = i[l][a]; i[l][a] = i[l][b]; i[l][b] = ti; float tw = w[l][a]; w[l][a] = w[l][b]; w[l][b] = tw; }
        CSWAP(0, 1) CSWAP(1, 2) CSWAP(0, 1)
#undef CSWAP
        /* every term's final distribution entry requested at once (missing terms: state 0) */
        fd_t[l] = fin[tr[l] != RANGE_ ? tr[l] : 0];
#pragma unroll
        for (int e = 0; e < 3; e++) fd_e[l][e] = fin[i[l][e] != 0x7fff ? i[l][e] : 0];
    }
    float f = 0;                                          /* wfalib.c:152-180 */
#pragma unroll
    for (int l = 0; l < 2; l++) {
        const Range &ch = fr.child[l];
        tree[l * PA + s] = (short) tr[l];
        xs[l * PA + s] = (uint16_t) ch.x;
        ys[l * PA + s] = (uint16_t) ch.y;
        if (tr[l] != RANGE_) f += fd_t[l];
#pragma unroll
        for (int e = 0; e < 3; e++)
            if (i[l][e] != 0x7fff) {
                into[(l * 6 + e) * PA + s] = (short) i[l][e];
                weight[(l * 6 + e) * PA + s] = w[l][e];
                f += w[l][e] * fd_e[l][e];
            }
        const int ne = (i[l][0] != 0x7fff) + (i[l][1] != 0x7fff) + (i[l][2] != 0x7fff);
        into[(l * 6 + ne) * PA + s] = NOEDGE;
        /* y_column (codec/subdivide.c:560-567), see the general form below */
        if (sh.par.color) {
            int yc = 0;
#pragma unroll
            for (int e = 0; e < 3; e++) if (i[l][e] != 0x7fff && i[l][e] == fr.ny[l]) yc = 1;
            ((GLOBAL_AS uint8_t *) sh.par.at_ycol)[l * PA + s] = (uint8_t) yc;
        }
    }
    fin[s] = f / 2;
    /* the term lists op_append works from (slot 0 = tree child with weight 1 if any, then the edges
     * in stored order; unused slots: valid dummies), so that it need not read the rows back */
#pragma unroll
    for (int l = 0; l < 2; l++) {
        int m = 0;
        const int c = tr[l] != RANGE_;
        sh.gs_c[l] = c;
        int   gi[4]; float gw[4];
#pragma unroll
        for (int a = 0; a < 4; a++) { gi[a] = 0; gw[a] = 0.0f; }
        if (c) { gi[0] = tr[l]; gw[0] = 1.0f; m = 1; }
#pragma unroll
        for (int e = 0; e < 3; e++)
            if (i[l][e] != 0x7fff) {
#pragma unroll
                for (int a = 0; a < 4; a++) if (a == m) { gi[a] = i[l][e]; gw[a] = w[l][e]; }
                m++;
            }
        sh.gs_n[l] = m;
#pragma unroll
        for (int a = 0; a <= MAXED; a++) { sh.gs_idx[l][a] = a < 4 ? gi[a < 4 ? a : 0] : 0; sh.gs_w[l][a] = a < 4 ? gw[a < 4 ? a : 0] : 0.0f; }
    }
    ((GLOBAL_AS uint8_t *) sh.par.at_los)[s] = (uint8_t) fr.rrange.level;
    ((GLOBAL_AS uint8_t *) sh.par.at_dtype)[s] = aux ? 0 : 2;
}
#else
__device__ void store_new_state(DevFrame &__restrict__ F, Sh &sh, SFrame &fr, int aux)
{
    const int s = sh.states;
    F.pos[s] = -1;
#if FC_GM
    if (!aux) gm_offer(F, sh, s);
#else
    if (!aux && sh.pool.n < sh.pool.max_domains) {
        F.pos[s] = (short) sh.pool.n;
        F.pool_states[sh.pool.n++] = (short) s;
#if FC_VARIANT_BIG
        if (sh.nslot == 5) sh.dpool.n = sh.pool.n;      /* one list, two sets of counters */
#endif
    }
#endif
    fr.rrange.into[0] = NOEDGE;
    fr.rrange.tree = s;
    for (int l = 0; l < 2; l++) {
        const Range &ch = fr.child[l];
        TREE(F, s, l) = (short) ch.tree;
        F.x[l * F.PA + s] = (uint16_t) ch.x;
        F.y[l * F.PA + s] = (uint16_t) ch.y;
        short si[MAXED + 1]; float sw[MAXED + 1];
        int ne = 0;
        for (int e = 0; ch.into[e] != NOEDGE; e++) {
            int pos = 0;
            while (pos < ne && si[pos] < ch.into[e]) pos++;
            for (int j = ne; j > pos; j--) { si[j] = si[j - 1]; sw[j] = sw[j - 1]; }
            si[pos] = ch.into[e]; sw[pos] = ch.weight[e];
            ne++;
        }
        for (int e = 0; e < ne; e++) { INTO(F, s, l, e) = si[e]; WEIGHT(F, s, l, e) = sw[e]; }
        INTO(F, s, l, ne) = NOEDGE;
        /* y_column (codec/subdivide.c:560-567).  The flag stays with the state ID when the
         * state is removed again (remove_states, codec/wfalib.c:283-309, does not clear it)
         * and the join states of a colour frame never set theirs: they show what an earlier,
         * removed state of the same ID left behind, and the stream writer reads it. */
        if (F.color) {
            int yc = 0;
            for (int e = 0; ch.into[e] != NOEDGE; e++) if (ch.into[e] == fr.ny[l]) yc = 1;
            F.ycol[l * F.PA + s] = (uint8_t) yc;
        }
#if FC_VARIANT_BIG
        if (F.frame_type)                              /* wfa->mv_tree, codec/subdivide.c:592 */
            for (int k = 0; k < 5; k++) F.mv[(k * 2 + l) * F.PA + s] = ch.mv[k];
#endif
    }
    F.final_d[s] = final_distribution_dev(F, s);
    F.level_of_state[s] = (uint8_t) fr.rrange.level;
    F.domain_type[s] = aux ? 0 : 2;
}
#endif

/* auxiliary state joining two band trees (codec/coder.c:803-833) */
__device__ int append_join_state(DevFrame &__restrict__ F, Sh &__restrict__ sh, int t0, int t1, int level)
{
    const int s = sh.states;
    if (s >= F.PA) { sh.failed = FC_ERR_CAPACITY; return 0; }
    TREE(F, s, 0) = (short) t0; TREE(F, s, 1) = (short) t1;
    for (int l = 0; l < 2; l++) {
        INTO(F, s, l, 0) = NOEDGE;
        F.x[l * F.PA + s] = 0; F.y[l * F.PA + s] = 0;
    }
    F.final_d[s] = final_distribution_dev(F, s);
    F.level_of_state[s] = (uint8_t) level;
    F.domain_type[s] = 0;
    F.pos[s] = -1;
#if FC_VARIANT_BIG
    if (F.frame_type) for (int k = 0; k < 10; k++) F.mv[k * F.PA + s] = 0;
#endif
    sh.states++;
    if (sh.states >= F.limit_states) { sh.failed = FC_ERR_STATES; return 0; }
    return 1;
}

__device__ void push_root(DevFrame &__restrict__ F, Sh &__restrict__ sh, int y_state)
{
    SFrame &r = sh.st[0];
    r.rg.x = r.rg.y = r.rg.image = r.rg.address = 0;
    r.rg.level = F.level; r.rg.tree = RANGE_;
    for (int i = 0; i < RANGE_E; i++) { r.rg.weight[i] = 0; r.rg.into[i] = 0; }
    r.rg.err = r.rg.tree_bits = r.rg.matrix_bits = r.rg.weights_bits = 0;
    r.max_costs = MAXCOSTS;
    r.y_state = y_state;
    r.phase = PH_ENTER;
#if FC_SPEC
    r.ckpt = 0;
#endif
#if FC_VARIANT_BIG
    r.rg.nd_tree_bits = r.rg.nd_weights_bits = r.rg.mv_tree_bits = r.rg.mv_coord_bits = 0; r.rg.prediction = 0;
    for (int i = 0; i < 5; i++) r.rg.mv[i] = 0;
    r.pred = sh.band == 0 ? F.pred_root : 0;     /* codec/coder.c:743-745,805-806 */
    r.delta = 0;
#endif
    sh.sp = 0;
}

/* a band of the frame is finished (codec/coder.c:738-833): record it, start the next one.
 * Returns 0 when the frame is complete (or has failed). */
__device__ int band_advance(DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    if (!sh.after_chroma) {
        const SFrame &r = sh.st[0];
        const Range &rg = r.rg;
        const int band = sh.band;
        if (band == 0) {
            F.costs = r.ret; F.err = rg.err; F.tree_bits = rg.tree_bits;
            F.matrix_bits = rg.matrix_bits; F.weights_bits = rg.weights_bits;
            F.root_state = rg.tree;
        } else {
            F.c_costs[band - 1] = r.ret; F.c_err[band - 1] = rg.err;
            F.c_tree_bits[band - 1] = rg.tree_bits; F.c_matrix_bits[band - 1] = rg.matrix_bits;
            F.c_weights_bits[band - 1] = rg.weights_bits;
        }
        if (sh.failed) return 0;
        if (rg.tree == RANGE_) { sh.failed = FC_ERR_NOROOT; return 0; }
        if (!F.color) return 0;
        sh.tree_band[band] = rg.tree;
        if (band == 1) {
            if (!append_join_state(F, sh, sh.tree_band[0], sh.tree_band[1], F.level + 1)) return 0;
            sh.tree_band[1] = sh.states - 1;             /* from here on: the Y+Cb state */
        }
        if (band == 2) {
            if (!append_join_state(F, sh, sh.tree_band[2], RANGE_, F.level + 1)) return 0;
            if (!append_join_state(F, sh, sh.tree_band[1], sh.states - 1, F.level + 2)) return 0;
            F.root_state = sh.states - 1;
            return 0;
        }
        sh.band = band + 1;
        if (band == 0) { sh.op = OP_CHROMA; sh.after_chroma = 1; return 1; }
    }
    sh.after_chroma = 0;
    sh.op = OP_NOP;
    push_root(F, sh, sh.tree_band[0]);
    return 1;
}

#if FC_SPEC
/* The chain raises `epoch` and then reads `busy`; a verifier counts itself into `busy` and then reads
 * `epoch`: a store followed by a load of ANOTHER word on each side (Dekker).  Release / acquire alone
 * order neither pair; a sequentially consistent fence between the two accesses does -- at least one of
 * the two sides then sees the other's write, so either the verifier drops the block or the chain waits
 * for it.  (Before round 4 this held only because both words share a cache line of FcSpecCtl.) */
#define SPEC_DEKKER_FENCE() __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent")
#define SPEC_TIMEOUT_TICKS 20000000ull      /* 0.2 s of the 100 MHz wall clock: then the chain does the block itself */
/* Chain, lane 0: consume the verdicts that have arrived, in block order.  `drain`: wait for all of
 * them (end of the frame); otherwise wait only while every checkpoint slot is taken.  Returns 0, or 1 +
 * the checkpoint slot the chain has to go back to.  (Called from the workgroup's operation loop, not from
 * the partition search: a call inside serial_advance() costs every one of its invocations the saving
 * and restoring of registers through scratch memory -- 7 % of a frame, measured.) */
__device__ __noinline__ int spec_poll(Sh &sh, bool drain)
{
    Sh::SpecLocal &sl = sh.sl;
    FcSpecCtl *c = sl.ctl;
    unsigned long long t0 = 0;
    if (sl.learn != 0.0f) { sl.mlc = sl.nlc ? 0.9f * sl.mlc + 0.1f * sl.learn : sl.learn; sl.nlc++; sl.learn = 0.0f; }
    while (sl.commit != sl.head) {
        const unsigned slot = sl.commit % FC_SPEC_W;
        const bool mine = (sl.spec_mask >> slot) & 1u;
        if (!mine) { sl.commit++; t0 = 0; continue; }     /* searched here anyway: whatever the verifier says */
        /* relaxed: the word guards no data (an acquire would drop the chain's L1 at every look; what a
         * return reads is the chain's own checkpoint, behind a fence of its own) */
        const unsigned v = __hip_atomic_load(&c->verdict[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((v >> 11) != sl.commit + 1) {                  /* not there yet */
            if (!drain && sl.head - sl.commit < FC_SPEC_W) {
                __hip_atomic_store(&c->committed, sl.commit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return 0;
            }
            const unsigned long long now = wall_clock64();
            if (!t0) t0 = now;
            if (now - t0 < SPEC_TIMEOUT_TICKS) { __builtin_amdgcn_s_sleep(16); continue; }
            sl.t_wait += now - t0;
            sl.n_timeout++;                                /* no verifier in sight: the chain is not held up by it */
        } else {
            if (t0) { sl.t_wait += wall_clock64() - t0; t0 = 0; }
            if ((v & 3u) == 1u) {
                /* colour: every state the block's search appended (and removed again) had its y_column
                 * flags written -- zeros, in the luminance band (codec/subdivide.c:560-567) -- under the id it
                 * had in the chain's numbering; the flags outlive the states (codec/wfalib.c:283-309) and
                 * the stream shows them.  The verifier used ids of its own and wrote nothing: here, for as
                 * many ids as its search ever used. */
                if (sh.par.color) {
                    GLOBAL_AS uint8_t *yc = (GLOBAL_AS uint8_t *) sh.par.at_ycol;
                    const unsigned used = (v >> 2) & 63u, s0 = sl.sk[slot];
                    for (unsigned j = 0; j < used; j++) { yc[s0 + j] = 0; yc[(unsigned) sh.par.PA + s0 + j] = 0; }
                }
                sl.mlc = sl.nlc ? 0.9f * sl.mlc + 0.1f * sl.lin[slot] : sl.lin[slot]; sl.nlc++;
                sl.commit++; sl.n_confirmed++;
                continue;
            }
            sl.n_wrong++;
            /* take over the verifier's state -- unless the states its search appended do not fit below the
             * verifiers' ids any more: then the chain searches the block itself and runs out of ids the
             * ordinary way (FC_ERR_CAPACITY, the host stages the frame again with more) */
            if ((v & 3u) == 3u && sl.sk[slot] + ((v >> 2) & 63u) <= (unsigned) sh.cap)
                return (1 + (int) slot) | 0x100 | (int) (((v >> 2) & 63u) << 16) | (int) (((v >> 8) & 7u) << 24);
        }
        return 1 + (int) slot;
    }
    /* (verifiers that wait with a result the chain did not ask for -- a block it searched itself -- go on) */
    __hip_atomic_store(&c->committed, sl.commit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return 0;
}
#endif

#if FC_SPEC
/* Chain, lane 0, end of the luminance band of a colour frame: the chroma bands number their states on
 * into the verifiers' id ranges.  No block search may start from here on (epoch), none may still be
 * running (a verifier looks at the epoch every few operations). */
__device__ __noinline__ void spec_luminance_done(Sh &sh)
{
    FcSpecCtl *c = sh.sl.ctl;
    sh.sl.epoch++;
    __hip_atomic_store(&c->epoch, sh.sl.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    SPEC_DEKKER_FENCE();
    const unsigned long long t0 = wall_clock64();
    while (__hip_atomic_load(&c->busy, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (wall_clock64() - t0 > 100000000ull) { sh.failed = FC_ERR_INTERNAL; break; }     /* 1 s */
        __builtin_amdgcn_s_sleep(32);
    }
    sh.sl.on = 0; sh.sl.mode = 0;        /* no more guesses: the chroma bands are searched by the chain ... */
    sh.sl.chroma_tabs = c->n_tabs > c->n_blocks;      /* ... with tables from all the other workgroups (OP_CHROMA) */
}
#endif

/* One transition of the state machine per call; 1 = call again, 0 = sh.op holds the next parallel
 * operation (or OP_DONE).  One transition per call on purpose: as a loop inside one function the
 * compiler hoists every constant and LDS address of every phase into registers for the whole
 * loop, ~120 VGPRs, and the function then saves and restores 48 callee-saved registers through
 * scratch memory on every call (a memory round trip on the serial path, ~100 k times per frame). */
#ifndef FC_SERIAL_LOOP
#define FC_SERIAL_LOOP 0
#endif
/* sp / phase: the stack pointer and the phase of the frame on top of the stack, held by the caller
 * (in registers across the transitions of one serial_advance()); in memory the stack pointer is
 * current between calls of serial_advance(), the phase of a frame while it is not on top */
__device__ __forceinline__ int serial_step(DevFrame &__restrict__ F, Sh &__restrict__ sh, int &sp, int &phase)
{
    const int ML = sh.par.ML;
    {
#if FC_SPEC
        /* what this workgroup is: 0 one workgroup per frame (or a chain that guesses no more), 1 a chain
         * that guesses, 2 + floor a verifier.  Read afresh in every transition: a plain read is hoisted
         * out of the loop of transitions (FC_SERIAL_LOOP) and then lives in a register of its own for
         * the whole of serial_advance() -- one more callee-saved register to save and restore through
         * scratch memory per call, three calls per range */
        const int spec_mode = *(volatile int *) &sh.sl.mode;
#endif
        if (sp < 0) {
            sh.sp = sp;
#if FC_SPEC
            if (spec_mode == 1) {                /* end of the band: every verdict, then no more guesses */
                sh.op = OP_SPEC_CKPT; sh.a0 = 2;
                return 0;
            }
#endif
            const int more = band_advance(F, sh);        /* may push the root of the next band */
            sp = sh.sp; phase = sp >= 0 ? sh.st[sp].phase : 0;
            if (!more) { sh.op = OP_DONE; return 0; }
            if (sh.op == OP_CHROMA) return 0;
            return 1;
        }
        SFrame &fr = sh.st[sp];
#ifdef FC_SERIAL_PROFILE
        {   /* developer profile: ticks per phase of the state machine (previous phase ends here) */
            unsigned long long t = wall_clock64();
            sh.tk_ph[sh.ph_prev] += t - sh.ph_t0; sh.ph_t0 = t; sh.ph_prev = phase;
        }
#endif
        switch (phase) {
        case PH_ENTER: {
            Range &rg = fr.rg;
            rg.into[0] = NOEDGE;
            rg.tree = RANGE_;
            fr.ret = MAXCOSTS;
            if (sh.failed || rg.level < 3) { fr.ret = MAXCOSTS; goto pop; }
            if (rg.x >= sh.par.width || rg.y >= sh.par.height) { fr.ret = 0; goto pop; }
#if FC_SPEC
            /* entry of a block of the largest block level: verdicts that have arrived, then the
             * checkpoint of this block (OP_SPEC_CKPT; the node is entered again afterwards) */
#endif
            fr.price = sh.par.price;
            if (sh.band) fr.price *= sh.par.chroma_decrease;
#if FC_VARIANT_BIG
            /* try_nd / try_mc (codec/subdivide.c:141-154) */
            fr.try_pred = 0;
            if (fr.pred && rg.level >= F.p_min && rg.level <= F.p_max) {
                if (F.frame_type == 0) fr.try_pred = 1;
                else if (rg.x + (int) width_of_level(rg.level) <= sh.par.width
                         && rg.y + (int) height_of_level(rg.level) <= sh.par.height) fr.try_pred = 2;
            }
            fr.pred_done = 0;
            fr.norm_first = 1; fr.norm_done = 0;     /* clear_norms_table, folded into the first update */
#endif
            phase = PH_AFTER_INIT;
            if (rg.level == sh.par.lc_max) {
                rg.address = rg.image = 0;
                sh.op = OP_INIT_RANGE; sh.a0 = rg.x; sh.a1 = rg.y;
#if FC_SPEC
                sh.a2 = (!sh.band || sh.sl.chroma_tabs) ? sh.blk++ : -1;      /* index of the block in the host's list (+ blocks per band) */
#endif
                return 0;
            }
            break;
        }
        case PH_AFTER_INIT: {
            Range &rg = fr.rg;
#if FC_SPEC
            /* a block of the largest block level, its tables done: verdicts that have arrived, then
             * the checkpoint of this block (OP_SPEC_CKPT; the phase is entered again afterwards) */
            if (spec_mode == 1 && rg.level == sh.par.lc_max && !sh.band && !fr.ckpt && sp > 0) {
                fr.ckpt = 1; sh.op = OP_SPEC_CKPT; sh.a0 = 1;        /* the operation sets ckpt = 2 if it takes a checkpoint */
                return 0;
            }
#endif
            /* A range that cannot be subdivided needs no model snapshots at all: a rejected
             * linear combination leaves every model untouched (codec/approx.c:264-268), an
             * accepted one is exactly the state to continue from, and the tree model is not
             * touched without children -- the reference's duplicate/restore pairs
             * (codec/subdivide.c:188-237,404-468) are no-ops for it. */
            fr.leaf = rg.level <= sh.lc_min && rg.level <= sh.par.lc_max;
#if FC_VARIANT_BIG
            if (fr.try_pred) fr.leaf = 0;       /* predict_range goes back to the entry models */
#endif
            /* the snapshots around a linear-combination search are taken by all lanes inside
             * OP_APPROX (snap_coop_*), not by this one */
            fr.coop = !fr.leaf && rg.level <= sh.par.lc_max;
            if (!fr.leaf && !fr.coop) {
                fr.pool0 = sh.pool;
                snap_save(F, sh, sp, 0);
                tm_save(sh, sp, ML);
#if FC_GM
                fr.rn0 = sh.dpool.n;
                gq_save(sh, 0, sp, 0);
#endif
#if FC_VARIANT_BIG
                if (sh.nslot == 5 && !fr.delta) {
                    fr.dpool0 = sh.dpool; snap_save_d(sh, sp, 2);
#if FC_GM
                    gq_save(sh, 1, sp, 2);
#endif
                }
#endif
            }
            fr.states = sh.states;
            for (int l = 0; l < 2; l++)                 /* codec/subdivide.c:167-173 */
                fr.ny[l] = (sh.band && fr.y_state != RANGE_) ? (int) TREE(F, fr.y_state, l) : RANGE_;
            phase = PH_AFTER_LC;
            if (rg.level <= sh.par.lc_max) {
                fr.lrange = rg;
                fr.lrange.tree = RANGE_;
#if FC_VARIANT_BIG
                fr.lrange.tree_bits = tree_bits_dev(sh, ML, 0, rg.level, 0);
#endif                              /* default build: priced by an idle lane of OP_APPROX (mp_tables, sh.tb) */
                fr.lrange.matrix_bits = 0;
                fr.lrange.weights_bits = 0;
#if FC_VARIANT_BIG
                fr.lrange.nd_tree_bits = 0; fr.lrange.nd_weights_bits = 0; fr.lrange.prediction = 0;
                fr.lrange.mv_tree_bits = fr.try_pred == 2 ? 1.0f : 0.0f;   /* mc allowed but not used */
                fr.lrange.mv_coord_bits = 0;
#endif
                sh.op = OP_APPROX;
                return 0;
            }
            fr.lincomb = MAXCOSTS;
            break;
        }
        case PH_AFTER_LC: {
            Range &rg = fr.rg;
            if (fr.leaf) {
                fr.subdiv = MAXCOSTS;
                phase = PH_DECIDE;
                break;
            }
            if (!fr.coop) {
#if FC_VARIANT_BIG
                fr.pool_lc = sh.pool;
                snap_save(F, sh, sp, 1);
#if FC_GM
                gq_save(sh, 0, sp, 1);
#endif
                sh.pool = fr.pool0;
                snap_load(F, sh, sp, 0);
#if FC_GM
                gq_load(sh, 0, sp, 0);
                if (fr.delta) sh.dpool.n = (unsigned short) fr.rn0;
#endif
#else
                /* a node above the largest block level: no linear combination has touched the
                 * models since the snapshot of its entry */
                fr.pool_lc = sh.pool;
#endif
            }
#if FC_SPEC
            if (fr.ckpt == 3) {                  /* the guess (spec_guess, end of OP_APPROX): the combination wins */
                fr.subdiv = MAXCOSTS;
                phase = PH_DECIDE;
                break;
            }
#endif
            if (rg.level > sh.lc_min) {
                Range z;
                z.x = z.y = z.image = z.address = z.level = 0; z.tree = 0;
                for (int i = 0; i < RANGE_E; i++) { z.weight[i] = 0; z.into[i] = 0; }
                z.err = z.tree_bits = z.matrix_bits = z.weights_bits = 0;
#if FC_VARIANT_BIG
                z.nd_tree_bits = z.nd_weights_bits = z.mv_tree_bits = z.mv_coord_bits = 0; z.prediction = 0;
                for (int i = 0; i < 5; i++) z.mv[i] = 0;
#endif
                fr.child[0] = z; fr.child[1] = z;
                fr.rrange = rg;
#if FC_VARIANT_BIG
                fr.rrange.tree_bits = tree_bits_dev(sh, ML, 1, rg.level, 0);
#else
                /* the tree model has not changed since the node's OP_APPROX priced both symbols
                 * (only finished children update it) */
                fr.rrange.tree_bits = rg.level <= sh.par.lc_max ? sh.tb[1] : tree_bits_dev(sh, ML, 1, rg.level, 0);
#endif
                fr.rrange.matrix_bits = 0;
                fr.rrange.weights_bits = 0;
                fr.rrange.err = 0;
#if FC_VARIANT_BIG
                /* codec/subdivide.c:257-271 */
                fr.rrange.mv_tree_bits = fr.try_pred == 2 ? 1.0f : 0.0f;
                fr.rrange.mv_coord_bits = 0;
                fr.rrange.nd_tree_bits = fr.try_pred == 1 ? tree_bits_dev(sh, ML, 1, rg.level, 1) : 0.0f;
                fr.rrange.nd_weights_bits = 0;
                fr.rrange.prediction = 0;
                fr.subdiv = (fr.rrange.tree_bits + fr.rrange.weights_bits + fr.rrange.matrix_bits
                             + fr.rrange.mv_tree_bits + fr.rrange.mv_coord_bits + fr.rrange.nd_tree_bits
                             + fr.rrange.nd_weights_bits) * fr.price;
#else
                fr.subdiv = (fr.rrange.tree_bits + fr.rrange.weights_bits + fr.rrange.matrix_bits) * fr.price;
#endif
                fr.label = 0;
                phase = PH_CHILD;
            } else {
                fr.subdiv = MAXCOSTS;
                phase = PH_DECIDE;
            }
            break;
        }
        case PH_CHILD: {
            const Range &rr = fr.rrange;
            const int label = fr.label;
            Range &ch = fr.child[label];
            ch.image = rr.image * 2 + label + 1;
            ch.address = rr.address * 2 + label;
            ch.level = rr.level - 1;
            ch.x = (rr.level & 1) ? rr.x : rr.x + label * (int) width_of_level(rr.level - 1);
            ch.y = (rr.level & 1) ? rr.y + label * (int) height_of_level(rr.level - 1) : rr.y;
            phase = PH_CHILD2;
            if (label && rr.level <= sh.par.lc_max && sh.states > fr.states && !sh.band) {
                sh.op = OP_IPIS_INCR; sh.a0 = ch.image; sh.a1 = ch.address; sh.a2 = ch.level;
                sh.a3 = fr.states;
                return 0;
            }
            break;
        }
        case PH_CHILD2: {
            float lim = fr.lincomb > fr.max_costs ? fr.max_costs : fr.lincomb;
            float remaining = lim - fr.subdiv;
            phase = PH_CHILD_RET;
            fr.ret = 0;
            if (remaining > 0) {
                if (sp + 1 >= FC_DEPTH) { sh.failed = FC_ERR_INTERNAL; break; }
                SFrame &cf = sh.st[sp + 1];
                cf.rg = fr.child[fr.label];
                cf.y_state = fr.ny[fr.label];
                cf.max_costs = remaining;
                cf.phase = PH_ENTER;
#if FC_SPEC
                cf.ckpt = 0;
#endif
#if FC_VARIANT_BIG
                cf.pred = fr.pred; cf.delta = fr.delta;
#endif
                fr.phase = phase; sp++; phase = PH_ENTER;   /* this frame rests: its phase goes to memory */
                break;                              /* child result arrives in fr.ret */
            }
            fr.ret = -1;                            /* marker: no recursion happened */
            break;
        }
        case PH_CHILD_RET: {
            const int label = fr.label;
            float lim = fr.lincomb > fr.max_costs ? fr.max_costs : fr.lincomb;
#if FC_VARIANT_BIG
            if (fr.try_pred == 2 && !fr.norm_done) {
                /* a child that was not searched gets its displacement table here
                 * (subdivide.c:311-315); then update_norms_table (:317-318) */
                const Range &c0 = fr.child[label];
                sh.op = OP_NORMS; sh.a0 = fr.rg.level; sh.a1 = fr.norm_first;
                sh.a2 = (fr.ret < 0 && c0.level >= F.p_min) ? c0.level : -1;
                sh.a3 = c0.x | (c0.y << 16);
                fr.norm_first = 0; fr.norm_done = 1;
                return 0;
            }
            fr.norm_done = 0;
#endif
            if (fr.ret >= 0) fr.subdiv += fr.ret;
            if (fr.subdiv >= lim) {
                fr.subdiv = MAXCOSTS;
                phase = PH_DECIDE;
                break;
            }
            const Range &ch = fr.child[label];
            fr.rrange.err          += ch.err;
            fr.rrange.tree_bits    += ch.tree_bits;
            fr.rrange.matrix_bits  += ch.matrix_bits;
            fr.rrange.weights_bits += ch.weights_bits;
#if FC_VARIANT_BIG
            fr.rrange.mv_tree_bits    += ch.mv_tree_bits;
            fr.rrange.mv_coord_bits   += ch.mv_coord_bits;
            fr.rrange.nd_weights_bits += ch.nd_weights_bits;
            fr.rrange.nd_tree_bits    += ch.nd_tree_bits;
            tree_update_dev(sh, ML, ch.tree != RANGE_, ch.level, 0);
            tree_update_dev(sh, ML, !ch.prediction, ch.level, 1);     /* subdivide.c:371-372 */
#else
            /* (the second tree model, codec/subdivide.c:371-372, prices nothing without prediction and is
             * not part of the default build's snapshots: not kept) */
            tree_update_dev(sh, ML, ch.tree != RANGE_, ch.level, 0);
#endif
            fr.label = label + 1;
            phase = fr.label < 2 ? PH_CHILD : PH_DECIDE;
            break;
        }
        case PH_DECIDE: {
            Range &rg = fr.rg;
#if FC_SPEC
            if (spec_mode >= 2 && sp == spec_mode - 2) {
                /* the verifier's block: all the chain needs to know is whether the combination wins
                 * (the branch `lincomb < subdiv` below) */
                sh.sl.verdict = (!sh.failed && !fr.leaf && fr.lincomb < MAXCOSTS && fr.lincomb < fr.subdiv) ? 1 : 2;
                /* 3: the subdivision wins (the last branch below).  The chain need not search the block
                 * again: it takes over this workgroup's state as it stands here (OP_SPEC_CKPT) */
                if (!sh.failed && !fr.leaf && fr.subdiv < MAXCOSTS && !(fr.lincomb < fr.subdiv)) sh.sl.verdict = 3;
                sh.op = OP_DONE;
                return 0;
            }
#endif
#if FC_VARIANT_BIG
            if (fr.try_pred && !fr.pred_done && !sh.failed) { phase = PH_PRED_BEGIN; break; }
#endif
            if (fr.leaf) {                       /* models are already what they have to be */
                if (fr.lincomb < MAXCOSTS) { rg = fr.lrange; fr.ret = fr.lincomb; }
                else fr.ret = MAXCOSTS;
                goto pop;
            } else if (fr.lincomb >= MAXCOSTS && fr.subdiv >= MAXCOSTS) {
                sh.pool = fr.pool0;
                snap_load(F, sh, sp, 0);
                tm_load(sh, sp, ML);
#if FC_GM
                gq_load(sh, 0, sp, 0);
                if (fr.delta) sh.dpool.n = (unsigned short) fr.rn0;
#endif
#if FC_VARIANT_BIG
                if (sh.nslot == 5 && !fr.delta) {
                    sh.dpool = fr.dpool0; snap_load_d(sh, sp, 2);
#if FC_GM
                    gq_load(sh, 1, sp, 2);
#endif
                }
#endif
                sh.states = fr.states;
                if (sh.flim > sh.states) sh.flim = sh.states & ~(GRAM_FB - 1);
                fr.ret = MAXCOSTS;
                goto pop;
            } else if (fr.lincomb < fr.subdiv) {
#if FC_SPEC
                if (fr.ckpt == 2 && spec_mode == 1) sh.sl.learn = fr.lincomb;    /* searched here, kept its combination */
#endif
                sh.pool = fr.pool_lc;
                snap_load(F, sh, sp, 1);
                tm_load(sh, sp, ML);
#if FC_GM
                gq_load(sh, 0, sp, 1);
                if (fr.delta) sh.dpool.n = (unsigned short) fr.rn0;
#endif
#if FC_VARIANT_BIG
                /* the linear combination left the resting models as they were at the entry */
                if (sh.nslot == 5 && !fr.delta) {
                    sh.dpool = fr.dpool0; snap_load_d(sh, sp, 2);
#if FC_GM
                    gq_load(sh, 1, sp, 2);
#endif
                }
#endif
                rg = fr.lrange;
                sh.states = fr.states;
                if (sh.flim > sh.states) sh.flim = sh.states & ~(GRAM_FB - 1);
                fr.ret = fr.lincomb;
                goto pop;
            } else {
                int aux = sh.band > 0 || rg.x + (int) width_of_level(rg.level) > sh.par.width
                          || rg.y + (int) height_of_level(rg.level) > sh.par.height;
#if FC_VARIANT_BIG
                /* with a second rle pool as delta pool a state that neither pool takes keeps no
                 * tables (codec/subdivide.c:571-583,607; the constant pool takes every state) */
#if FC_GM
                /* ... in general: a state that neither pool takes (without prediction the delta pool is the
                 * constant pool, which takes everything) */
                if (!(gm_accepts(sh.pool, sh.gm.pk[0]) || !F.pred_on || gm_accepts(sh.dpool, sh.gm.pk[1]))) aux = 1;
#else
                if (F.pred_on && sh.pool.n >= sh.pool.max_domains) aux = 1;
#endif
#endif
#if FC_SPEC
                /* (volatile: see spec_mode) */
                if (sh.states >= (sh.band ? sh.par.PA : *(volatile int *) &sh.cap)) { sh.failed = FC_ERR_CAPACITY; fr.ret = MAXCOSTS; goto pop; }
#else
                if (sh.states >= (sh.band ? sh.par.PA : sh.par.P)) { sh.failed = FC_ERR_CAPACITY; fr.ret = MAXCOSTS; goto pop; }
#endif
                store_new_state(F, sh, fr, aux);
                phase = PH_AFTER_APPEND;
                if (!aux) { sh.op = OP_APPEND; sh.a0 = sh.states; return 0; }
                break;
            }
        }
#if FC_SPEC
        case PH_SPEC_END: {                  /* a verifier's block has left the stack without a verdict (not reached:
                                              * it ends in PH_DECIDE of the block): the chain does the block itself */
            sh.sl.verdict = 2; sh.op = OP_DONE;
            return 0;
        }
#endif
        case PH_AFTER_APPEND: {
            sh.states++;
#if FC_SPEC
            if (sh.states - *(volatile int *) &sh.gap_shift >= sh.par.limit_states) sh.failed = FC_ERR_STATES;
#else
            if (sh.states >= sh.par.limit_states) sh.failed = FC_ERR_STATES;
#endif
            fr.rg = fr.rrange;
            fr.ret = fr.subdiv;
            goto pop;
        }
#if FC_VARIANT_BIG
        case PH_PRED_BEGIN: {                /* predict_range + nd_prediction, prediction.c:96-150,371-404 */
            Range &rg = fr.rg;
            const int il = sh.par.images_level, P = sh.par.P;
            float maxc = fr.lincomb > fr.subdiv ? fr.subdiv : fr.lincomb;
            if (maxc > fr.max_costs) maxc = fr.max_costs;
            fr.pred_done = 1;
            fr.pred_max = maxc;
            fr.rec_states = sh.states;
            /* what the recursion left behind */
            fr.pool_rec = sh.pool; fr.dpool_rec = sh.dpool;
            snap_save(F, sh, sp, 3); snap_save_d(sh, sp, 4); tm_save(sh, sp, ML, 1);
#if FC_GM
            gq_save(sh, 0, sp, 3); gq_save(sh, 1, sp, 4);
#endif
            /* back to the models of the entry */
            sh.pool = fr.pool0; sh.dpool = fr.dpool0;
            snap_load(F, sh, sp, 0); snap_load_d(sh, sp, 2); tm_load(sh, sp, ML, 0);
#if FC_GM
            gq_load(sh, 0, sp, 0); gq_load(sh, 1, sp, 2);
#endif
            sh.states = fr.states;
            if (sh.flim > sh.states) sh.flim = sh.states & ~(GRAM_FB - 1);
            if (fr.try_pred == 2) {          /* mc_prediction, prediction.c:262-289 */
                sh.op = OP_MC_SEARCH; sh.a0 = rg.level; sh.a1 = rg.x | (rg.y << 16);
                sh.a2 = (rg.level == F.p_min ? 1 : 0) | (rg.level > F.p_min && fr.norm_first ? 2 : 0);
                phase = PH_PRED_MC2;
                return 0;
            }
            {   /* the range's DC part in the DC format of the normal model */
                const float x = rg.level > il ? sh.par.ipis[(size_t) rg.image * P]
                                              : (rg.level == il ? sh.par.d5 : sh.par.d4)[(size_t) rg.address * P];
                const float y = sh.par.diag[(size_t) (rg.level - sh.par.gl0) * P];
                const int sym = rtob_dev(x / y, sh.par.dc_mant, sh.par.dc_range);
                const int cnt = sym < 0 ? 0 : (int) sh.cb.cnt[sym];      /* RPF_ZERO: see coeff_bits of the oracle */
                fr.nd_w = btor_fast(sym, sh.par.dc_mant, sh.par.dc_range);
                fr.nd_tbits = tree_bits_dev(sh, ML, 0, rg.level, 1);
                fr.nd_wbits = (float) (0.0 - log2((double) (cnt / (float) sh.cb.tot[0])));
#if FC_GM
                if (sh.gm.ck[0] == FC_CK_UNIFORM) fr.nd_wbits = (float) (sh.par.dc_mant + 1);     /* uniform_bits, codec/coeff.c:155-170 */
#endif
            }
            fr.pred_costs = fr.price * (fr.nd_wbits + fr.nd_tbits);
            phase = PH_PRED_GO;
            break;
        }
        case PH_PRED_MC2: {                  /* find_P_frame_mc done: vector in sh.mc (prediction.c:282-289) */
            fr.prange = fr.rg;
            fr.prange.mv[0] = (short) sh.mc.type; fr.prange.mv[1] = (short) sh.mc.fx; fr.prange.mv[2] = (short) sh.mc.fy;
            fr.prange.mv[3] = (short) sh.mc.bx; fr.prange.mv[4] = (short) sh.mc.by;
            fr.prange.mv_tree_bits = sh.mc.tree_bits; fr.prange.mv_coord_bits = sh.mc.bits;
            fr.nd_tbits = sh.mc.tree_bits; fr.nd_wbits = sh.mc.bits;      /* mvt, mvc kept for PH_PRED_DONE */
            fr.pred_costs = (fr.prange.mv_tree_bits + fr.prange.mv_coord_bits) * fr.price;
            phase = PH_PRED_GO;
            break;
        }
        case PH_PRED_GO: {
            if (fr.pred_costs < fr.pred_max) {
                if (fr.rec_states - fr.states > F.max_save || sp + 1 >= FC_DEPTH) { sh.failed = FC_ERR_INTERNAL; }
                else {
                    sh.op = OP_PRED_SETUP; sh.a0 = fr.rg.level; sh.a1 = fr.rg.address;
                    phase = PH_PRED_RECURSE;
                    return 0;
                }
            }
            /* no residual search: everything back as the recursion left it */
            sh.pool = fr.pool_rec; sh.dpool = fr.dpool_rec;
            snap_load(F, sh, sp, 3); snap_load_d(sh, sp, 4); tm_load(sh, sp, ML, 1);
#if FC_GM
            gq_load(sh, 0, sp, 3); gq_load(sh, 1, sp, 4);
#endif
            sh.states = fr.rec_states;
            fr.rg.prediction = 0;
            phase = PH_DECIDE;
            break;
        }
        case PH_PRED_RECURSE: {              /* subdivide (max_costs - costs, ..., NO, YES), :432-456 */
            SFrame &cf = sh.st[sp + 1];
            cf.rg = fr.rg;
            if (fr.try_pred == 2) for (int i = 0; i < 5; i++) cf.rg.mv[i] = fr.prange.mv[i];
            cf.rg.tree_bits = cf.rg.matrix_bits = cf.rg.weights_bits = 0;
            cf.rg.nd_tree_bits = cf.rg.nd_weights_bits = cf.rg.mv_tree_bits = cf.rg.mv_coord_bits = 0;
            cf.rg.image = 0; cf.rg.address = 0;
            cf.y_state = fr.y_state;
            cf.max_costs = fr.pred_max - fr.pred_costs;
            cf.phase = PH_ENTER;
            cf.pred = 0; cf.delta = 1;
            fr.phase = PH_PRED_RET;
            sp++; phase = PH_ENTER;
            break;
        }
        case PH_PRED_RET: {
            const float costs = fr.pred_costs + fr.ret;
            /* nd: only a subdivided residual counts (:460); mc: any (:329) */
            const int keep = !sh.failed && costs < fr.pred_max && (fr.try_pred == 2 || fr.prange.tree != RANGE_);
            fr.pred_costs = costs;
            sh.op = OP_PRED_FINISH; sh.a0 = keep;
            phase = PH_PRED_DONE;
            fr.label = keep;                 /* remembered for PH_PRED_DONE */
            return 0;
        }
        case PH_PRED_DONE: {
            Range &rg = fr.rg;
            if (fr.label) {                  /* use the prediction, prediction.c:460-485,152-180 */
                const int img = rg.image, adr = rg.address;
                const float mvt = fr.try_pred == 2 ? fr.nd_tbits : 0.0f, mvc = fr.try_pred == 2 ? fr.nd_wbits : 0.0f;
                rg = fr.prange;
                rg.image = img; rg.address = adr;
                if (fr.try_pred == 2) {      /* prediction.c:333-340 */
                    rg.mv_coord_bits = mvc; rg.mv_tree_bits = mvt;
                } else {
                    rg.nd_tree_bits += fr.nd_tbits;
                    rg.nd_weights_bits += fr.nd_wbits;
                    rg.into[0] = 0; rg.weight[0] = fr.nd_w; rg.into[1] = NOEDGE;
                }
                rg.prediction = 1;
                if (sh.flim > sh.states) sh.flim = sh.states & ~(GRAM_FB - 1);
                fr.ret = (rg.tree_bits + rg.matrix_bits + rg.weights_bits + rg.mv_tree_bits + rg.mv_coord_bits
                          + rg.nd_tree_bits + rg.nd_weights_bits) * fr.price + rg.err;
                goto pop;
            }
            sh.pool = fr.pool_rec; sh.dpool = fr.dpool_rec;
            snap_load(F, sh, sp, 3); snap_load_d(sh, sp, 4); tm_load(sh, sp, ML, 1);
#if FC_GM
            gq_load(sh, 0, sp, 3); gq_load(sh, 1, sp, 4);
#endif
            sh.states = fr.rec_states;
            {   /* columns of ids the residual search used are stale in older rows */
                const int lim = fr.states & ~(GRAM_FB - 1);
                if (sh.flim > lim) sh.flim = lim;
            }
            rg.prediction = 0;
            phase = PH_DECIDE;
            break;
        }
#endif
        }
        return 1;
    pop:
        if (sp > 0) {
            SFrame &pf = sh.st[sp - 1];
#if FC_VARIANT_BIG
            if (pf.phase == PH_PRED_RET) pf.prange = fr.rg;
            else
#endif
            pf.child[pf.label] = fr.rg;
            pf.ret = fr.ret;
        }
        sp--;
        if (sp >= 0) phase = sh.st[sp].phase;
    }
    return 1;
}

/* advance the partition search until a data-parallel operation is required */
#if FC_SERIAL_LOOP
__device__ __noinline__ void serial_advance(DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    int sp = sh.sp, phase = sp >= 0 ? sh.st[sp].phase : 0;
    while (serial_step(F, sh, sp, phase))
        ;
    sh.sp = sp;
    if (sp >= 0) sh.st[sp].phase = phase;
}
#else
/* One transition per out-of-line call on purpose (builds with machine LICM): as a loop inside one
 * function the compiler hoists every constant and LDS address of every phase into registers for the
 * whole loop, ~120 VGPRs, and the function then saves and restores 48 callee-saved registers
 * through scratch memory on every call. */
__device__ __noinline__ int serial_step_call(DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    int sp = sh.sp, phase = sp >= 0 ? sh.st[sp].phase : 0;
    const int r = serial_step(F, sh, sp, phase);
    sh.sp = sp;
    if (sp >= 0) sh.st[sp].phase = phase;
    return r;
}
__device__ __forceinline__ void serial_advance(DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    while (serial_step_call(F, sh))
        ;
}
#endif
