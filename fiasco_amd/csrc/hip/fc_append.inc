/*
 *  fc_append.inc -- the tables of a new state: its Gram rows (append_row_part), op_append; the
 *  domain pool of the chroma bands (op_chroma_pool).
 *
 *  Reference: state tables codec/control.c:48-131,205-258; inner-product tables codec/ip.c:46-323;
 *  rle pool codec/domain-pool.c:621-852, rle_chroma :854-879.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

#if FC_VARIANT_BIG
__device__ void pred_save_tables(DevFrame &__restrict__ F, Sh &__restrict__ sh, int s);
__device__ void subtract_mc_dev(DevFrame &__restrict__ F, Sh &__restrict__ sh);
#endif

/* Gram row of the new state s at every table level -- the entries t with (t / B) mod parts == part (all of them:
 * part 0 of 1); level q needs level q-1 of states < s.  The term lists of s are in sh.gs_*.  Out of op_append so that
 * the append helpers of a speculating frame (FcSpecCtl.app_*) run the same code on their shares. */
__device__ __forceinline__ void append_row_part(DevFrame &__restrict__ F, Sh &__restrict__ sh, int s, int part, int parts)
{
    const int tid = threadIdx.x, P = F.P;
#if FC_VARIANT_BIG
    const int il = F.images_level;
#endif
    {
        const int flim = __builtin_amdgcn_readfirstlane(sh.flim);
        const int Pu = __builtin_amdgcn_readfirstlane(P);
        s = __builtin_amdgcn_readfirstlane(s);
        const unsigned LS = (unsigned) __builtin_amdgcn_readfirstlane((int) F.gram_ls);   /* floats per table level */
        const unsigned rs = GROW(s, Pu);               /* start of the new state's row in a level */
        GLOBAL_AS float *const gram = uniform_ptr(F.gram);
        GLOBAL_AS float *const diag = uniform_ptr(F.diag);
        AutoTabs T;
        auto_tabs(F, T);
        /* level-images_level image of s (the same for every lane): 32 loads in flight once;
         * per t the other 32.  A `for (k < 1 << images_level)` loop is not unrolled by the
         * compiler and would wait for every single load. */
        GLOBAL_AS const float *imgT = uniform_ptr((const float *) F.imgT);
        float vs[32];
#pragma unroll
        for (int k = 0; k < 32; k++) vs[k] = ldg(imgT, (unsigned) (k * Pu + s));
        for (int t = tid + part * B; t <= s; t += B * parts) {
            EdgeRows rows;
            load_edge_rows(T, t, rows);
            float vt[32];
#pragma unroll
            for (int k = 0; k < 32; k++) vt[k] = ldg(imgT, (unsigned) (k * Pu + t));
            if (!rows.dt || DEAD(sh, t)) continue;
            /* term lists of t in registers (fixed slots: 0 = tree child, 1.. = edges), loaded
             * once and reused by every table level */
            int   i2[2][FC_MAXE + 1];
            float w2[2][FC_MAXE + 1];
            unsigned m2[2];
#pragma unroll
            for (int l = 0; l < 2; l++) {
                int k = rows.tree[l];
                m2[l] = k != RANGE_ ? 1u : 0u;
                i2[l][0] = k != RANGE_ ? k : 0;
                w2[l][0] = 1.0f;
                bool live = true;
#pragma unroll
                for (int e = 0; e < FC_MAXE; e++) {
                    live = live && rows.rd[l][e] != NOEDGE;
                    i2[l][e + 1] = live ? rows.rd[l][e] : 0;
                    w2[l][e + 1] = live ? rows.rw[l][e] : 0.0f;
                    m2[l] |= live ? (2u << e) : 0u;
                }
            }
            /* only the row of s is written here: see gram_flush() */
            int q1 = 1;
#if FC_VARIANT_BIG
            if (F.gl0 < il) {                      /* levels <= images_level: direct dots */
                GLOBAL_AS const float *imgT4 = uniform_ptr((const float *) F.imgT4);
                float a4[16], b4[16], v4 = 0;
#pragma unroll
                for (int k = 0; k < 16; k++) { a4[k] = ldg(imgT4, (unsigned) (k * Pu + s)); b4[k] = ldg(imgT4, (unsigned) (k * Pu + t)); }
#pragma unroll
                for (int k = 0; k < 16; k++) v4 += a4[k] * b4[k];
                stg(gram, rs + (unsigned) t, v4);
                if (s == t) stg(diag, (unsigned) s, v4);
                q1 = 2;
            }
#endif
            {
                float v0 = 0;                         /* codec/ip.c:297-323, sequential */
#pragma unroll
                for (int k = 0; k < 32; k++) v0 += vs[k] * vt[k];
                stg(gram, (unsigned) (q1 - 1) * LS + rs + (unsigned) t, v0);
                if (s == t) stg(diag, (unsigned) ((q1 - 1) * Pu + s), v0);
#if FC_GRAM_TRI
                if (t < FC_TRI_HOT && t < s) F.gcol[((size_t) (q1 - 1) * FC_TRI_HOT + t) * Pu + s] = v0;
#endif
            }
            for (int q = q1; q < F.NL; q++) {
#if FC_VARIANT_BIG
                if (F.bx && t < F.basis_states) {      /* the terms of a basis state: DevFrame.bx */
                    const BxView V = bx_view(F);
                    GLOBAL_AS const float *Gb = gram + (size_t) (q - 1) * LS;
                    float ipb = 0;
                    for (int l = 0; l < 2; l++) {
                        const int na = sh.gs_n[l], ca = sh.gs_c[l];
                        for (int a = 0; a < na; a++) {
                            const int A = sh.gs_idx[l][a];
                            float sum = 0;
                            int d2;
                            for (int e2 = (t * 2 + l) * 6; (d2 = V.into[e2]) != NOEDGE; e2++)
                                sum += V.w[e2] * ldg(Gb, gram_idx(Pu, A, d2, flim));
                            if (a == 0 && ca) ipb += sum;
                            else ipb += sh.gs_w[l][a] * sum;
                        }
                    }
                    stg(gram, (unsigned) q * LS + rs + (unsigned) t, ipb);
                    continue;
                }
#endif
                /* codec/ip.c:213-257: ip = sum_label sum_{a in terms(s)} [w_a *] ( sum_{b in
                 * terms(t)} [w_b *] G_{q-1}[a][b] ); a tree child enters without a multiply.
                 * All gathers of a label (terms(s) x 6 slots of t) are issued before the first
                 * is used; dead term slots of t read a valid dummy entry (no per-lane branch). */
                GLOBAL_AS const float *G = gram + (size_t) (q - 1) * LS;
                float ip = 0;
                float g[2][FC_MAXE + 1][FC_MAXE + 1];
#pragma unroll
                for (int l = 0; l < 2; l++) {                      /* gathers of both labels */
                    const int na = __builtin_amdgcn_readfirstlane(sh.gs_n[l]);
#pragma unroll
                    for (int a = 0; a <= FC_MAXE; a++) {
                        if (a >= na) break;                            /* uniform */
                        const int A = __builtin_amdgcn_readfirstlane(sh.gs_idx[l][a]);
#pragma unroll
                        for (int b = 0; b <= FC_MAXE; b++) {
                            g[l][a][b] = ldg(G, gram_idx(Pu, A, i2[l][b], flim));
                        }
                    }
                }
#pragma unroll
                for (int l = 0; l < 2; l++) {
                    const int na = __builtin_amdgcn_readfirstlane(sh.gs_n[l]);
                    const int ca = __builtin_amdgcn_readfirstlane(sh.gs_c[l]);
#pragma unroll
                    for (int a = 0; a <= FC_MAXE; a++) {
                        if (a >= na) break;
                        float sum = 0;
                        if (m2[l] & 1u) sum = g[l][a][0];
#pragma unroll
                        for (int b = 1; b <= FC_MAXE; b++)
                            if ((m2[l] >> b) & 1u) sum += w2[l][b] * g[l][a][b];
                        if (a == 0 && ca) ip += sum;
                        else ip += sh.gs_w[l][a] * sum;
                    }
                }
                stg(gram, (unsigned) q * LS + rs + (unsigned) t, ip);
                if (s == t) stg(diag, (unsigned) (q * Pu + s), ip);
#if FC_GRAM_TRI
                if (t < FC_TRI_HOT && t < s) F.gcol[((size_t) q * FC_TRI_HOT + t) * Pu + s] = ip;
#endif
            }
        }
    }
}

#if FC_SPEC
/* ... as a call: the shares of a dealt row (chain and append helpers) */
__device__ __noinline__ void append_row_part_ool(DevFrame &__restrict__ F, Sh &__restrict__ sh, int s, int part, int parts)
{
    append_row_part(F, sh, s, part, parts);
}
#endif

/* codec/control.c:48-131 for a non-auxiliary state s whose edges are already stored */
__device__ __noinline__ void op_append(DevFrame &__restrict__ F, Sh &__restrict__ sh, int s)
{
    const int tid = threadIdx.x, il = F.images_level, P = F.P;
#if FC_VARIANT_BIG
    pred_save_tables(F, sh, s);         /* residual search: the id may belong to a displaced state */
#endif
    /* term lists of the new state s (slot 0 = tree child with weight 1 if any, then the
     * edges): twelve lanes read one row slot each (one memory round trip instead of a chain of
     * dependent ones), two lanes compact them into LDS; uniform for the whole workgroup */
#if !FC_VARIANT_BIG
    /* default build: store_new_state() has left the term lists in sh.gs_* */
#else
    if (tid < 12) {
        const int l = tid / 6, e = tid % 6;
        sh.gs_raw_idx[l][e] = e == 0 ? (int) TREE(F, s, l) : (int) INTO(F, s, l, e - 1);
        sh.gs_raw_w[l][e] = e == 0 ? 1.0f : WEIGHT(F, s, l, e - 1);
    }
    __syncthreads();
    if (tid < 2) {
        const int l = tid;
        int m = 0;
        sh.gs_c[l] = sh.gs_raw_idx[l][0] != RANGE_;
        if (sh.gs_c[l]) { sh.gs_idx[l][0] = sh.gs_raw_idx[l][0]; sh.gs_w[l][0] = 1.0f; m = 1; }
        for (int e = 1; e <= MAXED && sh.gs_raw_idx[l][e] != NOEDGE; e++) {
            sh.gs_idx[l][m] = sh.gs_raw_idx[l][e]; sh.gs_w[l][m] = sh.gs_raw_w[l][e]; m++;
        }
        sh.gs_n[l] = m;
        for (; m <= MAXED; m++) { sh.gs_idx[l][m] = 0; sh.gs_w[l][m] = 0.0f; }   /* valid dummies */
    }
    __syncthreads();
#endif
    /* images: level 0 is the final distribution (control.c:97); a level l >= 1 element
     * depends on level l-1 of OTHER states only (codec/control.c:205-258) */
    GLOBAL_AS float *const gimg = uniform_ptr(F.img);
    GLOBAL_AS float *const gimgT = uniform_ptr(F.imgT);
    const int NIu = __builtin_amdgcn_readfirstlane(F.NI);
    if (tid == B - 1) stg(gimg, (unsigned) (s * NIu), F.final_d[s]);
    for (int i = tid; i < NIu - 1; i += B) {
        int l = 31 - __clz(i + 2);                      /* offset 2^l - 1 + pos = i + 1 */
        int pos = i + 1 - ((1 << l) - 1);
        const int half = 1 << (l - 1), label = pos >= half;
        const int off = half - 1 + (pos - label * half);
        const int n = sh.gs_n[label];
        float t[FC_MAXE + 1];
#pragma unroll
        for (int a = 0; a <= FC_MAXE; a++)              /* all term images in flight */
            t[a] = ldg((GLOBAL_AS const float *) gimg, (unsigned) (sh.gs_idx[label][a] * NIu + off));      /* dead slots: state 0 */
        float v = 0;
#pragma unroll
        for (int a = 0; a <= FC_MAXE; a++)
            if (a < n) v = (a == 0 && sh.gs_c[label]) ? t[0] : v + t[a] * sh.gs_w[label][a];
        stg(gimg, (unsigned) (s * NIu + i + 1), v);
        if (l == il) stg(gimgT, (unsigned) (pos * P + s), v);
#if FC_VARIANT_BIG
        if (l == il - 1 && F.gl0 < il) F.imgT4[(size_t) pos * P + s] = v;
#endif
    }
    __syncthreads();
    /* Gram row/column of s at every table level; level q needs level q-1 of states < s */
#if FC_SPEC
    {
        /* a long row of the chain of a frame with append helpers: dealt (FcSpecCtl.app_*) */
        FcSpecCtl *const c = sh.sl.ctl;
        const bool deal = sh.sl.role == 0 && sh.sl.on && c && sh.sl.app_H > 0 && !sh.sl.app_off
                          && (unsigned) (s + 1) >= sh.sl.app_min;                      /* uniform */
        if (!deal) append_row_part(F, sh, s, 0, 1);
        else {
            const unsigned H = sh.sl.app_H;
            WAVE_DRAIN();                       /* images of s, its automaton row: in L2 before the row is published */
            __syncthreads();
            if (tid == 0) {
                c->app_s = s; c->app_flim = sh.flim;
                for (int l = 0; l < 2; l++) {
                    c->app_n[l] = sh.gs_n[l]; c->app_c[l] = sh.gs_c[l];
                    for (int e = 0; e <= MAXED; e++) { c->app_idx[l][e] = sh.gs_idx[l][e]; c->app_w[l][e] = sh.gs_w[l][e]; }
                }
                publish_release();
                __hip_atomic_store(&c->app_seq, ++sh.sl.app_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            append_row_part_ool(F, sh, s, 0, (int) H + 1);
            __syncthreads();
            if (tid == 0) {
                const unsigned want = sh.sl.app_seq * H;
                const unsigned wait_ticks = c->app_wait;
                const unsigned long long t0 = wall_clock64();
                int late = 0;
                while (__hip_atomic_load(&c->app_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != want) {
                    if (wall_clock64() - t0 > wait_ticks) { late = 1; break; }
                    __builtin_amdgcn_s_sleep(1);
                }
                take_acquire();                 /* the helpers' entries, not this CU's stale lines */
                sh.sl.t_app_wait += wall_clock64() - t0;
                sh.sl.n_app_dealt++;
                if (late) {
                    /* helpers that do not answer (not resident: masked CUs, a busy device).  A helper that turns up
                     * later could write a row the chain has re-made since: the frame is given up -- FC_ERR_COOP, the
                     * host searches it again without helpers (core_hip.cpp complete_wave) -- and the helpers are sent home */
                    sh.sl.app_off = 1;
                    sh.failed = FC_ERR_COOP;
                    __hip_atomic_store(&c->app_off, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            __syncthreads();
            if (c->app_dbg)                     /* developer: the helpers' shares once more, here */
                for (int p = 1; p <= (int) H; p++) append_row_part_ool(F, sh, s, p, (int) H + 1);
        }
    }
#else
    append_row_part(F, sh, s, 0, 1);
#endif
    {
        GLOBAL_AS float *const gd5 = uniform_ptr(ACT_D5(F, sh));
        for (int a = tid; a < F.NA; a += B) {
            float vs[32], ip = 0;
#pragma unroll
            for (int k = 0; k < 32; k++) vs[k] = ldg((GLOBAL_AS const float *) gimgT, (unsigned) (k * P + s));
#pragma unroll
            for (int k = 0; k < 32; k++) ip += sh.pixels[a * 32 + k] * vs[k];
            stg(gd5, D5_AT(P, F.NA, a, s), ip);
        }
    }
#if FC_VARIANT_BIG
    if (F.gl0 < il)
        for (int a = tid; a < 2 * F.NA; a += B) {
            float v4[16], ip = 0;
#pragma unroll
            for (int k = 0; k < 16; k++) v4[k] = F.imgT4[(size_t) k * P + s];
#pragma unroll
            for (int k = 0; k < 16; k++) ip += sh.pixels[a * 16 + k] * v4[k];
            ACT_D4(F, sh)[(size_t) a * P + s] = ip;
        }
#endif
    if (tid == 0) {
        const int E = sh.gs_n[0] + sh.gs_n[1];       /* tree children + edges of the new state */
        /* SURVEY.md 8d: B_gram = 5 * 4 * N * (1 + E) read + 5 * 4 * N written -- the five table levels of the
         * reference (6..lc_max), one row per level, no mirrored entries.  (Until round 3 this counted what THIS
         * layout writes, 8 * 6 * (s + 1): the cached level-5 row and the mirror; 6 % more bytes per frame.) */
        sh.cnt.bytes_gram += (unsigned long long) (F.NL - 1) * 4ull * (s + 1) * (1 + E) + 4ull * (s + 1) * (F.NL - 1);
        sh.cnt.n_appends++;
    }
    gram_flush(F, sh, s + 1);
}

/* Start of the chroma bands: rle_chroma (codec/domain-pool.c:854-879) keeps the chroma_max
 * most referenced states as the domain list -- compute_hits (codec/wfalib.c:182-231): state 0
 * first, then by edge-target count descending (ties: lower state, the order glibc's stable
 * qsort leaves), only counts > 0, the kept ones ascending -- and the minimum block level
 * becomes the finest level the luminance band used (codec/coder.c:785-797). */
__device__ __noinline__ void op_chroma_pool(DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int states = sh.states, to = states - 1;
    Pool &m = sh.pool;
    const int maxd = F.chroma_max;
#if FC_VARIANT_BIG
    if (F.frame_type) { subtract_mc_dev(F, sh); __syncthreads(); }     /* codec/coder.c:798-799 */
#endif
    if (tid == 0) { sh.lc_min = F.ML; sh.ystates = states; }
    /* chroma dictionaries of more than 63 states (cfiasco --chroma-dictionary 64 ..; big builds): the list does not
     * fit sh.dl / one wave -- it lives in F.pool_states, the search is mp_steps_list_global */
    const bool longl = FC_GM || (FC_VARIANT_BIG && maxd > 63);
#if FC_GM
    /* default_chroma (codec/domain-pool.c:964-968): the constant, the uniform and the rle-no-chroma pool stay as they are */
    const bool keep_pool = sh.gm.pk[0] == FC_PK_CONSTANT || sh.gm.pk[0] == FC_PK_UNIFORM || sh.gm.pk[0] == FC_PK_RLE_NO_CHROMA;
#else
    const bool keep_pool = false;
#endif
    const int oldn = (int) m.n;
    (void) oldn;
    if (keep_pool) {
    } else
    if (longl && maxd < (int) m.n) {
        uint8_t *const mark = F.used;                     /* [P] scratch of the general scan: free between the bands */
        for (int d = tid; d < to; d += B) { __hip_atomic_store(&F.hits[d], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); mark[d] = 0; }
        __syncthreads();
        for (int s = F.basis_states + tid; s <= to; s += B)
            for (int l = 0; l < 2; l++)
                for (int e = 0, d; (d = INTO(F, s, l, e)) != NOEDGE; e++)
                    __hip_atomic_fetch_add(&F.hits[d], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        unsigned long long best = 0;
        for (int d = 1 + tid; d < to; d += B) {
            int k = (short) __hip_atomic_load(&F.hits[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned long long pk = ((unsigned long long) (unsigned) k << 32) | (0xffffffffu - (unsigned) d);
            if (k > 0 && pk > best) best = pk;
        }
        int n = maxd < to ? maxd : to, npick = 0;
        if (n > 0) { if (tid == 0) mark[0] = 1; npick = 1; }
        unsigned long long *red = sh.red;
        while (npick < n) {                              /* the same rounds as below; a pick is a mark */
            unsigned long long w = best;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                unsigned long long t = __shfl_xor(w, o);
                if (t > w) w = t;
            }
            if (lane == 0) red[wave] = w;
            __syncthreads();
            unsigned long long g = red[0];
#pragma unroll
            for (int i = 1; i < B / 64; i++) if (red[i] > g) g = red[i];
            if (g == 0) break;
            int d = (int) (0xffffffffu - (unsigned) (g & 0xffffffffu));
            npick++;
            if (best == g) {
                mark[d] = 1;
                __hip_atomic_store(&F.hits[d], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                best = 0;
                for (int dd = 1 + tid; dd < to; dd += B) {
                    int k = (short) __hip_atomic_load(&F.hits[dd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned long long pk = ((unsigned long long) (unsigned) k << 32) | (0xffffffffu - (unsigned) dd);
                    if (k > 0 && pk > best) best = pk;
                }
            }
            __syncthreads();
        }
        __syncthreads();
        /* the kept states in ascending order (wfalib.c:226): every lane compacts its share of the marks */
        int *const scr = (int *) sh.pixels;              /* B counters; the block's pixels are not needed between the bands */
        const int chunk = (to + B - 1) / B, lo = tid * chunk, hi = lo + chunk < to ? lo + chunk : to;
        int cnt = 0;
        for (int d = lo; d < hi; d++) cnt += mark[d];
        scr[tid] = cnt;
        __syncthreads();
        if (tid == 0) {
            int acc = 0;
            for (int t = 0; t < B; t++) { const int c = scr[t]; scr[t] = acc; acc += c; }
            m.n = (unsigned short) acc;
            scr[B] = 0x7fffffff;
        }
        __syncthreads();
        int o = scr[tid];
#if FC_GM
        if (GM_QAC(sh.gm.pk[0])) {
            /* qac_chroma (codec/domain-pool.c:466-498): a kept state keeps the probability index it had; through a
             * snapshot slot nobody uses between the bands (the compaction moves entries in place) */
            int16_t *q = GQ_CUR(sh, 0), *tmp = GQ_SNAP(sh, 0, 0);
            /* the reference walks the old and the new list side by side (:480-486): behind the first kept state that
             * the pool did not hold (a full pool) every index stays 0 */
            int miss = 0x7fffffff, oo = o;
            for (int d = lo; d < hi; d++)
                if (mark[d]) { const int pd = F.pos[d]; if ((pd < 0 || pd >= oldn) && oo < miss) miss = oo; oo++; }
            atomicMin(&scr[B], miss);
            __syncthreads();
            const int fm = scr[B];
            for (int d = lo; d < hi; d++) if (mark[d]) { tmp[o] = o < fm ? q[F.pos[d]] : (int16_t) 0; F.pool_states[o++] = (short) d; }
            __syncthreads();
            for (int i = tid; i < (int) m.n; i += B) q[i] = tmp[i];
        } else
#endif
        for (int d = lo; d < hi; d++) if (mark[d]) F.pool_states[o++] = (short) d;
    } else if (longl) {
        /* every pool state stays in the list (F.pool_states as it is) */
    } else
    if (maxd < (int) m.n) {
        /* histogram in HBM with device-scope atomics; read back past the L1 */
        for (int d = tid; d < to; d += B) __hip_atomic_store(&F.hits[d], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        for (int s = F.basis_states + tid; s <= to; s += B)
            for (int l = 0; l < 2; l++)
                for (int e = 0, d; (d = INTO(F, s, l, e)) != NOEDGE; e++)
                    __hip_atomic_fetch_add(&F.hits[d], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        /* lane-private best (count, lowest state) over the states d = 1 + tid, + B, ...; the
         * reference's counters are int16 (wfalib.c:187): wrap like them */
        unsigned long long best = 0;
        for (int d = 1 + tid; d < to; d += B) {
            int k = (short) __hip_atomic_load(&F.hits[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            unsigned long long pk = ((unsigned long long) (unsigned) k << 32) | (0xffffffffu - (unsigned) d);
            if (k > 0 && pk > best) best = pk;
        }
        int n = maxd < to ? maxd : to, npick = 0;
        if (n > 0) { if (tid == 0) sh.dl[0] = 0; npick = 1; }
        unsigned long long *red = sh.red;
        while (npick < n) {
            unsigned long long w = best;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                unsigned long long t = __shfl_xor(w, o);
                if (t > w) w = t;
            }
            if (lane == 0) red[wave] = w;
            __syncthreads();
            unsigned long long g = red[0];
#pragma unroll
            for (int i = 1; i < B / 64; i++) if (red[i] > g) g = red[i];
            if (g == 0) break;                           /* no state with a count > 0 left */
            int d = (int) (0xffffffffu - (unsigned) (g & 0xffffffffu));
            if (tid == 0) sh.dl[npick] = (short) d;
            npick++;
            if (best == g) {                             /* owner: retire it, rescan its share */
                __hip_atomic_store(&F.hits[d], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                best = 0;
                for (int dd = 1 + tid; dd < to; dd += B) {
                    int k = (short) __hip_atomic_load(&F.hits[dd], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    unsigned long long pk = ((unsigned long long) (unsigned) k << 32) | (0xffffffffu - (unsigned) dd);
                    if (k > 0 && pk > best) best = pk;
                }
            }
            __syncthreads();
        }
        __syncthreads();
        if (tid == 0) {
            for (int i = 1; i < npick; i++) {            /* ascending, wfalib.c:226 */
                short v = sh.dl[i];
                int j = i;
                while (j > 0 && sh.dl[j - 1] > v) { sh.dl[j] = sh.dl[j - 1]; j--; }
                sh.dl[j] = v;
            }
            for (int i = 0; i < npick; i++) F.pool_states[i] = sh.dl[i];
            m.n = (unsigned short) npick;
        }
    } else if (tid < (int) m.n) {
        sh.dl[tid] = F.pool_states[tid];                 /* n <= chroma_max <= 63 */
    }
    __syncthreads();
    if (tid == 0 && !keep_pool) { m.y_index = 0; m.max_domains = m.n; }
    for (int s = tid; s < states; s += B) F.pos[s] = -1;
    /* finest level with a linear combination in the luminance band */
    int mn = F.ML;
    for (int s = F.basis_states + tid; s < states; s += B) {
        int lin = (TREE(F, s, 0) == RANGE_) + (TREE(F, s, 1) == RANGE_);
        unsigned lv = (unsigned) ((int) F.level_of_state[s] - 1);
        if (lin && lv < (unsigned) mn) mn = (int) lv;
    }
    atomicMin(&sh.lc_min, mn);
    __syncthreads();
    if (longl) { for (int i = tid; i < (int) m.n; i += B) F.pos[F.pool_states[i]] = (short) i; }
    else if (tid < (int) m.n) F.pos[sh.dl[tid]] = (short) tid;
#if !FC_SPEC
    if (!F.bx && F.chroma_sparse) chroma_need_static(F, sh);
#endif
}
