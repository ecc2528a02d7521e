/*
 *  fc_spec.inc -- block-level speculation, FC_SPEC builds only (frame_coder.h, FcSpecCtl): the
 *  tables a chain takes for a block (spec_tables), the table workers (spec_worker) and the append
 *  helpers (spec_append_helper).
 *
 *  Reference: no code of its own; the workers build the chain's tables, bit for bit: inner-product
 *  tables codec/ip.c:46-323, state tables codec/control.c:48-131,205-258.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

#if FC_SPEC
/* Chain, all lanes: whose tables does block `blk` get?  The buffer a table worker has filled for it
 * (sh.tab_from = the states whose entries are good: what the worker saw, less what a return of the
 * chain has replaced since), or -- no worker got there in time -- the chain's own tables, from scratch. */
__device__ void spec_tables(DevFrame &__restrict__ F, Sh &__restrict__ sh, int blk)
{
    if (threadIdx.x == 0) {
        Sh::SpecLocal &sl = sh.sl;
        FcSpecCtl *c = sl.ctl;
        const unsigned b = (unsigned) blk % FC_SPEC_R;
        int from = -1;
        {   /* for the table workers: where the chain is, and which buffers it needs no more (those of the
             * blocks below the oldest one that still waits for its verdict; in the chroma bands none does) */
            unsigned oldest = (unsigned) blk;
            if (!sh.band && sl.commit != sl.head) oldest = sl.blkof[sl.commit % FC_SPEC_W];
            __hip_atomic_store(&c->tab_free, oldest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&c->blk_cur, (unsigned) blk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if ((unsigned) blk < c->n_tabs) {
            const unsigned long long t0 = wall_clock64();
            for (;;) {
                if (__hip_atomic_load(&c->tab_seq[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned) blk + 1) {   /* (fence below) */
                    unsigned S = __hip_atomic_load(&c->tab_s[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned te = __hip_atomic_load(&c->tab_epoch[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (sl.epoch - te > 32u) S = 0;
                    else for (unsigned e = te; e != sl.epoch; e++) if (sl.rb_s[e % 32u] < S) S = sl.rb_s[e % 32u];
                    from = (int) S < table_states(sh) ? (int) S : table_states(sh);
                    break;
                }
                if (wall_clock64() - t0 > c->tab_wait) break;
                __builtin_amdgcn_s_sleep(8);
            }
        }
        if (from >= 0) {
            sh.par.ipis = (float *) (sl.tabs + (size_t) b * c->tab_stride);
            sh.par.d5 = sh.par.ipis + (size_t) F.NS * F.P;
            sh.tab_shared = 1; sl.n_tab_used++;
        } else {
            sh.par.ipis = F.ipis; sh.par.d5 = F.d5;
            sh.tab_shared = 0; sl.n_tab_missed++; from = 0;
        }
        sh.tab_from = from;
        take_acquire();                 /* the worker's entries, not this CU's stale lines (one lane; the barrier follows) */
    }
    __syncthreads();
}
#endif

#if FC_SPEC
/* Table worker (all lanes; returns when the chain is done).  Luminance band: workgroup `role` of the T
 * workers builds the tables of every T-th block of the host's list, ahead of the chain, for the states
 * the chain has published, into the buffer blk % FC_SPEC_R.  Chroma bands of a colour frame (block
 * indices from n_blocks on; dynamic: a verifier that has turned worker): blocks handed out one by one. */
__device__ __noinline__ void spec_worker(DevFrame &__restrict__ F, Sh &__restrict__ sh, unsigned role, unsigned T, bool dynamic)
{
    __shared__ int tw_x, tw_y, tw_go;
    __shared__ unsigned tw_e0;
    const int tid = threadIdx.x;
    FcSpecCtl *const c = F.spec;
    unsigned j = role - 1;                      /* lane 0's */
    const unsigned short *blocks = (const unsigned short *) ((const char *) c + c->off_blocks);
    if (tid == 0) { sh.band = 0; sh.gap_lo = sh.gap_hi = 0; sh.deadmask = 0; sh.sl.role = (int) role; sh.ystates = 0; }
    for (;;) {
        __syncthreads();
        if (tid == 0) {
            int go = 1;
            const unsigned nb = c->n_blocks;
            bool have = false;                  /* dynamic: j is a block taken from tab_next */
            for (;;) {
                if (__hip_atomic_load(&c->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { go = 0; break; }
                if (!dynamic) {
                    const unsigned cur = __hip_atomic_load(&c->blk_cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    while (j + 1 < cur) j += T;           /* the chain is past these (it may still wait for block cur - 1) */
                    if (j >= nb) dynamic = true;
                }
                if (dynamic) {
                    if (!__hip_atomic_load(&c->chroma_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) || c->n_tabs <= nb) {
                        __builtin_amdgcn_s_sleep(64);
                        continue;
                    }
                    if (!have) { j = nb + atomicAdd(&c->tab_next, 1u); have = true; }
                    if (j >= c->n_tabs) { __builtin_amdgcn_s_sleep(64); continue; }       /* nothing left: wait for the end */
                }
                if (j < __hip_atomic_load(&c->tab_free, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + FC_SPEC_R
                    && __hip_atomic_load(&c->s_pub, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
                __builtin_amdgcn_s_sleep(32);
            }
            tw_go = go;
            if (go) {
                const unsigned b = j % FC_SPEC_R;
                __hip_atomic_store(&c->tab_seq[b], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                /* the epoch first: a return of the chain lowers s_pub before it raises the epoch */
                tw_e0 = __hip_atomic_load(&c->epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                unsigned S = __hip_atomic_load(&c->s_pub, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                const unsigned band = j / nb;
                if (band) S = c->ystates;                 /* the finished luminance dictionary */
                sh.band = (int) band; sh.states = (int) S; sh.ystates = (int) S;
                sh.par.ipis = (float *) ((char *) c + c->off_tabs + (size_t) b * c->tab_stride);
                sh.par.d5 = sh.par.ipis + (size_t) F.NS * F.P;
                tw_x = blocks[2 * (j % nb)]; tw_y = blocks[2 * (j % nb) + 1];
            }
        }
        __syncthreads();
        if (!tw_go) break;              /* (lane 0's acquire loads of epoch / s_pub have dropped this CU's L1) */
        op_init_range(F, sh, tw_x, tw_y, 0);
        WAVE_DRAIN();
        __syncthreads();
        if (tid == 0) {
            const unsigned b = j % FC_SPEC_R;
            publish_release();
            __hip_atomic_store(&c->tab_s[b], (unsigned) sh.states, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&c->tab_epoch[b], tw_e0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            WAVE_DRAIN();                       /* tab_s / tab_epoch before tab_seq */
            __hip_atomic_store(&c->tab_seq[b], j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (dynamic) j = c->n_tabs + 1;     /* take the next one */
            else j += T;
        }
    }
}
#endif

#if FC_SPEC
/* Append helper h of the H helpers of a frame (all lanes; returns when the chain is done): the entries t with
 * (t / B) mod (H + 1) == h + 1 of every Gram row the chain publishes (FcSpecCtl.app_*, frame_coder.h).  F is the CHAIN's
 * descriptor, read only; of sh only what append_row_part looks at is set up. */
__device__ __noinline__ void spec_append_helper(DevFrame &__restrict__ F, Sh &__restrict__ sh, unsigned h, unsigned H)
{
    __shared__ int ah_go, ah_s;
    const int tid = threadIdx.x;
    FcSpecCtl *const c = F.spec;
    unsigned seen = 0;
    if (!c) return;                                  /* the launch speculates without its buffers: nothing to help with */
    if (tid == 0) { sh.gap_lo = sh.gap_hi = 0; sh.gap_shift = 0; sh.deadmask = 0; sh.band = 0; }
    for (;;) {
        __syncthreads();
        if (tid == 0) {
            int go = 0;
            for (;;) {                               /* relaxed polls, ONE acquire once there is something to take */
                if (__hip_atomic_load(&c->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                    || __hip_atomic_load(&c->app_off, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                const unsigned q = __hip_atomic_load(&c->app_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (q != seen) { seen = q; go = 1; break; }
                __builtin_amdgcn_s_sleep(1);
            }
            if (go) {
                take_acquire();                      /* the chain's rows, images, automaton and the descriptor: nothing stale */
                ah_s = c->app_s; sh.flim = c->app_flim;
                for (int l = 0; l < 2; l++) {
                    sh.gs_n[l] = c->app_n[l]; sh.gs_c[l] = c->app_c[l];
                    for (int e = 0; e <= MAXED; e++) { sh.gs_idx[l][e] = c->app_idx[l][e]; sh.gs_w[l][e] = c->app_w[l][e]; }
                }
            }
            ah_go = go;
        }
        __syncthreads();
        if (!ah_go) break;                           /* uniform */
        if (c->app_dbg != 1) append_row_part_ool(F, sh, ah_s, (int) h + 1, (int) H + 1);
        WAVE_DRAIN();
        __syncthreads();
        if (tid == 0) publish_release();
        if (tid == 0) __hip_atomic_fetch_add(&c->app_done, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
#endif
