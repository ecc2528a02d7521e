/*
 *  frame_coder.hip -- the FIASCO encode-side hot path as ONE persistent gfx950 kernel:
 *  one workgroup owns one frame and runs its complete partition search; helper workgroups may
 *  serve the same frame (table passes: FcCoop, fc_tables.inc; speculation: fc_spec.inc).
 *
 *  One translation unit, built nine ways (csrc/Makefile).  The parts, in include order, and below
 *  each part that computes, the reference file:line it is bit-compatible with:
 *    fc_config.inc     build geometry, per-build symbols, constants, OP_* and PH_* enums
 *    fc_lds.inc        LDS layout: the range stack, model pools and snapshots, Sh
 *    fc_access.inc     small helpers, hand-offs between workgroups, Gram and image table access
 *                                  lib/rpf.c:59-169, lib/misc.c:223-244
 *    fc_tables.inc     inner-product tables, FcCoop, chroma-need closure, op_init_range (and ipt_layout.h,
 *                      which it includes: the state-major copy of the recursion's sources, FC_IPT)
 *                                  codec/ip.c:46-323, codec/subdivide.c:504-541,612-644
 *    fc_append.inc     state append, chroma domain pool
 *                                  codec/control.c:48-131,205-258, codec/domain-pool.c:621-852
 *    fc_predict.inc    prediction and motion search (big build)
 *                                  codec/prediction.c, codec/mwfa.c
 *    fc_models.inc     snapshot slots, generic models (FC_GM)
 *                                  codec/domain-pool.c:621-852, codec/coeff.c:215-267
 *    mp_device.inc     matching pursuit: rate terms, table pass, the scans with scratch in HBM, op_approx as a
 *                      sequence of steps (and what it includes: mp_roles.h, the roles of the table pass; mp_step.inc,
 *                      the pieces of a step every scan shares; mp_reg.inc, the register scan and the short list scan)
 *                                  codec/approx.c:74-271,317-699 (domain-parallel, see below)
 *    fc_serial.inc     partition search: serial state machine, lane 0, explicit LDS stack; bands
 *                                  codec/subdivide.c:60-502, codec/coder.c:738-833, codec/bintree.c:35-73
 *    fc_spec.inc       speculation: table workers, append helpers (FC_SPEC)
 *    frame_coder.hip   basis_init, the kernel (frame queue, operation loop), the launch stubs
 *                                  codec/control.c:133-173
 *
 *  Parallel decomposition of one matching-pursuit call (D candidate domains):
 *    phase A (all waves)  per candidate d, fused: Gram-Schmidt update of rem_num/rem_den
 *                         against the vector chosen in the previous step + stage-1 cost
 *                         estimate e_d; wave-wide min of e_d per 64-candidate block.
 *    phase B (rounds)     exact replay of the reference's index-ordered scan with its
 *                         running `min_costs`: blocks whose min e_d cannot beat the
 *                         running minimum are skipped; the wave that owns the next block
 *                         evaluates its survivors' true costs lane-parallel and accepts in
 *                         index order by ballot/ffs (strict '<', codec/approx.c:459-462,592).
 *  Per-candidate scratch lives in registers (mp_reg.inc); mp_device.inc holds the rate
 *  terms, the general (HBM scratch) and the chroma (explicit list) variants of the scan.
 *  All float arithmetic keeps the reference's operation order; every part MUST be built
 *  with -ffp-contract=off (no FMA).  double log2() is evaluated once per call into small
 *  LDS tables (the rate models only ever need log2 of count/total ratios).
 *
 *  Device scope: gray and colour frames, I, P and B (bands: codec/coder.c:738-833).  The default
 *  build covers the CLI defaults (block levels 6..10, <= 3 vectors, `rle' pool, `adaptive'
 *  coefficients); FC_VARIANT_BIG the other option sets, FC_HM and FC_GM the rest of the model
 *  registries (fc_config.inc, csrc/Makefile).
 *
 *  Register budget: the default build is compiled for 4 workgroups per CU, i.e. <= 128 VGPRs.
 *  The persistent loop makes EVERYTHING loop invariant in the compiler's eyes; what must not be
 *  computed once at kernel entry and kept for the kernel's lifetime is hidden from the hoisting
 *  (opaque thread index in the scan, out-of-line log2 tables, descriptor fields through
 *  sh.par in LDS).  tests/isa_spills.sh shows what still goes to scratch and from which line.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "frame_coder.h"

#include "fc_config.inc"
#include "fc_lds.inc"
#include "fc_access.inc"
#include "fc_tables.inc"
#include "fc_append.inc"
#include "fc_predict.inc"
#include "fc_models.inc"
#include "mp_device.inc"
#include "fc_serial.inc"
#include "fc_spec.inc"

/* basis states: images, Gram tables (codec/control.c:133-173); lane 0, a few hundred flops */
__device__ void basis_init(DevFrame &F, Sh &sh)
{
    const int nb = F.basis_states, il = F.images_level;
    for (int s = 0; s < nb; s++) {
        F.img[(size_t) s * F.NI] = F.final_d[s];
        if (il == 0) F.imgT[s] = F.final_d[s];
    }
    for (int l = 1; l <= il; l++)
        for (int s = 0; s < nb; s++)
            for (int i = 0; i < (1 << l); i++) {
                float v = image_elem(F, s, l, i);
                F.img[(size_t) s * F.NI + (1 << l) - 1 + i] = v;
                if (l == il) F.imgT[(size_t) i * F.P + s] = v;
#if FC_VARIANT_BIG
                if (l == il - 1 && F.gl0 < il) F.imgT4[(size_t) i * F.P + s] = v;
#endif
            }
    for (int q = 0; q < F.NL; q++)
        for (int s1 = 0; s1 < nb; s1++)
            for (int s2 = 0; s2 <= s1; s2++) {
                if (!F.domain_type[s2]) continue;
#if FC_VARIANT_BIG
                if (F.gl0 < il) {
                    gram_store(F, q, s1, s2, q == 0 ? gram_dot4(F, s1, s2) : q == 1 ? gram_dot(F, s1, s2)
                                                                   : gram_entry(F, q, s1, s2));
                    continue;
                }
#endif
                gram_store(F, q, s1, s2, q == 0 ? gram_dot(F, s1, s2) : gram_entry(F, q, s1, s2));
            }
    sh.states = nb;
}

#if FC_VARIANT_BIG
/* the same for a basis in DevFrame.bx (hundreds of states with edge lists of up to 33 entries): all lanes; a level
 * of the images / of the Gram tables needs the level below complete for ALL basis states (codec/control.c:205-258,
 * codec/ip.c:213-257) */
__device__ void basis_init_bx(DevFrame &F, Sh &sh)
{
    const int tid = threadIdx.x, il = F.images_level;
    const BxView V = bx_view(F);
    const int nb = V.nb;
    for (int s = tid; s < nb; s += B) {
        F.img[(size_t) s * F.NI] = F.final_d[s];
        if (il == 0) F.imgT[s] = F.final_d[s];
    }
    __syncthreads();
    for (int l = 1; l <= il; l++) {
        for (int k = tid; k < (nb << l); k += B) {
            const int s = k >> l, i = k & ((1 << l) - 1);
            const float v = image_elem_bx(F, V, s, l, i);
            F.img[(size_t) s * F.NI + (1 << l) - 1 + i] = v;
            if (l == il) F.imgT[(size_t) i * F.P + s] = v;
            if (l == il - 1 && F.gl0 < il) F.imgT4[(size_t) i * F.P + s] = v;
        }
        __syncthreads();
    }
    for (int q = 0; q < F.NL; q++) {
        for (int k = tid; k < nb * nb; k += B) {
            const int s1 = k / nb, s2 = k - s1 * nb;
            if (s2 > s1 || !F.domain_type[s2]) continue;
            float v;
            if (F.gl0 < il) v = q == 0 ? gram_dot4(F, s1, s2) : q == 1 ? gram_dot(F, s1, s2) : gram_entry_bx(F, V, q, s1, s2);
            else v = q == 0 ? gram_dot(F, s1, s2) : gram_entry_bx(F, V, q, s1, s2);
            gram_store(F, q, s1, s2, v);
        }
        __syncthreads();
    }
}
#endif

/*
 *  One workgroup per frame.  A launch may hold more frames than slabs (more than the chip runs at
 *  once, or than HBM holds): the first `nlend` frames own a slab each, the others borrow one --
 *  the hardware's workgroup dispatcher is the queue.  A workgroup that finishes hands its slab to
 *  a ring of free slabs (ring[ctr[1]++] = base); a borrower takes the next ticket (ctr[0]++) and
 *  waits for that entry.  With as many slabs as resident workgroups the entry is always there
 *  already: the borrower only became resident because another workgroup had left.  The borrower
 *  re-bases every slab pointer of its own descriptor (ptrmask: one bit per 8-byte word) onto the
 *  slab it got.  No tail of idle CUs waiting for the slowest of the first frames, no limit on the
 *  size of a launch from the 200 MB slabs.
 */
#if FC_SPEC
#define SPEC_STRIDE ((unsigned) ((sizeof(Sh) + 255) / 256 * 256))          /* bytes per checkpoint slot */
#define SPEC_SLOTS(ctl) ((char *) (ctl) + (sizeof(FcSpecCtl) + 255) / 256 * 256)
#endif

__global__ void __launch_bounds__(B, FC_WG_PER_CU)
#if FC_SPEC
/* G workgroups per frame: workgroup f * G is the chain of frame f (descriptor frames[f]), the G - 1
 * after it are its verifiers (descriptors vframes[f * (G - 1) ..]: the chain's with private
 * <sub-block, state> tables, scratch and state-id range).  G == 1: no speculation. */
FC_KERNEL(DevFrame *frames, DevFrame *vframes, unsigned G, unsigned n, unsigned H)
#else
FC_KERNEL(DevFrame *frames, unsigned nlend, unsigned long long *ring, unsigned *ctr, const unsigned *ptrmask,
          unsigned long long queue_wait_ticks, unsigned coopW)
#endif
{
    /* the LDS budget of the build: FC_WG_PER_CU workgroups share the 160 KB of a CU.  Beside Sh the kernel keeps a few
     * words (and, speculating builds, one SpecLocal): the big 256-thread build is at 81 736 of its 81 920 bytes */
#if FC_SPEC
    constexpr unsigned FC_LDS_EXTRA = sizeof(Sh::SpecLocal) + 64;
#else
    constexpr unsigned FC_LDS_EXTRA = 64;
#endif
    static_assert(sizeof(Sh) + FC_LDS_EXTRA <= (160u * 1024u) / FC_WG_PER_CU, "Sh outgrows the LDS share of a workgroup of this build");
    __shared__ Sh sh;
#if FC_SPEC
    __shared__ Sh::SpecLocal sl_keep;
    __shared__ unsigned task_seq, spec_slot, spec_used, spec_vid;
    __shared__ int task_go, spec_act, spec_bad;
    if (threadIdx.x == 0) spec_bad = 0;
    if (blockIdx.x >= n * G) {
        /* behind the n * G workgroups of the frames: H append helpers per frame, on the chain's descriptor (read only) */
        const unsigned k = blockIdx.x - n * G;
        spec_append_helper(frames[k / H], sh, k % H, H);
        return;
    }
    const unsigned role = blockIdx.x % G;
    DevFrame &F = role ? vframes[(blockIdx.x / G) * (G - 1) + role - 1] : frames[blockIdx.x / G];
    unsigned long long *const ring = nullptr;
#elif FC_VARIANT_BIG
    /* coopW > 1: that many workgroups per frame (FcCoop; nlend = frames, no queue).  The workgroups of a frame get
     * block ids that differ by multiples of 8: the same XCD where the dispatcher deals blocks round robin -- a
     * matter of speed only, the hand-offs are agent-scope release / acquire */
    const unsigned cW = coopW > 1 ? coopW : 1;
    unsigned fidx = blockIdx.x, member = 0;
    if (cW > 1) {
        fidx = (blockIdx.x / (8 * cW)) * 8 + blockIdx.x % 8;
        member = (blockIdx.x / 8) % cW;
        if (fidx >= nlend) return;
    }
    DevFrame &F = frames[fidx];
    if (member) { coop_helper(F, sh, member, cW); return; }
    if (threadIdx.x == 0) {
        sh.coopW = F.coop ? cW : 1; sh.coop_seq = 0;
        sh.coopD = cW > 1 && F.coop ? (int) F.coop->depth : 0; sh.coop_minsub = cW > 1 && F.coop ? F.coop->minsub : 0;
        sh.coop_ticks = cW > 1 && F.coop ? F.coop->done_ticks : 0;
    }
#else
    DevFrame &F = frames[blockIdx.x];
#endif
    const int tid = threadIdx.x;

#if !FC_SPEC
    if (ring && blockIdx.x >= nlend) {
        /* a frame without a slab: wait for the next free one and move the descriptor onto it */
        __shared__ unsigned long long got;
        if (tid == 0) {
            const unsigned t = atomicAdd(&ctr[0], 1u);
            unsigned long long b;
            /* Forward progress rests on an observation, not a promise of HIP: workgroups become
             * resident in blockIdx order, so every slab owner is resident (or done) before a
             * borrower spins here.  Should that ever not hold the wait is bounded (wall clock,
             * 100 MHz): the frame gives up with FC_ERR_QUEUE and the host encodes it again in a slab
             * of its own (complete_wave) -- a diagnostic and a retry instead of a hung GPU. */
            const unsigned long long t_give_up = wall_clock64() + queue_wait_ticks;
            while ((b = __hip_atomic_load(&ring[t], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
                if (wall_clock64() > t_give_up) break;
                __builtin_amdgcn_s_sleep(32);
            }
            got = b;                                        /* (the acquire has dropped the CU's L1: nothing stale of the slab's earlier users) */
        }
        __syncthreads();
        if (got == 0) {                                     /* uniform: no slab arrived */
            if (tid == 0) { F.status = FC_ERR_QUEUE; F.states = 0; }
            return;
        }
        {
            unsigned long long *d = (unsigned long long *) &F;
            const unsigned long long lo = (unsigned long long) F.slab_base, span = F.slab_bytes;
            const unsigned long long delta = got - lo;
            unsigned long long v[(FC_DESC_WORDS + B - 1) / B];
#pragma unroll
            for (unsigned k = 0; k < (FC_DESC_WORDS + B - 1) / B; k++) {      /* read everything first: slab_base moves too */
                const unsigned w = k * B + tid;
                v[k] = w < FC_DESC_WORDS ? d[w] : 0;
            }
            __syncthreads();
#pragma unroll
            for (unsigned k = 0; k < (FC_DESC_WORDS + B - 1) / B; k++) {
                const unsigned w = k * B + tid;
                if (w < FC_DESC_WORDS && ((ptrmask[w >> 5] >> (w & 31)) & 1u) && v[k] - lo < span) d[w] = v[k] + delta;
            }
        }
        __threadfence();
        __syncthreads();
        __builtin_amdgcn_s_dcache_inv();                    /* the descriptor is read through the scalar cache */
    }
#endif

#if FC_SPEC
    if (tid == 0) {
        Sh::SpecLocal &sl = sh.sl;
        sh.gap_lo = sh.gap_hi = 0; sh.gap_shift = 0; sh.deadmask = 0;
        sh.cap = F.spec ? F.spec_cap : F.P;
        sl.ctl = F.spec; sl.slots = F.spec ? SPEC_SLOTS(F.spec) : nullptr;
        sl.role = (int) role; sl.on = F.spec != nullptr && G > 1;
        sl.mode = role == 0 && sl.on ? 1 : 0;
        sl.T = F.spec_T; sl.tabs = F.spec ? (char *) F.spec + F.spec->off_tabs : nullptr;
        sl.chroma_tabs = 0;
        sl.n_tab_used = sl.n_tab_missed = sl.n_adopted = 0;
        sl.app_H = role == 0 && F.spec && G > 1 ? F.spec->app_H : 0u; sl.app_min = F.spec ? F.spec->app_min : 0u;
        sl.app_seq = 0; sl.app_off = 0; sl.n_app_dealt = sl.t_app_wait = 0;
        for (int k = 0; k < 32; k++) sl.rb_s[k] = 0;
        sh.blk = 0; sh.tab_shared = 0; sh.tab_from = 0;
        sl.floor = 0; sl.head = sl.commit = 0; sl.spec_mask = 0; sl.nospec = 0; sl.epoch = 0;
        sl.verdict = 0; sl.abort = 0; sl.ops = 0; sl.mlc = 0.0f; sl.nlc = 0; sl.learn = 0.0f;
        sl.n_tasks = sl.n_confirmed = sl.n_wrong = sl.n_timeout = sl.n_inline = sl.t_wait = 0;
        sl_keep = sl;
    }
    if (role == 0) {
#endif
    if (tid < 10 && tid >= 1)
        sh.m0tab[tid] = (float) -log2((double) (1 - 1 / (float) (1 << tid)));
    if (tid == 0) {
        const int ML = F.ML;
        static const unsigned c0[22] = {20,17,15,10,5,4,3,2,1,1,1,1,1,1,1,1,1,1,1,1,1,1};
        static const unsigned c1[22] = {1,1,1,1,1,1,1,1,1,2,3,5,10,15,20,25,30,35,60,60,60,60};
        sh.failed = 0;
        /* a staged frame may be encoded several times: start from clean counters */
        /* the roofline / profile counters are accumulated in LDS (a global read-modify-write
         * per call is a memory round trip of the serial lane) and stored once at the end */
        sh.cnt.bytes_mp = sh.cnt.bytes_img = sh.cnt.bytes_gram = 0;
        sh.cnt.n_mp = sh.cnt.n_steps = sh.cnt.n_blocks = sh.cnt.n_appends = sh.cnt.n_fulleval = 0;
        sh.cnt.t_mpA = sh.cnt.t_mpB = sh.cnt.n_blockevals = 0;
        F.trace_n = 0;
        for (int k = 0; k < 8; k++) F.dbg[k] = 0;
#ifdef FC_LATENCY_PROBE
        {   /* developer probe: dependent-load latency on a small global array (L2 resident)
             * and on a freshly stored one */
            volatile float *a = F.est;
            for (int k = 0; k < 64; k++) a[k] = (float) ((k * 7 + 3) & 63);
            __builtin_amdgcn_s_waitcnt(0);
            unsigned long long c0 = __builtin_readcyclecounter();
            int idx = 0;
            for (int k = 0; k < 64; k++) idx = (int) a[idx];
            unsigned long long c1 = __builtin_readcyclecounter();
            F.dbg[5] = (c1 - c0) / 64 + (idx & 0);
            /* store -> load of the same word */
            c0 = __builtin_readcyclecounter();
            for (int k = 0; k < 64; k++) { a[64] = (float) k; idx += (int) a[64]; }
            c1 = __builtin_readcyclecounter();
            F.dbg[6] = (c1 - c0) / 64 + (idx & 0);
        }
#endif
        /* rows of the basis states (input/basis.c:61-114, input/read.c:219-340) */
#if FC_VARIANT_BIG
        if (F.bx) {                          /* their edges stay in DevFrame.bx (bx_view) */
            const BxView V = bx_view(F);
            for (int s = 0; s < V.nb; s++) {
                F.final_d[s] = V.final_d[s];
                F.domain_type[s] = (uint8_t) V.dtype[s];
                F.level_of_state[s] = 0xff;
                for (int l = 0; l < 2; l++) { TREE(F, s, l) = RANGE_; INTO(F, s, l, 0) = NOEDGE; }
            }
        } else
#endif
        for (int s = 0; s < F.basis_states; s++) {
            F.final_d[s] = F.b_final[s];
            F.domain_type[s] = F.b_dtype[s];
            F.level_of_state[s] = 0xff;
            for (int l = 0; l < 2; l++) {
                TREE(F, s, l) = F.b_tree[s][l];
                for (int e = 0; e < 6; e++) {
                    INTO(F, s, l, e) = F.b_into[s][l][e];
                    WEIGHT(F, s, l, e) = F.b_weight[s][l][e];
                    if (F.b_into[s][l][e] == NOEDGE) break;
                }
            }
        }
        for (int w = 0; w < 2; w++)
            for (int l = 0; l < ML; l++) {
                int k = l < 22 ? l : 21;
                sh.tm[w * 2 * ML + l] = c1[k];
                sh.tm[w * 2 * ML + ML + l] = c0[k] + c1[k];
            }
        for (int i = 4 * ML; i < TM_WORDS; i++) sh.tm[i] = 0;
        /* rle pool over the usable basis states (domain-pool.c:632-676) */
        Pool &m = sh.pool;
        m.total = 0;
        for (int i = 0; i <= MAXED; i++) { m.count[i] = 1; m.total++; }
        m.n = 0; m.max_domains = (unsigned short) F.pool_max; m.y_index = 0;
        m.d0_index = 0; m.d0_yindex = 0; m.d0_n = 0;
#if FC_GM
        /* alloc_domain_pool and the allocators behind it (codec/domain-pool.c:203-236) for the kinds of both sets */
        sh.gm.pk[0] = F.gm_pool[0]; sh.gm.pk[1] = F.pred_on ? F.gm_pool[1] : FC_PK_CONSTANT;
        sh.gm.ck[0] = F.gm_coeff[0]; sh.gm.ck[1] = F.gm_coeff[1];
        sh.gm.qa = 0; sh.gm.gq = F.gq; sh.gm.P = F.P;
        sh.gm.base = sh.gm.kept = 0.0f; sh.gm.lg1 = 0.0;
        sh.dpool = m;
        for (int set = 0; set < 2; set++) {
            Pool &pm = set ? sh.dpool : sh.pool;
            const int k = sh.gm.pk[set];
            int maxd = F.pool_max ? F.pool_max : 1;                 /* "Using at least DC component.", :221-226 */
            if (k == FC_PK_BASIS) maxd = F.basis_states;
            if (k == FC_PK_UNIFORM || k == FC_PK_CONSTANT) maxd = 0xffff;
            pm.max_domains = (unsigned short) maxd;
            if (!GM_RLE(k)) { pm.total = 0; for (int i = 0; i <= MAXED; i++) pm.count[i] = 0; }
        }
        for (int s = 0; s < F.basis_states; s++) {
            F.pos[s] = -1;
            if (F.domain_type[s] & 2) gm_offer(F, sh, s);
        }
        if ((F.domain_type[0] & 2) && F.pos[0] < 0) { F.pos[0] = 0; F.pool_states[0] = 0; }   /* no pool keeps a list */
        if (sh.gm.pk[0] == FC_PK_CONSTANT) sh.pool.n = 1;          /* the list {0} */
        if (sh.gm.pk[1] == FC_PK_CONSTANT) sh.dpool.n = 0;
#else
        for (int s = 0; s < F.basis_states; s++) {
            F.pos[s] = -1;
            if ((F.domain_type[s] & 2) && m.n < m.max_domains) {
                F.pos[s] = (short) m.n;
                F.pool_states[m.n++] = (short) s;
                if (s == 0) m.d0_n = 1;
            }
        }
#endif
        /* aac model, all-ones (coeff.c:297-310) */
        sh.n16 = (32 + 2 * F.coeff_size + 15) / 16;
#if FC_VARIANT_BIG
        if (F.pred_on && (32 + 2 * F.d_coeff_size + 15) / 16 > sh.n16) sh.n16 = (32 + 2 * F.d_coeff_size + 15) / 16;
        sh.nslot = F.pred_on ? 5 : 2;
        /* snapshots that outgrow LDS (wide level window x many mantissa symbols) live in HBM; with
         * prediction (5 slots per depth, deeper stack) always: aac snapshots in the first part of
         * the area, tree-model snapshots behind them */
        sh.snap = (F.pred_on || (F.level - F.lc_min + 3) * 2 * sh.n16 > SNAP_POOL16) && F.snap_hbm
                  ? (uint4 *) F.snap_hbm : sh.snap_pool;
        sh.snap_tm_p = F.pred_on && F.snap_hbm ? (uint4 *) F.snap_hbm + FC_DEPTH * 5 * FC_N16MAX : (uint4 *) sh.snap_tm;
        sh.pred_active = 0; sh.pred_lo = sh.pred_rec = 0;
#endif
        {
            const int depth_need = F.level - F.lc_min + 2
#if FC_VARIANT_BIG
                                   + (F.pred_on ? F.p_max - F.lc_min + 2 : 0)
#endif
                                   ;
#if FC_VARIANT_BIG
            const bool snap_lds = sh.snap == &sh.snap_pool[0];
            const bool tm_lds = (const void *) sh.snap_tm_p == (const void *) &sh.snap_tm[0];
#else
            const bool snap_lds = true, tm_lds = true;
#endif
#if FC_VARIANT_BIG
            const int snap_need = (F.level - F.lc_min + 3) * 2 * sh.n16;
#else
            const int snap_need = (F.level - F.lc_min + 3 + F.lc_max - F.lc_min) * sh.n16;
            sh.par.snap_b1 = (F.level - F.lc_min + 3) - (F.level - F.lc_max);
#endif
            if ((snap_lds && snap_need > SNAP_POOL16)
                || (tm_lds && (F.level - F.lc_min + 3) * 4 * TM_N16(ML) > SNAP_TM_WORDS) || F.coeff_nt > 16
                || (F.P + 63) / 64 > NBLOCKMIN            /* block minima of the general scan */
                || depth_need > FC_DEPTH
                || F.max_elements > FC_MAXE               /* term slots of the table ops */
                || (!FC_VARIANT_BIG && F.pred_on))        /* prediction needs the big build */
                sh.failed = FC_ERR_INTERNAL;
        }
        for (int i = 0; i < (FC_VARIANT_BIG ? FC_MAXCOEFF_BIG : FC_MAXCOEFF); i++) sh.cb.cnt[i] = 0;
        for (int i = 0; i < 16; i++) sh.cb.tot[i] = 0;
        for (int i = 0; i < F.coeff_size; i++) sh.cb.cnt[i] = 1;
        sh.cb.tot[0] = (short) F.dcs;
        for (int i = 1; i < F.coeff_nt; i++) sh.cb.tot[i] = (short) F.sy;
#if FC_VARIANT_BIG
        /* d_coeff (codec/coder.c:732-736) and the second rle pool over the same basis states */
        for (int i = 0; i < FC_MAXCOEFF_BIG; i++) sh.dcb.cnt[i] = 0;
        for (int i = 0; i < 16; i++) sh.dcb.tot[i] = 0;
        for (int i = 0; i < F.d_coeff_size; i++) sh.dcb.cnt[i] = 1;
        sh.dcb.tot[0] = (short) F.d_dcs;
        for (int i = 1; i < F.coeff_nt; i++) sh.dcb.tot[i] = (short) F.d_sy;
#if !FC_GM
        sh.dpool = sh.pool;
#endif
        sh.dq.rpf_mant = F.d_rpf_mant; sh.dq.dc_mant = F.d_dc_mant; sh.dq.sy = F.d_sy; sh.dq.dcs = F.d_dcs;
        sh.dq.rpf_range = F.d_rpf_range; sh.dq.dc_range = F.d_dc_range;
        sh.dq.half_nd = rtob_dev(0.5f, F.d_rpf_mant, F.d_rpf_range); sh.dq.half_dc = rtob_dev(0.5f, F.d_dc_mant, F.d_dc_range);
        if (F.pred_on && F.d_coeff_size > FC_MAXCOEFF_BIG) sh.failed = FC_ERR_INTERNAL;
#endif
#if FC_VARIANT_BIG
        if (F.bx) sh.states = F.basis_states;        /* tables: basis_init_bx below, all lanes */
        else
#else
        if (F.bx) sh.failed = FC_ERR_INTERNAL;       /* a long basis needs a big build (core_hip.cpp routes) */
#endif
        basis_init(F, sh);
        /* root range (codec/coder.c:738-745) */
        sh.flim = 0;
        sh.par.lc_max = F.lc_max; sh.par.width = F.width; sh.par.height = F.height;
        sh.par.limit_states = F.limit_states; sh.par.PA = F.PA; sh.par.P = F.P; sh.par.ML = F.ML;
        sh.par.price = F.price; sh.par.chroma_decrease = F.chroma_decrease;
        sh.par.gram = F.gram; sh.par.gram_ls = F.gram_ls; sh.par.diag = F.diag; sh.par.ipis = F.ipis; sh.par.pos = F.pos;
        sh.par.gcol = F.gcol;
        sh.par.d5 = F.d5; sh.par.d4 = F.d4;
        sh.par.at_tree = F.tree; sh.par.at_into = F.into; sh.par.at_pool = F.pool_states; sh.par.at_weight = F.weight;
        sh.par.at_final = F.final_d; sh.par.at_los = F.level_of_state; sh.par.at_dtype = F.domain_type;
        sh.par.at_ycol = F.ycol; sh.par.at_x = F.x; sh.par.at_y = F.y; sh.par.color = F.color;
        sh.par.l2_keys = F.l2_keys; sh.par.l2_vals = F.l2_vals; sh.par.l2_mask = F.l2_mask;
        sh.par.max_elements = F.max_elements; sh.par.rpf_mant = F.rpf_mant; sh.par.dc_mant = F.dc_mant;
        sh.par.sy = F.sy; sh.par.dcs = F.dcs; sh.par.gl0 = F.gl0; sh.par.images_level = F.images_level;
        sh.par.lc_min_opt = F.lc_min; sh.par.trace_on = F.trace != nullptr;
        sh.par.rpf_range = F.rpf_range; sh.par.dc_range = F.dc_range;
        sh.par.half_nd = rtob_dev(0.5f, F.rpf_mant, F.rpf_range); sh.par.half_dc = rtob_dev(0.5f, F.dc_mant, F.dc_range);
        sh.band = 0; sh.lc_min = F.lc_min; sh.after_chroma = 0; sh.ystates = 0;
        push_root(F, sh, RANGE_);
        sh.op = OP_NOP;                      /* first pass: no parallel op, just run the search */
    }
    if (F.color)                              /* calloc'ed in the reference (codec/wfa.h) */
        for (int i = tid; i < 2 * F.PA; i += B) F.ycol[i] = F.ycol0 ? F.ycol0[i] : (uint8_t) 0;
#if FC_VARIANT_BIG
    if (F.bx) { __syncthreads(); basis_init_bx(F, sh); }
#endif
#if FC_SPEC
    }
#endif
    /* per-op tick counters live in LDS: a private array indexed by `op` would be scratch */
    unsigned long long *tk = sh.tk;
    if (tid == 0) for (int k = 0; k < 16; k++) tk[k] = 0;
#ifdef FC_SERIAL_PROFILE
    if (tid == 0) { for (int k = 0; k < 8; k++) sh.tk_ph[k] = 0; sh.ph_prev = 0; sh.ph_t0 = 0; sh.tk_init[0] = sh.tk_init[1] = 0; for (int k = 0; k < 4; k++) sh.tk_apx[k] = 0; }
#endif
    unsigned long long t_begin = wall_clock64();
    /* everything below is inlined into this one loop (a single call site per op keeps the
     * kernel argument visible to the compiler: DevFrame fields come through scalar loads and
     * table accesses are global_load, not flat_load through a generic reference) */
#if FC_SPEC
    const unsigned T = F.spec ? (unsigned) F.spec_T : 0u;
    if (role == 0 && F.spec && G > 1) {
        /* the rows of the basis states are complete: table workers may start */
        __threadfence();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(&F.spec->s_pub, (unsigned) sh.states, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (role >= 1 && role <= T) { spec_worker(F, sh, role, T, false); return; }
    for (;;) {          /* chain: once.  Verifier: once per block it verifies, until the chain is done. */
    if (role) {
        FcSpecCtl *const c = F.spec;
        __syncthreads();
        if (tid == 0) {
            unsigned t = atomicAdd(&c->next, 1u);
            int go = 1;
            for (;;) {                  /* relaxed polls (an acquire per look drops the CU's L1 every time), ONE acquire on a find */
                const unsigned q = __hip_atomic_load(&c->slot_seq[t % FC_SPEC_W], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (q == t + 1) { take_acquire(); break; }        /* nothing stale in this CU's L1: the slot, the rows of the states */
                /* the slot already holds a LATER block: the chain went back behind block t, dropped it and has
                 * come round to the slot again before anybody looked at it.  Waiting for it would be for ever. */
                if (q > t + 1) { t = atomicAdd(&c->next, 1u); continue; }
                if (__hip_atomic_load(&c->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { go = 0; break; }
                /* colour frame, luminance band done: nothing left to verify, the chroma bands' tables to build */
                if (__hip_atomic_load(&c->chroma_ready, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) { take_acquire(); go = 2; break; }
                __builtin_amdgcn_s_sleep(32);
            }
            task_seq = t; task_go = go;
        }
        __syncthreads();
        if (task_go != 1) break;                                  /* uniform */
        {   /* the chain's LDS state at the entry of the block */
            const uint4 *src = (const uint4 *) (SPEC_SLOTS(c) + (size_t) (task_seq % FC_SPEC_W) * SPEC_STRIDE);
            for (unsigned i = tid; i < sizeof(Sh) / 16; i += B) ((uint4 *) &sh)[i] = src[i];
        }
        __syncthreads();                /* the copy is complete (its loads were waited for by the LDS stores) before lane 0 looks at the slot again */
        if (tid == 0) {
            const unsigned task_epoch = sh.sl.epoch;              /* the chain's, as of the checkpoint */
            /* the slot was not taken for a later block while it was read, and the chain has not gone
             * back behind this block since */
            bool valid = __hip_atomic_load(&c->slot_seq[task_seq % FC_SPEC_W], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == task_seq + 1
                         && __hip_atomic_load(&c->epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == task_epoch;
            sh.sl = sl_keep;
            sh.sl.epoch = task_epoch;
            const int S0 = sh.states, TB = F.spec_tb;
            if (valid && (S0 > TB || sh.sp < 0 || sh.sp >= FC_DEPTH)) valid = false;
            sh.sl.floor = sh.sp; sh.sl.verdict = 2; sh.sl.abort = valid ? 0 : 1; sh.sl.ops = 0; sh.sl.busy = 0;
            sh.sl.mode = 2 + sh.sp;
            if (sh.sp > 0) sh.st[sh.sp - 1].phase = PH_SPEC_END;     /* what the block's parent does should the block ever return */
            sh.gap_lo = S0; sh.gap_hi = TB; sh.gap_shift = TB - S0; sh.states = TB; sh.cap = TB + FC_SPEC_TEMPS;
            unsigned dm = 0;
            for (int k = 0; k < 32; k++) if (k * B >= S0 && (k + 1) * B <= TB) dm |= 1u << k;
            sh.deadmask = dm;
            sh.par.at_pool = F.pool_states;                       /* private pool list */
            sh.par.trace_on = 0;
            sh.par.color = 0;                                     /* no y_column flags from here: spec_poll */
            /* which of this workgroup's ids the search uses is read off their level entries afterwards */
            for (int k = 0; k < FC_SPEC_TEMPS; k++) F.level_of_state[TB + k] = 0;
            sh.op = valid ? OP_NOP : OP_DONE;
            if (valid) {
                atomicAdd(&c->busy, 1u);
                SPEC_DEKKER_FENCE();
                /* (the chain may have raised the epoch between the check above and this count: once more) */
                if (__hip_atomic_load(&c->epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != task_epoch) {
                    atomicSub(&c->busy, 1u); valid = false; sh.sl.abort = 1; sh.op = OP_DONE;
                } else sh.sl.busy = 1;
            }
            if (valid && !sh.tab_shared) {
                /* the chain built this block's tables in its own memory: this workgroup builds them
                 * again in its own (otherwise they are in a buffer of the ring, complete for every
                 * state below gap_lo, and the states appended here add their entries behind gap_hi) */
                const Range &rg = sh.st[sh.sp].rg;
                sh.par.ipis = F.ipis; sh.par.d5 = F.d5;
                sh.op = OP_INIT_RANGE; sh.a0 = rg.x; sh.a1 = rg.y; sh.a2 = -1;
            }
        }
    }
#endif
    for (;;) {
        __syncthreads();
        const int op = sh.op;
        if (op == OP_DONE) break;
        unsigned long long t0 = wall_clock64();
#if FC_PRIO_ROTATE
        {
            /* Four frames share a CU, one wave of each per SIMD, and the instruction arbiter takes the OLDEST ready
             * wave: the frame whose workgroup arrived first ran 18 % faster than the one that arrived last (1.52 /
             * 1.61 / 1.70 / 1.79 s by block id / 256), and a launch lasts as long as its slowest frame.  The user
             * priority (s_setprio, above age in the arbitration) of the co-resident frames rotates with the wall
             * clock -- every frame is first, second, third and last a quarter of the time -- so that they finish
             * together.  What a frame computes does not depend on when its instructions issue. */
            const unsigned pr = ((unsigned) (t0 >> FC_PRIO_SHIFT) + (blockIdx.x >> 8)) & 3u;       /* wave uniform */
            if (pr == 0) __builtin_amdgcn_s_setprio(0);
            else if (pr == 1) __builtin_amdgcn_s_setprio(1);
            else if (pr == 2) __builtin_amdgcn_s_setprio(2);
            else __builtin_amdgcn_s_setprio(3);
        }
#endif
        switch (op) {
#if FC_SPEC
        case OP_SPEC_CKPT: {
            /* a0 = 1, a block of the largest block level with its tables done: the verdicts that have
             * arrived, then the checkpoint of this block -- the complete LDS state of the chain: what a
             * verifier starts from, and what the chain returns to if its guess about the block is wrong.
             * a0 = 2, end of the band: every verdict.  Either way a verdict may send the chain back. */
            FcSpecCtl *const c = sh.sl.ctl;
            if (tid == 0) {
                int act = 0;
                const int back = spec_poll(sh, sh.a0 == 2);
                if (back) {
                    act = (back & 0x100) ? 3 : 2; spec_slot = (unsigned) ((back & 0xff) - 1);
                    spec_used = (unsigned) (back >> 16) & 63u; spec_vid = (unsigned) (back >> 24) & 7u;
                    if (act == 3) {
                        /* the state to take over is what this block's verifier left: anything else is a bug */
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                        const Sh *im = (const Sh *) (sh.sl.slots + (size_t) (FC_SPEC_W + spec_vid) * SPEC_STRIDE);
                        const int TB = im->gap_hi, S0 = im->gap_lo, m = im->states - TB;
                        int bad = 0;
                        if (S0 != (int) sh.sl.sk[spec_slot]) bad |= 1;
                        if (TB < F.spec_cap || TB + FC_SPEC_TEMPS > F.P || ((TB - F.spec_cap) % FC_SPEC_TEMPS)) bad |= 2;
                        if (m < 0 || m > FC_SPEC_TEMPS || m > (int) spec_used) bad |= 4;
                        if (im->sp < 1 || im->sp >= FC_DEPTH) bad |= 8;
                        if (im->sl.epoch != sh.sl.epoch) bad |= 16;
                        if (S0 + m > F.spec_cap) bad |= 32;
                        if (im->sl.verdict != 3 || im->failed) bad |= 64;
                        if (bad) { spec_bad |= bad; act = 2; }
                    }
                }
                else if (sh.a0 == 1) {
                    SFrame &fr = sh.st[sh.sp];
                    if (!sh.sl.nospec && fr.rg.level > sh.lc_min) { fr.ckpt = 2; act = 1; }
                } else if (sh.par.color && !sh.band && !sh.after_chroma) spec_luminance_done(sh);
                else { sh.sl.on = 0; sh.sl.mode = 0; }       /* a gray frame: it is over */
                spec_act = act;
            }
            __syncthreads();
            if (spec_act == 1) {
                const unsigned seq = sh.sl.head, slot = seq % FC_SPEC_W;
                /* (hand-off recipe at the top of the file: the waves drain, ONE lane releases -- this runs once per block
                 * of the largest level, 8 100 times per 4K frame; until round 6 every lane fenced twice here.)  The slot is
                 * marked "being written" with a write-through store that is complete before any of its new bytes exist */
                if (tid == 0) __hip_atomic_store(&c->slot_seq[slot], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                WAVE_DRAIN();
                __syncthreads();
                uint4 *dst = (uint4 *) (sh.sl.slots + (size_t) slot * SPEC_STRIDE);
                for (unsigned i = tid; i < sizeof(Sh) / 16; i += B) dst[i] = ((const uint4 *) &sh)[i];
                WAVE_DRAIN();                    /* the slot + every table row written so far: in L2 */
                __syncthreads();
                if (tid == 0) {
                    /* every table row of the states so far is complete and visible: table workers may use them */
                    publish_release();
                    __hip_atomic_store(&c->s_pub, (unsigned) sh.states, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&c->slot_seq[slot], seq + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    sh.sl.head = seq + 1; sh.sl.spec_mask &= ~(1u << slot); sh.sl.n_tasks++;
                    sh.sl.blkof[slot] = (unsigned) (sh.blk - 1);
                    sh.sl.sk[slot] = (unsigned) sh.states;
                }
            } else if (spec_act == 3) {
                /* A wrong guess whose verifier found the subdivision to win: instead of going back to the
                 * checkpoint and searching the block again, the chain takes over the verifier's state at the
                 * decision of the block -- models, stack, the block's children -- and the states its search
                 * has appended: their rows move from the verifier's ids (from TB on) to the chain's (from the
                 * block's state count on), references to them with them.  Same values as a search of the
                 * chain's own: same code on the same inputs. */
                if (tid == 0) sl_keep = sh.sl;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __syncthreads();
                const uint4 *src = (const uint4 *) (sl_keep.slots + (size_t) (FC_SPEC_W + spec_vid) * SPEC_STRIDE);
                for (unsigned i = tid; i < sizeof(Sh) / 16; i += B) ((uint4 *) &sh)[i] = src[i];
                __syncthreads();
                const int TB = sh.gap_hi, S0 = sh.gap_lo, m = sh.states - TB, shift = TB - S0;
                __syncthreads();
                if (tid == 0) {
                    sh.sl = sl_keep;
                    sh.sl.nospec = 0;
                    sh.sl.commit = sh.sl.head;
                    sh.sl.rb_s[sh.sl.epoch % 32u] = (unsigned) S0;
                    __hip_atomic_store(&c->s_pub, (unsigned) S0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    /* Rows from S0 on are about to change under every verification in flight (all void: they
                     * started from later checkpoints).  Half-moved rows must not be searched -- a state's
                     * position in the pool and the counters of a later checkpoint need not agree: first the
                     * epoch, then wait until every search has seen it.  The verifier whose rows move waits
                     * for `adopting` to clear before it uses its ids again. */
                    __hip_atomic_store(&c->adopting, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    sh.sl.epoch++;
                    __hip_atomic_store(&c->epoch, sh.sl.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    SPEC_DEKKER_FENCE();
                    while (__hip_atomic_load(&c->busy, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) __builtin_amdgcn_s_sleep(8);
                    sh.sl.n_adopted++;
                    sh.gap_lo = sh.gap_hi = sh.gap_shift = 0; sh.deadmask = 0;
                    sh.cap = F.spec_cap;
                    sh.states = S0 + m;
                    sh.par.at_pool = F.pool_states; sh.par.color = F.color; sh.par.trace_on = 0;
                    if (!sh.tab_shared) { sh.par.ipis = F.ipis; sh.par.d5 = F.d5; }
                    sh.st[sh.sp - 1].phase = PH_CHILD_RET;               /* (the verifier's terminal phase) */
                    SFrame &fr = sh.st[sh.sp];
                    fr.states = S0;
                    for (int l = 0; l < 2; l++) {
                        Range &ch = fr.child[l];
                        if (ch.tree >= TB) ch.tree -= shift;
                        for (int e = 0; e < RANGE_E; e++) if (ch.into[e] >= TB) ch.into[e] = (short) (ch.into[e] - shift);
                    }
                    if (F.color) {                                       /* see spec_poll: flags of the ids the search used */
                        GLOBAL_AS uint8_t *yc = (GLOBAL_AS uint8_t *) F.ycol;
                        for (unsigned j = 0; j < spec_used; j++) { yc[S0 + j] = 0; yc[(unsigned) F.PA + S0 + j] = 0; }
                    }
                }
                __syncthreads();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                /* the rows */
                for (int j = 0; j < m; j++) {
                    const int sid = TB + j, did = S0 + j;
                    if (tid < 2) {
                        const int l = tid;
                        const int t = TREE(F, sid, l);
                        TREE(F, did, l) = (short) (t >= TB ? t - shift : t);
                        for (int e = 0; e < 6; e++) {
                            const int d = INTO(F, sid, l, e);
                            INTO(F, did, l, e) = (short) (d >= TB ? d - shift : d);
                            WEIGHT(F, did, l, e) = WEIGHT(F, sid, l, e);
                        }
                        F.x[l * F.PA + did] = F.x[l * F.PA + sid]; F.y[l * F.PA + did] = F.y[l * F.PA + sid];
                    } else if (tid == 2) {
                        F.final_d[did] = F.final_d[sid]; F.level_of_state[did] = F.level_of_state[sid];
                        F.domain_type[did] = F.domain_type[sid];
                        const short p = F.pos[sid];
                        F.pos[did] = p;
                        if (p >= 0) F.pool_states[p] = (short) did;      /* the chain's list (the verifier kept its own) */
                    }
                    if (!F.domain_type[sid]) continue;                   /* an auxiliary state: no tables (uniform) */
                    for (int i = tid; i < F.NI; i += B) F.img[(size_t) did * F.NI + i] = F.img[(size_t) sid * F.NI + i];
                    if (tid < 32) F.imgT[(size_t) tid * F.P + did] = F.imgT[(size_t) tid * F.P + sid];
                    for (int q = 0; q < F.NL; q++) {
                        const float *Gs = GRAM(F, q) + GROW(sid, F.P);
                        float *Gd = GRAM(F, q) + GROW(did, F.P);
                        for (int t = tid; t < S0; t += B) Gd[t] = Gs[t];
                        if (tid <= j) Gd[S0 + tid] = Gs[TB + tid];
                        if (tid == 0) F.diag[(size_t) q * F.P + did] = F.diag[(size_t) q * F.P + sid];
                    }
                }
                __threadfence();
                __syncthreads();
                if (tid == 0)            /* the verifier has its ids back */
                    __hip_atomic_store(&c->adopting, 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            } else if (spec_act == 2) {
                const unsigned slot = spec_slot;
                if (tid == 0) sl_keep = sh.sl;
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __syncthreads();
                const uint4 *src = (const uint4 *) (sl_keep.slots + (size_t) slot * SPEC_STRIDE);
                for (unsigned i = tid; i < sizeof(Sh) / 16; i += B) ((uint4 *) &sh)[i] = src[i];
                __syncthreads();
                if (tid == 0) {
                    sh.sl = sl_keep;
                    sh.sl.nospec = 1;                     /* this block is searched here */
                    sh.sl.commit = sh.sl.head;            /* every verification in flight is void ... */
                    /* the rows of the states from here on will be written again: tables computed from them
                     * in this epoch or before count up to here only (spec_tables), and nothing beyond is
                     * offered to the table workers until the next checkpoint */
                    sh.sl.rb_s[sh.sl.epoch % 32u] = (unsigned) sh.states;
                    __hip_atomic_store(&c->s_pub, (unsigned) sh.states, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    sh.sl.epoch++;                        /* ... and its verifier should drop it */
                    __hip_atomic_store(&c->epoch, sh.sl.epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                    SPEC_DEKKER_FENCE();
                    /* ... before the search here appends a state: rows from this state count on, read by a
                     * search that has not looked at the epoch yet, would change under it */
                    while (__hip_atomic_load(&c->busy, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) __builtin_amdgcn_s_sleep(8);
                }
                __syncthreads();
                /* the checkpoint was taken with the block's tables done.  In a buffer of the ring they still
                 * are; the chain's own tables have been those of later blocks since: once more */
                if (!sh.tab_shared) op_init_range(F, sh, sh.st[sh.sp].rg.x, sh.st[sh.sp].rg.y, 0);
                /* Verdicts that do not come (every wait for one is bounded, but 0.2 s each): the verifiers are
                 * not resident, or too few for a chain this fast.  Three of them and this frame goes on
                 * without guesses -- one workgroup, as if it had no others. */
                if (tid == 0 && sh.sl.n_timeout >= 3) { sh.sl.on = 0; sh.sl.mode = 0; }
            }
            break;
        }
#endif
#if FC_SPEC
        case OP_INIT_RANGE:
            if (((sh.sl.on && sh.sl.T > 0) || sh.sl.chroma_tabs) && sh.sl.role == 0 && sh.a2 >= 0) spec_tables(F, sh, sh.a2);
            else if (tid == 0) { sh.tab_from = 0; if (sh.sl.role == 0) { sh.par.ipis = F.ipis; sh.par.d5 = F.d5; sh.tab_shared = 0; } }
            __syncthreads();
            op_init_range(F, sh, sh.a0, sh.a1, sh.tab_from);
            break;
#else
        case OP_INIT_RANGE: op_init_range(F, sh, sh.a0, sh.a1, 0); FC_DUP(OP_INIT_RANGE, op_init_range(F, sh, sh.a0, sh.a1, 0)); break;
#endif
        case OP_APPROX:     op_approx(F, sh); break;
        case OP_IPIS_INCR:  op_ipis(F, sh, sh.a0, sh.a1, sh.a2, sh.a3); FC_DUP(OP_IPIS_INCR, op_ipis(F, sh, sh.a0, sh.a1, sh.a2, sh.a3)); break;
        case OP_APPEND:     op_append(F, sh, sh.a0); FC_DUP(OP_APPEND, op_append(F, sh, sh.a0)); break;
        case OP_CHROMA:
            op_chroma_pool(F, sh);
#if FC_SPEC
            if (sh.sl.chroma_tabs) {                 /* uniform: the luminance dictionary is final and visible */
                __threadfence();
                __syncthreads();
                if (tid == 0) {
                    FcSpecCtl *c = sh.sl.ctl;
                    c->ystates = (unsigned) sh.ystates;
                    __hip_atomic_store(&c->chroma_ready, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
#endif
            break;
#if FC_VARIANT_BIG
        case OP_PRED_SETUP:  op_pred_setup(F, sh, sh.a0, sh.a1); break;
        case OP_PRED_FINISH: op_pred_finish(F, sh, sh.a0); break;
        case OP_NORMS:       op_norms(F, sh, sh.a0, sh.a1, sh.a2, sh.a3); break;
        case OP_MC_SEARCH:   op_mc_search(F, sh, sh.a0, sh.a1, sh.a2); break;
#endif
        default: break;                      /* OP_NOP */
        }
        __syncthreads();
#if FC_SPEC
        if (tid == 0 && role && (++sh.sl.ops & 1u) == 0
            && __hip_atomic_load(&F.spec->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != sh.sl.epoch) {
            sh.sl.abort = 1; sh.op = OP_DONE;         /* the chain has gone back behind this block */
        } else
#endif
        if (tid == 0) {                       /* partition search, lane 0 */
            unsigned long long t1 = wall_clock64();
            tk[op] += t1 - t0;
#ifdef FC_SERIAL_PROFILE
            sh.ph_t0 = t1;
#endif
            serial_advance(F, sh);
#ifdef FC_SERIAL_PROFILE
            { unsigned long long t = wall_clock64(); sh.tk_ph[sh.ph_prev] += t - sh.ph_t0; }
#endif
            tk[0] += wall_clock64() - t1;
        }
    }
#if FC_SPEC
    if (!role) break;
    __syncthreads();
    /* A search of a block the chain has dropped meanwhile may get here without having looked at the epoch
     * (it does every few operations): its result slot is the slot of a LATER block by now -- it must not
     * write there.  (A return raises the epoch long before the later block's own result can be written:
     * what still slips through between this look and the copy lands first and is overwritten.) */
    if (tid == 0 && !sh.sl.abort
        && __hip_atomic_load(&F.spec->epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != sh.sl.epoch) sh.sl.abort = 1;
    __syncthreads();
    if (!sh.sl.abort && sh.sl.verdict == 3) {            /* uniform: this workgroup's state, for the chain to take over */
        /* (a buffer per verifier, behind the checkpoint slots: nobody else ever writes it, and this workgroup
         * not again before the chain has read it -- see the wait below) */
        uint4 *dst = (uint4 *) (SPEC_SLOTS(F.spec) + (size_t) (FC_SPEC_W + (role - T - 1)) * SPEC_STRIDE);
        for (unsigned i = tid; i < sizeof(Sh) / 16; i += B) dst[i] = ((const uint4 *) &sh)[i];
        __threadfence();                                 /* + the rows of the states the search has appended */
        __syncthreads();
    }
    if (tid == 0) {
        if (!sh.sl.abort) {
            /* (seq + 1) << 11 | verifier << 8 | ids the search used << 2 | verdict */
            unsigned used = 0;
            while (used < FC_SPEC_TEMPS && F.level_of_state[sh.gap_hi + (int) used] != 0) used++;
            __hip_atomic_store(&F.spec->verdict[task_seq % FC_SPEC_W],
                               ((task_seq + 1) << 11) | ((role - T - 1) << 8) | (used << 2) | (unsigned) sh.sl.verdict,
                               __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (sh.sl.busy) { __threadfence(); atomicSub(&F.spec->busy, 1u); }      /* its rows are written */
        if (!sh.sl.abort && sh.sl.verdict == 3) {
            /* the rows of the states this search appended wait under this workgroup's ids for the chain to
             * move them: no new search (it would write the same ids) before the chain has -- it raises the
             * epoch when it is done with them, as it does when it drops the block for another reason */
            while (__hip_atomic_load(&F.spec->epoch, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) == sh.sl.epoch
                   && __hip_atomic_load(&F.spec->committed, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) <= task_seq
                   && !__hip_atomic_load(&F.spec->done, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT))
                __builtin_amdgcn_s_sleep(16);
            while (__hip_atomic_load(&F.spec->adopting, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) __builtin_amdgcn_s_sleep(16);
        }
    }
    }
    if (role) {
        if (task_go == 2) spec_worker(F, sh, role, T, true);
        return;
    }
    if (tid == 0 && sh.sl.ctl && G > 1) {
        FcSpecCtl *const c = sh.sl.ctl;
        /* verifiers that are still at a block the chain went back behind drop it; the others leave */
        __hip_atomic_store(&c->epoch, sh.sl.epoch + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&c->done, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        c->n_tasks = sh.sl.n_tasks; c->n_confirmed = sh.sl.n_confirmed; c->n_wrong = sh.sl.n_wrong;
        c->n_timeout = sh.sl.n_timeout; c->n_inline = sh.sl.n_inline; c->t_wait = sh.sl.t_wait;
        c->n_tab_used = sh.sl.n_tab_used; c->n_tab_missed = sh.sl.n_tab_missed; c->n_adopted = sh.sl.n_adopted;
        c->n_app_dealt = sh.sl.n_app_dealt; c->t_app_wait = sh.sl.t_app_wait;
    }
#endif
    if (tid == 0) {
        F.t_serial = tk[0]; F.t_init = tk[OP_INIT_RANGE]; F.t_approx = tk[OP_APPROX];
        F.t_ipis = tk[OP_IPIS_INCR]; F.t_append = tk[OP_APPEND];
        F.t_total = wall_clock64() - t_begin;
        F.bytes_mp = sh.cnt.bytes_mp; F.bytes_img = sh.cnt.bytes_img; F.bytes_gram = sh.cnt.bytes_gram;
        F.n_mp = sh.cnt.n_mp; F.n_steps = sh.cnt.n_steps; F.n_blocks = sh.cnt.n_blocks;
        F.n_appends = sh.cnt.n_appends; F.n_fulleval = sh.cnt.n_fulleval;
        F.n_blockevals = sh.cnt.n_blockevals; F.t_mpA = sh.cnt.t_mpA; F.t_mpB = sh.cnt.t_mpB;
#if FC_VARIANT_BIG && !defined(FC_SERIAL_PROFILE)
        /* the ops only this build has (ticks): chroma set-up, prediction set-up / finish, norms, motion search */
        F.dbg[2] = tk[OP_CHROMA]; F.dbg[3] = tk[OP_PRED_SETUP]; F.dbg[4] = tk[OP_PRED_FINISH];
        F.dbg[5] = tk[OP_NORMS]; F.dbg[6] = tk[OP_MC_SEARCH];
#endif
#ifdef FC_SERIAL_PROFILE
        for (int k = 0; k < 8; k++) F.dbg[k] = sh.tk_ph[k];
        F.dbg[0] = sh.tk_init[0]; F.dbg[7] = sh.tk_init[1];      /* d5 / ipis of init_range */
        /* OP_APPROX: tables, init, steps, finalize (replace the CHILD* phase slots) */
        F.dbg[3] = sh.tk_apx[0]; F.dbg[4] = sh.tk_apx[1]; F.dbg[5] = sh.tk_apx[2]; F.dbg[2] = sh.tk_apx[3];
#endif
    }
#if FC_SPEC && !defined(FC_SERIAL_PROFILE)
    if (tid == 0) { F.dbg[0] = tk[OP_SPEC_CKPT]; F.dbg[1] = 0; }   /* ticks of the chain in checkpoints, verdicts and returns */
#endif
    if (tid == 0) {
        /* per-band results and the root state were recorded by band_advance() */
#if FC_VARIANT_BIG && !FC_SPEC
        if (sh.coopW > 1 && F.coop) __hip_atomic_store(&F.coop->quit, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
        F.states = sh.states;
        F.ystates_out = sh.band ? sh.ystates : sh.states;
        F.lc_min_out = sh.lc_min;
        F.status = sh.failed ? sh.failed : FC_OK;
#if FC_SPEC
        if (spec_bad) F.status = 128 + spec_bad;
#endif
    }
    if (F.pack_dst) {                         /* the automaton for the host writer, packed */
        const uint4 *src = (const uint4 *) F.pack_src;
        uint4 *dst = (uint4 *) F.pack_dst;
        const unsigned n16 = F.pack_bytes / 16;
        for (unsigned i = tid; i < n16; i += B) dst[i] = src[i];
    }
#if !FC_SPEC
    if (ring) {                               /* the slab is free for the next frame without one */
        __threadfence();
        __syncthreads();
        if (tid == 0) {
            const unsigned i = atomicAdd(&ctr[1], 1u);
            __hip_atomic_store(&ring[i], (unsigned long long) F.slab_base, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#endif
}

/* workgroups of this build a CU holds at once: what the build was compiled for (its launch bound
 * caps the registers) unless its LDS allows fewer.  The launcher sizes the frame queue and the
 * number of slabs by it.  (hipOccupancyMaxActiveBlocksPerMultiprocessor answered 1 and 2 for
 * builds that demonstrably run 4 and 5 workgroups per CU: not used.) */
extern "C" int FC_OCCUPANCY(void)
{
    const int by_lds = (int) (163840 / sizeof(Sh));
    return by_lds < FC_WG_PER_CU ? (by_lds < 1 ? 1 : by_lds) : FC_WG_PER_CU;
}

#if FC_SPEC
/* n frames, G workgroups each (all n * G must be resident at once: a chain whose verifiers are not
 * does their blocks itself after a bounded wait, see spec_poll) */
extern "C" void FC_LAUNCH(DevFrame *d_frames, DevFrame *d_vframes, unsigned n, unsigned G, unsigned H, hipStream_t stream)
{
    /* ... and H append helpers per frame behind them (FcSpecCtl.app_H of every frame of the launch; 0: none) */
    hipLaunchKernelGGL(FC_KERNEL, dim3(n * (G + H)), dim3(B), 0, stream, d_frames, d_vframes, G, n, H);
}
extern "C" unsigned FC_SPEC_SLOT_BYTES(void) { return SPEC_STRIDE; }
#if !FC_VARIANT_WIDE
extern "C" unsigned fc_spec_ctl_bytes(void) { return (unsigned) ((sizeof(FcSpecCtl) + 255) / 256 * 256); }
#endif
#else
extern "C" void FC_LAUNCH(DevFrame *d_frames, unsigned n, unsigned nlend, unsigned long long *ring, unsigned *ctr,
                          const unsigned *ptrmask, unsigned long long queue_wait_ticks, unsigned coopW, hipStream_t stream)
{
    /* coopW > 1 (big builds, no queue): coopW workgroups per frame, frames in groups of eight (kernel entry) */
    const unsigned grid = coopW > 1 ? (n + 7) / 8 * 8 * coopW : n;
    hipLaunchKernelGGL(FC_KERNEL, dim3(grid), dim3(B), 0, stream, d_frames, nlend, ring, ctr, ptrmask, queue_wait_ticks, coopW);
}
#endif
