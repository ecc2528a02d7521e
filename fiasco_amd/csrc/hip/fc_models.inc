/*
 *  fc_models.inc -- where model snapshots live (SNAP_AT, TM_AT, ...); the generic models of the
 *  FC_GM build (gq_*, gm_*); the snapshots all lanes copy around a linear combination
 *  (snap_coop_*); the declaration of tree_bits_dev (defined in fc_serial.inc).
 *
 *  Reference: rle pool / aac / tree codec/domain-pool.c:621-852, codec/coeff.c:215-267;
 *  rate models codec/bintree.c:35-73.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

#if FC_VARIANT_BIG
#define SNAP(sh) ((sh).snap)
#define NSLOT(sh) ((sh).nslot)
#define SNAP_TM(sh) ((sh).snap_tm_p)
#define TM_SLOTS(sh) ((sh).nslot == 5 ? 2 : 1)
#else
#define SNAP(sh) ((sh).snap_pool)
#define NSLOT(sh) 2
#define SNAP_TM(sh) ((uint4 *) (sh).snap_tm)
#define TM_SLOTS(sh) 1
#endif
/* aac snapshot slots of a depth: 0 entry, 1 after the linear combination; with prediction (big
 * build) 2 = resting model at entry, 3 / 4 = active / resting model after the recursion
 * (rec_coeff_model, rec_d_coeff_model of predict_range) */
#if FC_VARIANT_BIG
#define SNAP_AT(sh, depth, which) (SNAP(sh) + ((depth) * NSLOT(sh) + (which)) * (sh).n16)
#else
/* slot 0 of depth d is slot d; slot 1 exists for the block levels with children only and follows
 * the depth slots: snap_b1 + d (the depth of a node is frame level - node level) */
#define SNAP_AT(sh, depth, which) (SNAP(sh) + ((which) ? (sh).par.snap_b1 + (depth) : (depth)) * (sh).n16)
#endif
/* tree-model snapshots: slot 0 entry, slot 1 (prediction) after the recursion */
/* uint4 per tree-model snapshot: both models (4 ML words) in the big build, the first one in the
 * default build */
#if FC_VARIANT_BIG
#define TM_N16(ML) (ML)
#else
#define TM_N16(ML) ((2 * (ML) + 3) / 4)
#endif
#define TM_AT(sh, depth, which, ML) (SNAP_TM(sh) + ((depth) * TM_SLOTS(sh) + (which)) * TM_N16(ML))

#if FC_GM
/* ---- generic models (frame_coder.h FC_GM) ------------------------------------------------------------
 * The two model sets keep ONE list of states (F.pool_states, F.pos) like the two `rle' pools of the other builds:
 * every pool that keeps a list takes the states it is offered in the same order until it is full
 * (codec/subdivide.c:571-581; rle_append codec/domain-pool.c:832-852, qac_append :448-464, default_append
 * :957-962), so the list of a pool is the first Pool.n entries of the common one.  A `uniform' pool has no model:
 * its list is every usable state (:578-590), Pool.n counts them; the `constant' pool is the list {0} (:518-528). */

__device__ __forceinline__ float gm_m0(const Sh &sh, int idx) { return sh.m0tab[qac_shift(idx)]; }   /* matrix_0, domain-pool.c:970-999 */
__device__ __forceinline__ float gm_m1(int idx) { return (float) qac_shift(idx); }                   /* matrix_1 */

/* lane 0: n probability indices, 16 bytes at a time (the arrays are P int16 apart, P a multiple of 64) */
__device__ void gq_copy(int16_t *dst, const int16_t *src, int n)
{
    const int n16 = (n + 7) / 8;
    for (int i = 0; i < n16; i++) ((uint4 *) dst)[i] = ((const uint4 *) src)[i];
}
/* qac_model_duplicate (codec/domain-pool.c:318-331) beside the copy of the Pool struct: lane 0 */
__device__ void gq_save(Sh &sh, int set, int depth, int slot)
{
    if (GM_QAC(sh.gm.pk[set])) gq_copy(GQ_SNAP(sh, depth, slot), GQ_CUR(sh, set), set ? sh.dpool.n : sh.pool.n);
}
__device__ void gq_load(Sh &sh, int set, int depth, int slot)      /* AFTER the Pool struct is back: its n says how many */
{
    if (GM_QAC(sh.gm.pk[set])) gq_copy(GQ_CUR(sh, set), GQ_SNAP(sh, depth, slot), set ? sh.dpool.n : sh.pool.n);
}
/* the same by all lanes of the workgroup */
__device__ __forceinline__ void gq_save_par(Sh &sh, int set, int depth, int slot)
{
    if (!GM_QAC(sh.gm.pk[set])) return;
    const int n = set ? sh.dpool.n : sh.pool.n;
    int16_t *d = GQ_SNAP(sh, depth, slot);
    const int16_t *c = GQ_CUR(sh, set);
    for (int i = threadIdx.x; i < n; i += B) d[i] = c[i];
}

/* would the pool take another state?  (the constant and the uniform pool take everything) */
__device__ __forceinline__ bool gm_accepts(const Pool &m, int kind)
{
    return kind == FC_PK_CONSTANT || kind == FC_PK_UNIFORM || m.n < m.max_domains;
}
/* ->append; true: the pool's list grew */
__device__ bool gm_take(Sh &sh, Pool &m, int kind, int set, int state)
{
    if (kind == FC_PK_CONSTANT) return false;
    if (kind != FC_PK_UNIFORM && m.n >= m.max_domains) return false;
    if (GM_QAC(kind)) { int16_t *q = GQ_CUR(sh, set); q[m.n] = m.n > 0 ? q[m.n - 1] : (int16_t) 0; }
    if (GM_RLE(kind) && state == 0) { m.d0_index = 0; m.d0_n = 1; }
    m.n++;
    return true;
}
/* a non-auxiliary state is offered to both pools (both of normal_domains / delta_domains are on) */
__device__ void gm_offer(DevFrame &F, Sh &sh, int s)
{
    const int L = sh.pool.n > sh.dpool.n ? sh.pool.n : sh.dpool.n;        /* length of the common list */
    bool grow = gm_take(sh, sh.pool, sh.gm.pk[0], 0, s);
    if (F.pred_on) grow = gm_take(sh, sh.dpool, sh.gm.pk[1], 1, s) || grow;
    F.pos[s] = -1;
    if (grow) { F.pos[s] = (short) L; F.pool_states[L] = (short) s; }
}
#endif

/* the same snapshots taken by the whole workgroup around a linear-combination search
 * (codec/subdivide.c:188-237): before it, models -> slot 0 (+ tree model); after it, models ->
 * slot 1 and slot 0 -> models.  One 16-byte element per lane. */
__device__ __forceinline__ void snap_coop_before(Sh &sh, SFrame &fr, int depth, int ML)
{
    const int tid = threadIdx.x;
#if FC_HM
    for (int i = tid; i < sh.n16; i += B) SNAP_AT(sh, depth, 0)[i] = ((const uint4 *) &sh.cb)[i];
    if (tid >= 96 && tid < 96 + TM_N16(ML)) TM_AT(sh, depth, 0, ML)[tid - 96] = ((const uint4 *) sh.tm)[tid - 96];
    if (tid == 128) fr.pool0 = sh.pool;
#if FC_GM
    /* The reference duplicates all four models at every node (codec/subdivide.c:185-192).  Inside a residual search
     * the resting (normal) models are not touched -- except that the normal pool is offered the states the search
     * appends (gm_offer): its length goes back with the active pool's */
    if (tid == 130) fr.rn0 = sh.dpool.n;
    gq_save_par(sh, 0, depth, 0);
#endif
    if (sh.nslot == 5 && !fr.delta) {
        if (tid == 129) fr.dpool0 = sh.dpool;
        for (int i = tid; i < sh.n16; i += B) SNAP_AT(sh, depth, 2)[i] = ((const uint4 *) &sh.dcb)[i];
#if FC_GM
        gq_save_par(sh, 1, depth, 2);
#endif
    }
    return;
#endif
    if (tid < sh.n16) SNAP_AT(sh, depth, 0)[tid] = ((const uint4 *) &sh.cb)[tid];
    else if (tid >= 96 && tid < 96 + TM_N16(ML))   /* n16 <= 82 (FC_MAXCOEFF_BIG), ML <= 26 */
        TM_AT(sh, depth, 0, ML)[tid - 96] = ((const uint4 *) sh.tm)[tid - 96];
    else if (tid == 128) fr.pool0 = sh.pool;
#if FC_VARIANT_BIG
    /* a node outside a residual search also keeps the resting (delta) models: a prediction
     * further down may change them, and this node may have to go back (subdivide.c:189-191) */
    else if (sh.nslot == 5 && !fr.delta) {
        if (tid == 129) fr.dpool0 = sh.dpool;
        else if (tid >= 160 && tid < 160 + sh.n16) SNAP_AT(sh, depth, 2)[tid - 160] = ((const uint4 *) &sh.dcb)[tid - 160];
    }
#endif
}

__device__ __forceinline__ void snap_coop_after(Sh &sh, SFrame &fr, int depth)
{
    const int tid = threadIdx.x;
#if FC_HM
    for (int i = tid; i < sh.n16; i += B) {
        SNAP_AT(sh, depth, 1)[i] = ((const uint4 *) &sh.cb)[i];
        ((uint4 *) &sh.cb)[i] = SNAP_AT(sh, depth, 0)[i];
    }
#if FC_GM
    if (GM_QAC(sh.gm.pk[0])) {           /* pool_lc <- the pool after the combination; the pool <- pool0 (below) */
        const int n1 = sh.pool.n, n0 = fr.pool0.n;
        int16_t *cur = GQ_CUR(sh, 0), *s1 = GQ_SNAP(sh, depth, 1);
        const int16_t *s0 = GQ_SNAP(sh, depth, 0);
        for (int i = tid; i < (n1 > n0 ? n1 : n0); i += B) {
            if (i < n1) s1[i] = cur[i];
            if (i < n0) cur[i] = s0[i];
        }
    }
    __syncthreads();                     /* sh.pool.n was read above: it changes now */
#endif
    if (tid == 128) {
#else
    if (tid < sh.n16) {
        SNAP_AT(sh, depth, 1)[tid] = ((const uint4 *) &sh.cb)[tid];
        ((uint4 *) &sh.cb)[tid] = SNAP_AT(sh, depth, 0)[tid];
    } else if (tid == 128) {
#endif
        fr.pool_lc = sh.pool;
        sh.pool = fr.pool0;
#if FC_GM
        if (fr.delta) sh.dpool.n = (unsigned short) fr.rn0;
#endif
    }
}

__device__ float tree_bits_dev(const Sh &sh, int ML, int child, int level, int which);
