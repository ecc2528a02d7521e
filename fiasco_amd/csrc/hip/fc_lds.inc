/*
 *  fc_lds.inc -- the LDS layout of a frame's workgroup: the explicit stack of range records
 *  (Range, SFrame), the rle model (Pool), matching-pursuit state (MPState, RoundBox), the aac
 *  model and its snapshot pool (CoeffBuf, SNAP_POOL16) and Sh, the workgroup's whole shared state; the
 *  GM_* and GQ_* macros of the generic models and DEAD (FC_SPEC).
 *
 *  Reference: partition search codec/subdivide.c:60-502 (explicit LDS stack); rle pool / aac /
 *  tree codec/domain-pool.c:621-852, codec/coeff.c:215-267.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

/* edge slots of a range record: the vectors a build can keep plus the terminator (the stack of
 * range records is a third of the default build's LDS) */
#define RANGE_E (FC_MAXE + 1)
struct __attribute__((aligned(16))) Range {     /* copied as 128-bit LDS words by the serial lane */
    int   x, y, image, address, level, tree;
    float weight[RANGE_E];
    short into[RANGE_E];
    float err, tree_bits, matrix_bits, weights_bits;
#if FC_VARIANT_BIG
    float nd_tree_bits, nd_weights_bits, mv_tree_bits, mv_coord_bits;   /* codec/cwfa.h:68-73 */
    int   prediction;
    short mv[5];                           /* type, fx, fy, bx, by (mv_t, codec/wfa.h:58-72) */
#endif
};

struct Pool {                    /* rle model, codec/domain-pool.c:621-630 */
    short count[MAXED + 1];
    unsigned short total, n, max_domains, y_index;
    short d0_index;
    unsigned short d0_yindex, d0_n;
};

struct __attribute__((aligned(16))) SFrame {
    Range rg, lrange, rrange, child[2];
    Pool  pool0, pool_lc;
    float max_costs, lincomb, subdiv, ret, price;
    int   label, states, phase, leaf, coop;
    int   y_state, ny[2];        /* co-located luminance state of the range / of its children */
#if FC_GM
    int   rn0;                   /* Pool.n of the RESTING pool at the entry of the node (see PH_AFTER_INIT) */
#endif
#if FC_SPEC
    int   ckpt;                  /* a checkpoint of the workgroup was taken at the entry of this node */
#endif
#if FC_VARIANT_BIG
    /* prediction (codec/prediction.c:96-208): `pred` / `delta` are the arguments of the same name
     * of subdivide(); the rec_* members are what predict_range keeps of the subdivision result */
    int   pred, delta, try_pred, pred_done, rec_states;     /* try_pred: 1 nd, 2 mc */
    int   norm_first, norm_done;
    Pool  dpool0, pool_rec, dpool_rec;
    Range prange;                /* range of the residual search */
    float pred_max, pred_costs, nd_w, nd_wbits, nd_tbits;
#endif
};

struct MPState {
    int   n, best_n, index, D, N, level, image, address, row_state;
    short indices[MAXED + 1], into[MAXED + 1];
    float weight[MAXED];
    /* the RPF symbols of weight[0..2] as full_eval quantised them (SYMP_*; rtob(btor(sym)) == sym: what mp_step_prepare
     * and models_update would compute from the weights again, ~45 instructions of the serial lane apiece); an entry
     * that is not known is 0 (the scans with scratch in HBM do not carry them) */
    unsigned symp;
    float matrix_bits, weights_bits, err, costs, min_costs;
    float sel_ipdo[MAXED][MAXED];
    float norm_ov[MAXED + 1], ipio[MAXED + 1];
    short psorted[MAXED + 1];
    int   np;
    float wb_dc, wb_nd, norm, ab, price;
    int   y_state, ypos;         /* usable co-located luminance state / its list position, or -1 */
#if FC_VARIANT_BIG
    const float *numrow;         /* <range, state> row of the call: ipis slot, d5 or d4 address */
    short excl[MAXED + 1];       /* list positions excluded from this run, NOEDGE terminated */
#endif
#if FC_GM
    short kq[MAXED + 1];         /* quasi-arithmetic pools: probability index of the kept vectors' positions */
#endif
    /* per-step uniform parts of the stage-1 position pricing (mp_device.inc, StepCtx) */
    float s1_pre[MAXED], s1_sfx[MAXED], s1_z0, s1_zy;
    int   s1_last[MAXED], s1_k[MAXED], s1_thr[MAXED];
    unsigned s1_cd, s1_has;
};

/* aac model (coeff.c:190-208): totals first, then the counts, one 16-byte aligned block so
 * that a snapshot is a short run of 128-bit LDS copies */
struct __attribute__((aligned(16))) CoeffBuf {
    short tot[16];                 /* coeff_nt <= 16 contexts */
    short cnt[FC_VARIANT_BIG ? FC_MAXCOEFF_BIG : FC_MAXCOEFF];
};
#if FC_VARIANT_BIG
#define SNAP_POOL16 880            /* uint4 slots for aac snapshots: depth x 2 x n16 (what outgrows it lives in HBM) */
#define SNAP_TM_WORDS 2392         /* tree-model snapshots: depth x 4 x MAXLEVEL words */
#else
/* aac snapshots of the default build: one slot per depth (the models at the entry of the node) and
 * one more for each block level that has both a linear combination and children (the models
 * after the combination): (depths + levels) x n16 uint4.  The 256-thread build is sized for the
 * frames the stock reference accepts (level <= 22) at the CLI's models; what needs more goes to
 * the 512-thread build (one frame per CU, LDS to spare) -- core_hip.cpp routes by these numbers. */
#define SNAP_POOL16 (FC_VARIANT_WIDE ? FC_SNAP16_WIDE : FC_SNAP16_NARROW)
/* the default build never prices with the second tree model (prediction, big build only): a
 * snapshot holds the first one alone, 2 x MAXLEVEL words rounded to 16 bytes (21 depths x 13 uint4) */
#define SNAP_TM_WORDS (FC_VARIANT_WIDE ? FC_SNAPTM_WIDE : FC_SNAPTM_NARROW)
#endif
#if FC_VARIANT_BIG || FC_VARIANT_WIDE
#define NBLOCKMIN   256            /* 64-candidate blocks: D <= 16384 */
#else
#define NBLOCKMIN   64             /* the 256-thread default build is given P <= 3072 (core_hip.cpp) */
#endif
#define TM_WORDS    (4 * 26 + 8)   /* 112 words = 28 uint4 */

struct RoundBox {                    /* mp_reg.inc: winner of the running step, in LDS */
    /* running min_costs, one slot per round parity: the owner of round r publishes into
     * m2[r & 1] and everybody reads it after the round's barrier.  With a single slot a fast
     * owner of round r + 1 could overwrite the value before a slow wave has read round r's
     * (seen as rare non-deterministic streams with four frames per CU) */
    float m2[2];
    int   state;                     /* winning state or -1 */
    int   idx;                       /* its list position (list-based scan only) */
    float cost, mbits, wbits, err, f[MAXED];
    float num, den, ip[MAXED - 1];
    unsigned evals, blockevals;
    unsigned symp;                   /* MPState::symp of the winner's weights */
};
/* sym + 2 in 10 bits per weight (sym = -1 .. 511); 0 = not known: that entry is quantised again (rtob) by whoever needs it
 * -- e.g. a weight left over from another run of the same call under full_search (codec/approx.c:439-446) */
#define SYMP_NONE 0u
#define SYMP_HAS(p, k) ((k) < 3 && (((p) >> (10 * (k))) & 1023u) != 0u)
#define SYMP_GET(p, k) ((int) (((p) >> (10 * (k))) & 1023u) - 2)
#define SYMP_PUT(sym, k) ((unsigned) ((sym) + 2) << (10 * (k)))

struct Sh {
    RoundBox rb;
    SFrame   st[FC_DEPTH];
    int      sp;
    int      op, a0, a1, a2, a3;
#if FC_VARIANT_BIG
    unsigned coopW, coop_seq;      /* workgroups of this frame (FcCoop), table builds published so far */
    int      coopD, coop_minsub;   /* FcCoop.depth / .minsub */
    unsigned long long coop_ticks; /* FcCoop.done_ticks */
#endif
    Pool     pool;
    CoeffBuf cb;
#if FC_VARIANT_BIG
    /* the second set of models (d_domain_pool, d_coeff; codec/coder.c:716-736).  The two `rle'
     * pools hold the same state list at all times (every state is offered to both,
     * codec/subdivide.c:571-581), only the counters differ: pool_states / pos are shared.
     * sh.pool / sh.cb / the quantiser in sh.par are the ACTIVE set: the normal models, or the
     * delta models while the residual of a predicted range is searched (swapped in and out by
     * OP_PRED_SETUP / OP_PRED_FINISH); the other set rests in dpool / dcb / dq. */
    Pool     dpool;
    CoeffBuf dcb;
    struct { int rpf_mant, dc_mant, sy, dcs; float rpf_range, dc_range; int half_nd, half_dc; } dq;
    int      nslot;                /* aac snapshot slots per depth: 2, or 5 with prediction */
    uint4   *snap_tm_p;            /* tree-model snapshots: snap_tm, or HBM with prediction */
    int      pred_active, pred_lo, pred_rec;   /* a residual search is running; displaced ids */
    struct { int type, fx, fy, bx, by; float bits, tree_bits; } mc;      /* result of OP_MC_SEARCH */
    unsigned long long mcred[B / 64];
    unsigned pred_saved[FC_MAXSAVE / 32];      /* their table rows are in the save area */
#endif
    uint4    snap_pool[SNAP_POOL16];
    uint4   *snap;                 /* snapshots live here: snap_pool, or HBM when they outgrow it */
    int      n16;                  /* uint4 per aac snapshot */
    __attribute__((aligned(16))) unsigned tm[TM_WORDS];
    __attribute__((aligned(16))) unsigned snap_tm[SNAP_TM_WORDS];
    float    m0tab[12];
    double   lgdc[FC_MAXSYM], lglv[FC_MAXSYM], lglv_m1;
    float    Ltab[MAXED + 1];
    float    Q0, Q1;
    float    tb[2];                /* default build: tree_bits (LEAF, CHILD) of the level being approximated (mp_tables) */
    MPState  mp;
#if FC_VARIANT_BIG
    MPState  mp_keep;              /* best result so far of a call with retries */
    int      apx_stage, apx_it, apx_more;   /* retry plan of approximate_range (lane 0) */
#endif
    float    blockmin[NBLOCKMIN];
    /* 16-byte aligned: op_d5 reads the block's pixels with 128-bit LDS loads (a member added in front of them in round 6
     * shifted them by four bytes: init_range +10 %) */
    __attribute__((aligned(16))) float pixels[FC_PIXELS];
    float    norms[FC_PIXELS / 32];  /* squared norms of the sub-blocks, heap order (NS <= 127) */
    unsigned long long tk[16];     /* ticks per op (lane 0) */
    struct {
        unsigned long long bytes_mp, bytes_img, bytes_gram, n_mp, n_steps, n_blocks, n_appends,
                           n_fulleval, n_blockevals, t_mpA, t_mpB;
    } cnt;                         /* DevFrame counters of the same names */
#ifdef FC_SERIAL_PROFILE
    unsigned long long tk_ph[8], ph_t0, tk_init[2], tk_apx[4];
    int      ph_prev;
#endif
    /* colour frames (codec/coder.c:775-800): band being coded, its dynamic minimum block
     * level, root states of the finished bands, states that own tables (= end of Y band) */
    int      band, lc_min, tree_band[3], ystates, after_chroma;
    short    dl[64];               /* candidate list of a chroma call: pool + luminance state */
#if !FC_SPEC
    /* chroma bands: the states whose <sub-block, state> entries of the current block anybody reads (chroma_need) */
    short    cl[FC_CLMAX];
    int      cln;
#endif
    unsigned long long red[B / 64];
    /* term lists of the state being appended (uniform for the whole workgroup) */
    int      gs_idx[2][MAXED + 1], gs_n[2], gs_c[2], gs_raw_idx[2][MAXED + 1];
    float    gs_raw_w[2][MAXED + 1];
    float    gs_w[2][MAXED + 1];
    /* parameters the serial lane reads per range, copied from the frame descriptor once (a
     * field of the descriptor is a global-memory round trip in the out-of-line search code) */
    struct {
        int lc_max, width, height, limit_states, PA, P, ML; float price, chroma_decrease;
        /* the same for the matching pursuit: table bases and quantiser parameters */
        float *gram, *diag, *ipis; int16_t *pos; unsigned gram_ls;
        float *gcol;               /* triangular build: DevFrame.gcol */
        float *d5, *d4;            /* big build: the active level-5 / level-4 dot tables */
        const unsigned *l2_keys; const double *l2_vals; unsigned l2_mask;
        int max_elements, rpf_mant, dc_mant, sy, dcs, gl0, images_level, lc_min_opt, trace_on;
        int snap_b1;               /* default build: first "after the linear combination" snapshot slot minus its depth */
        /* automaton arrays for the serial lane: through the frame descriptor (a generic reference in
         * the out-of-line search code) every access is a flat_ instruction behind a descriptor read */
        int16_t *at_tree, *at_into, *at_pool; float *at_weight, *at_final; uint8_t *at_los, *at_dtype, *at_ycol;
        uint16_t *at_x, *at_y; int color;
        float rpf_range, dc_range;
        /* rtob(0.5) in the two RPF formats of the ACTIVE coefficient model: the symbol of the placeholder weight of
         * the stage-1 estimates (codec/approx.c:457) -- a constant of the frame (and of the model set), not of the call */
        int half_nd, half_dc;
    } par;
#if FC_GM
    /* generic models (frame_coder.h FC_GM): kinds of the ACTIVE [0] and the resting [1] model set (pool, coefficients),
     * which of the two current probability-index arrays of DevFrame.gq is the active set's, and -- per call of the
     * matching pursuit -- the price of the empty domain list, of the kept vectors of the running step, log2(1 / n) */
    struct { int pk[2], ck[2], qa; float base, kept; double lg1; int16_t *gq; int P; } gm;
#endif
    int      states;               /* wfa->states */
    int      flim;                 /* Gram tables: states below it have mirrored entries */
    int      failed;
#if FC_SPEC
    /* A verifier sees the states the frame had at the entry of its block, [0, gap_lo), and the
     * states its own search appends, which get ids from gap_hi on (a private index range of every
     * table of the shared slab); the ids in between belong to the chain, which is ahead and still
     * writes them: nothing may look at them.  Chain: gap_lo == gap_hi == 0. */
    int      gap_lo, gap_hi, gap_shift;        /* gap_shift = gap_hi - gap_lo: what the gap adds to a state count */
    unsigned deadmask;             /* scan slots (B candidates each) that lie inside the gap */
    int      cap;                  /* state ids of this workgroup end here (FC_ERR_CAPACITY) */
    int      blk;                  /* chain: blocks of the largest block level entered so far (index into the host's list) */
    int      tab_shared;           /* the block's tables are in a buffer of the frame's ring (sh.par.ipis / d5) */
    int      tab_from;
    struct SpecLocal {
        FcSpecCtl *ctl;
        char     *slots;           /* FC_SPEC_W checkpoints of sizeof(Sh) bytes */
        int       role, on;        /* 0 chain, 1 .. T table workers, then verifiers; on: the frame speculates at all */
        int       mode;            /* the same for the partition search: 0, 1 (chain, on), 2 + floor (verifier) */
        int       T;
        int       chroma_tabs;     /* chain, chroma bands of a colour frame: the other workgroups build the blocks' tables */
        char     *tabs;            /* FC_SPEC_R table buffers */
        unsigned  rb_s[32];        /* chain: state count it returned to at the end of epoch e, [e % 32] */
        unsigned  blkof[FC_SPEC_W];    /* chain: block index of the checkpoint in a slot */
        unsigned  sk[FC_SPEC_W];       /* chain: states at that checkpoint */
        unsigned long long n_tab_used, n_tab_missed, n_adopted;
        int       floor;           /* verifier: stack depth of the block it verifies */
        unsigned  head, commit;    /* chain: checkpoints published / verdicts consumed */
        unsigned  spec_mask;       /* chain: per slot, the block's subtree was left to its verifier */
        int       nospec;          /* chain: the block being entered is searched here (wrong guess before) */
        unsigned  epoch;           /* chain: its count of returns; verifier: the epoch of its task */
        int       verdict, abort, busy;  /* verifier; busy: counted in FcSpecCtl.busy */
        unsigned  ops;
        /* chain: which blocks to guess about.  A wrong guess costs the blocks the chain ran ahead plus
         * the search of the block; searching a block here costs that search alone.  The costs of a
         * block's combination tell the two kinds apart fairly well: blocks whose combination costs more
         * than SPEC_THR x the running mean over the blocks that kept theirs are searched here. */
        float     mlc, lin[FC_SPEC_W];
        unsigned  nlc;
        float     learn;           /* costs of a combination that won in a search of the chain's own, not yet in mlc */
        unsigned long long n_tasks, n_confirmed, n_wrong, n_timeout, n_inline, t_wait;
        /* chain: append helpers (FcSpecCtl.app_*): how many, from which row length, rows published, given up */
        unsigned  app_H, app_min, app_seq, app_off;
        unsigned long long n_app_dealt, t_app_wait;
    } sl;
#endif
    /* where mp_tables() stores the logarithm of a lane whose role has no double / no float entry (every lane runs the
     * same stores).  Behind everything else: a member in front of `pixels` would shift them. */
    double   sink_d;
    float    sink_f;
};
static_assert(offsetof(Sh, pixels) % 16 == 0, "op_d5 reads Sh::pixels with 128-bit LDS loads");
#if FC_GM
/* generic models: kinds, and the probability-index arrays of the quasi-arithmetic pools in DevFrame.gq */
#define GM_QAC(k)   ((k) == FC_PK_ADAPTIVE || (k) == FC_PK_BASIS)
#define GM_RLE(k)   ((k) == FC_PK_RLE || (k) == FC_PK_RLE_NO_CHROMA)
#define GQ_CUR(sh, set)          ((sh).gm.gq + (size_t) ((sh).gm.qa ^ (set)) * (sh).gm.P)       /* set 0: active, 1: resting */
#define GQ_SNAP(sh, depth, slot) ((sh).gm.gq + (size_t) (2 + (depth) * 5 + (slot)) * (sh).gm.P)
/* snapshot slots of a depth: 0 pool0, 1 pool_lc, 2 dpool0, 3 pool_rec, 4 dpool_rec (SFrame) */
#endif
#if FC_SPEC
#define DEAD(sh, s) ((unsigned) ((int) (s) - (sh).gap_lo) < (unsigned) ((sh).gap_hi - (sh).gap_lo))
#else
#define DEAD(sh, s) false
#endif
