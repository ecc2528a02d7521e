/*
 *  enc_stage.inc -- staging (included by core_hip.cpp): FrameSlot and Staged, the descriptor of a frame (fill_frame),
 *  slabs and the frame queue (stage_slot, stage_borrower, fit_hbm, stage_frames), core1_stage / core1_unstage and the
 *  replacement inputs of a staged batch (core1_upload_buffer, core1_upload_commit).
 */

/* ------------------------------------------------------------------ staging */

struct FrameSlot {
    int      job;            /* index into jobs[] */
    char    *base = nullptr;
    size_t   bytes = 0;
    int      slab_dev = -1;  /* the device that allocated the slab: goes back to the pool with it */
    int      P = 0, PA = 0;
    int      floorP = 0, floorPA = 0;   /* what frames of this kind needed before (capacity memory) */
    Layout   L;
    DevFrame F;
    bool     staged = false, done = false, big = false, rejected = false;
    bool     hm = false;         /* coefficient models of more than 64 symbols per context: the FC_HM kernel build */
    bool     gm = false;         /* models beyond rle / adaptive: the FC_GM kernel build */
    std::vector<double> lginv_host;      /* upload source of DevFrame.lginv */
    bool     wide_only = false;  /* default geometry, but beyond the 256-thread build's LDS pools */
    bool     tri = false;        /* triangular Gram tables (half the slab; the wide_tri build of the kernel) */
    bool     borrow = false;     /* no slab of its own: encoded in the slab of a queue workgroup */
    bool     spec = false;       /* several workgroups per frame (FC_SPEC build): the slab's capacity holds the
                                  * verifiers' state-id ranges */
    std::vector<uint8_t> ycol_host;      /* upload source of ycol0, alive until the slot goes */
    std::vector<int32_t> bx_host;        /* ... of DevFrame.bx */
    const int16_t *ext_pix = nullptr;    /* pixel planes outside the slab (fa_core_upload_commit) */
    const int16_t *ext_next = nullptr;   /* ... of the frames the NEXT pass encodes */
    /* the host image this pass encodes, as of its submit: fiasco_amd_batch_upload() may point
     * job->image at the NEXT pass's frames while this one is still running, and a re-stage of the
     * running pass (capacity regrow, later wave) must not read those */
    const fa_image *src = nullptr;
};

struct Staged {
    unsigned n = 0;
    fa_job  *jobs = nullptr;
    std::vector<FrameSlot> slots;
    DevFrame *d_frames = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool ok = false;
    char err[200] = "";
    int  ncu = 256;                /* CUs of the device the batch was staged for */
    /* launch in flight (fa_core_submit .. fa_core_finish) */
    std::vector<size_t>   batch;
    std::vector<DevFrame> hf;
    FcTrace *d_trace = nullptr;
    bool inflight = false, launch_failed = false, broken = false;
    int  good = 0;
    std::vector<std::pair<size_t, size_t>> to_unpack;   /* (slot, offset in pinned) */
    char  *pinned = nullptr;       /* host staging buffer for the automaton downloads */
    size_t pinned_bytes = 0;
    /* packed automata of a launch (DevFrame.pack_dst), double buffered: launch i + 1 writes the
     * other buffer while the copy of launch i is still on its way to the host */
    char  *d_pack[2] = { nullptr, nullptr };
    size_t d_pack_bytes[2] = { 0, 0 }, pack_need = 0;
    int    parity = 0;
    bool   packed = false, copy_pending = false;
    std::vector<size_t> pack_off;
    hipStream_t cstream = nullptr;
    /* replacement inputs (fa_core_upload_buffer / _commit): pinned host staging memory, two
     * device buffers used alternately (the running pass reads one, the upload fills the
     * other), a stream of their own and the event the next launch waits for */
    char  *up_host = nullptr;
    size_t up_host_bytes = 0;
    bool   up_host_shared = false;   /* the buffer belongs to the batch of several shares (MultiStaged): not freed here */
    char  *up_dev[2] = { nullptr, nullptr };
    size_t up_dev_bytes[2] = { 0, 0 };
    int    up_parity = 0;
    bool   up_pending = false;
    hipStream_t ustream = nullptr;
    hipEvent_t  ev_up = nullptr;
    /* frames handed over in device memory (input_convert.inc): the descriptor table of the conversion kernel, pinned
     * on the host and on the device, the event after its copy, and the staging buffer for sources of another device */
    char  *ic_tab = nullptr, *d_ic = nullptr;     /* entries of the kind's descriptor (IcKind::entry_bytes) */
    size_t ic_cap = 0;                            /* bytes: IC_ENTRY_MAX per slot, whatever the kind */
    hipEvent_t  ev_ic = nullptr;
    char  *peer_buf = nullptr;
    size_t peer_bytes = 0;
    char   ic_failed[200] = "";      /* why the frames of a device-fed batch could not be converted at staging */
    /* frame queue (frame_coder.hip, FC_KERNEL): frames beyond the number of resident workgroups
     * (or beyond what HBM holds in slabs) borrow the slab of whichever workgroup takes them */
    int       lender0 = -1;        /* first slot with a slab of the queue's layout */
    Layout    qL;                  /* that layout and capacity (the slot itself may be re-staged larger) */
    int       qP = 0, qPA = 0;
    bool      qbig = false, qtri = false;   /* kernel build of the queue's frames */
    size_t    lenders = 0, borrowers = 0, lender_cap = 0;
    char     *qpix = nullptr;      /* pixel planes of the borrowers */
    size_t    qpix_bytes = 0, qpix_used = 0;
    unsigned long long *d_ring = nullptr;   /* free slabs in the order they were handed back, per kernel build */
    size_t    ring_n = 0;
    unsigned *d_queue = nullptr;   /* two counters per kernel build: tickets taken, slabs handed back */
    unsigned *d_ptrmask = nullptr;
    bool      ptrmask_ready = false;
    bool      no_coop = false, no_coop_done = false;
    FcCoop    coop_hdr;               /* what a launch writes over the control blocks of its frames (source of async copies) */        /* a frame's helper workgroups did not answer (FC_ERR_COOP): one workgroup per frame from here on */
    /* block-level speculation: workgroups per frame (0 = off), the descriptors of the verifier
     * workgroups, and one buffer with -- per frame -- control block + checkpoint slots, then the
     * verifiers' private tables */
    int       specG = 0;
    int       specH[2] = { 0, 0 };    /* append helpers per frame of the launch in flight, per workgroup width (FcSpecCtl.app_*) */
    bool      no_app = false;         /* the append helpers of a frame did not answer (FC_ERR_COOP): none from here on */
    DevFrame *d_vframes = nullptr;
    size_t    vframes_n = 0;
    char     *d_spec = nullptr;
    size_t    d_spec_bytes = 0, spec_ctl_span = 0;
    std::vector<size_t> spec_frames;       /* batch positions of the speculating frames of the launch in flight */
    size_t    spec_first[2] = { 0, 0 }, spec_n[2] = { 0, 0 };    /* ... per workgroup width (256, 1024 threads) */
};

/* The kernel build of a frame in the next launch.  The wide builds take launches with no more frames than CUs
 * (`few': the chip cannot be filled with frames anyway, give each frame more lanes) and frames beyond the
 * 256-thread build's register-resident scan (more than 3072 states: 4K) or its LDS pools. */
static Build build_of(const Staged *S, const FrameSlot &fs, bool few)
{
    const bool wide_only = fs.P > 12 * 256 || fs.wide_only;
    if (fs.spec && S->specG >= 2 && !fs.borrow && !fs.tri && !fs.big && fs.P <= 12 * 1024)
        return wide_only ? B_SPEC_WIDE : B_SPEC;
    if (fs.gm) return B_BIG_GM;
    if (fs.hm) return B_BIG_HM;
    if (fs.tri) return B_WIDE_TRI;
    return (Build) ((fs.big ? B_BIG : B_DEFAULT) + (few || wide_only ? 1 : 0));
}

/* workgroups (= frames) that one CU holds at once of the build of a frame's geometry and width -- what sizes the
 * slabs and the frame queue at staging, before a launch knows its batch: a speculating or triangular-table frame
 * counts as the plain build of its width */
static size_t frames_per_cu(const FrameSlot &fs)
{
    static std::atomic<int> cache[N_BUILDS];      /* 0: not asked yet; two threads that ask at once store the same answer */
    const Build b = fs.gm ? B_BIG_GM : fs.hm ? B_BIG_HM
                  : (Build) ((fs.big ? B_BIG : B_DEFAULT) + (fs.P > 12 * 256 || fs.wide_only ? 1 : 0));
    int occ = cache[b].load(std::memory_order_relaxed);
    if (!occ) {
        occ = k_build[b].occupancy();
        if (occ < 1) occ = 1;
        cache[b].store(occ, std::memory_order_relaxed);
    }
    return (size_t) occ;
}

static inline const fa_image *slot_image(const Staged *S, const FrameSlot &fs)
{
    return fs.src ? fs.src : S->jobs[fs.job].image;
}

/* blocks of the largest block level that cover the frame */
static void fill_frame(FrameSlot &fs, const fa_job *job)
{
    const fa_cparams *cp = &job->cp;
    const fa_wfa *w = job->wfa;
    DevFrame &F = fs.F;
    const Layout &L = fs.L;
    char *base = fs.base;
    memset(&F, 0, sizeof F);
    F.price = cp->price;
    F.lc_min = (int) cp->lc_min_level; F.lc_max = (int) cp->lc_max_level;
    F.images_level = (int) cp->images_level; F.max_elements = (int) cp->max_elements;
    const bool bxl = long_basis(w);
    {
        unsigned live = cp->max_elements;
        for (unsigned st = 0; st < (bxl ? 0u : w->basis_states); st++)
            for (unsigned l = 0; l < 2; l++) {
                unsigned e = 0;
                while (e < 6 && FA_INTO(w, st, l, e) != FA_NO_EDGE) e++;
                if (e > live) live = e;
            }
        F.maxe_live = (int) live;
    }
    F.level = (int) cp->level; F.width = (int) job->image->width; F.height = (int) job->image->height;
    F.pool_max = (int) cp->pool_max_states; F.limit_states = (int) cp->limit_states;
    F.ML = (int) cp->limit_level;
    F.rpf_mant = (int) cp->rpf.mantissa_bits; F.dc_mant = (int) cp->dc_rpf.mantissa_bits;
    F.rpf_range = cp->rpf.range; F.dc_range = cp->dc_rpf.range;
    F.P = fs.P; F.PA = fs.PA;
    F.gram_ls = fs.tri ? (unsigned) ((size_t) fs.P * (fs.P + 1) / 2 + fs.P) : (unsigned) fs.P * (unsigned) fs.P;
    F.color = job->image->color ? 1 : 0;
    /* pools whose chroma list is not cut down (uniform, rle-no-chroma ...: FC_GM build) search every state: full tables */
    F.chroma_cl_cap = (int) knob_int("FIASCO_AMD_CLMAX", 0);     /* tests: the overflow path of Sh::cl */
    F.chroma_sparse = !fa_knob("FIASCO_AMD_CHROMA_FULL") && (cp->pool_kind == FA_POOL_RLE || cp->pool_kind == FA_POOL_ADAPTIVE || cp->pool_kind == FA_POOL_BASIS);
    F.chroma_max = (int) cp->chroma_max_states;
    F.chroma_decrease = cp->chroma_decrease;
    F.plane = (unsigned long long) job->image->width * job->image->height;
    F.gl0 = (int) (cp->lc_min_level < cp->images_level ? cp->lc_min_level : cp->images_level);
    F.NL = (int) cp->lc_max_level - F.gl0 + 1;
    F.second_domain_block = cp->second_domain_block ? 1 : 0;
    F.check_underflow = cp->check_for_underflow ? 1 : 0;
    F.check_overflow = cp->check_for_overflow ? 1 : 0;
    F.full_search = cp->full_search ? 1 : 0;
    F.NS = (int) fa_size_of_tree(cp->products_level);
    F.NA = 1 << (cp->lc_max_level - cp->images_level);
    F.NI = (int) fa_size_of_tree(cp->images_level);
    F.dcs = 1 << (1 + F.dc_mant); F.sy = 1 << (1 + F.rpf_mant);
    F.coeff_size = (F.lc_max - F.lc_min + 1) * F.sy + F.dcs;
    F.coeff_nt = F.lc_max - F.lc_min + 2;
    F.basis_states = (int) w->basis_states;
    F.bx = bxl ? (const int *) (base + L.bx) : nullptr;
    F.gm_pool[0] = (int) cp->pool_kind; F.gm_pool[1] = (int) cp->d_pool_kind;
    F.gm_coeff[0] = (int) cp->coeff_kind; F.gm_coeff[1] = (int) cp->d_coeff_kind;
    F.gq = fs.gm ? (int16_t *) (base + L.gq) : nullptr;
    F.lginv = fs.gm ? (const double *) (base + L.lginv) : nullptr;
    for (unsigned s = 0; s < (bxl ? 0u : w->basis_states); s++) {
        F.b_final[s] = w->final_distribution[s];
        F.b_dtype[s] = w->domain_type[s];
        for (int l = 0; l < 2; l++) {
            F.b_tree[s][l] = FA_TREE(w, s, l);
            for (int e = 0; e < 6; e++) {
                F.b_into[s][l][e] = FA_INTO(w, s, l, e);
                F.b_weight[s][l][e] = FA_WEIGHT(w, s, l, e);
                if (FA_INTO(w, s, l, e) == FA_NO_EDGE) break;
            }
        }
    }
    F.pix16 = (const int16_t *) (base + L.pix16);
    F.gram = (float *) (base + L.gram); F.diag = (float *) (base + L.diag);
    F.ipis = (float *) (base + L.ipis); F.d5 = (float *) (base + L.d5);
    F.ipt = (float *) (base + L.ipt);
    F.gcol = (float *) (base + L.gcol);
    F.d4 = (float *) (base + L.d4); F.imgT4 = (float *) (base + L.imgT4);
    F.img = (float *) (base + L.img); F.imgT = (float *) (base + L.imgT);
    F.norms = (float *) (base + L.norms);
    F.num = (float *) (base + L.num); F.den = (float *) (base + L.den);
    F.est = (float *) (base + L.est); F.ipdo = (float *) (base + L.ipdo);
    F.used = (uint8_t *) (base + L.used);
    F.tree = (int16_t *) (base + L.tree); F.into = (int16_t *) (base + L.into);
    F.weight = (float *) (base + L.weight); F.final_d = (float *) (base + L.final_d);
    F.level_of_state = (uint8_t *) (base + L.level_of_state);
    F.domain_type = (uint8_t *) (base + L.domain_type);
    F.x = (uint16_t *) (base + L.x); F.y = (uint16_t *) (base + L.y);
    F.ycol = (uint8_t *) (base + L.ycol);
    F.ycol0 = job->ycol_carry ? (const uint8_t *) (base + L.ycol0) : nullptr;
    F.pool_states = (int16_t *) (base + L.pool_states);
    F.pos = (int16_t *) (base + L.pos);
    F.hits = (int *) (base + L.hits);
    F.snap_hbm = fs.big ? (void *) (base + L.snap) : nullptr;
    F.l2_keys = g_l2.d_keys; F.l2_vals = g_l2.d_vals; F.l2_mask = g_l2.mask;
    /* prediction (codec/coder.c:716-745): gray frames try it from the root; a colour frame only
     * gets the second rle pool (intra prediction is never asked for its bands, :805-806) */
    const int inter = job->frame_type != FA_I_FRAME;
    F.pred_on = cp->prediction || inter ? 1 : 0;
    F.pred_root = job->image->color ? inter : (cp->prediction || inter ? 1 : 0);
    F.search_range = (int) cp->search_range;
    F.mv = (int16_t *) (base + L.mv);
    F.past = (const int16_t *) (base + L.past); F.future = (const int16_t *) (base + L.future);
    F.coop = (FcCoop *) (base + L.coop);
    F.mc_fwd = (float *) (base + L.mc_fwd); F.mc_bwd = inter ? (float *) (base + L.mc_bwd) : nullptr;
    F.pix_chroma = (int16_t *) (base + L.pix_chroma);
    F.frame_type = job->frame_type;
    F.p_min = (int) cp->p_min_level; F.p_max = (int) cp->p_max_level;
    F.d_rpf_mant = (int) cp->d_rpf.mantissa_bits; F.d_dc_mant = (int) cp->d_dc_rpf.mantissa_bits;
    F.d_rpf_range = cp->d_rpf.range; F.d_dc_range = cp->d_dc_rpf.range;
    F.d_dcs = 1 << (1 + F.d_dc_mant); F.d_sy = 1 << (1 + F.d_rpf_mant);
    F.d_coeff_size = (F.lc_max - F.lc_min + 1) * F.d_sy + F.d_dcs;
    F.ipis_alt = (float *) (base + L.ipis_alt); F.d5_alt = (float *) (base + L.d5_alt);
    F.d4_alt = (float *) (base + L.d4_alt); F.pix_save = (float *) (base + L.pix_save);
    F.sv_gram = (float *) (base + L.sv_gram); F.sv_img = (float *) (base + L.sv_img);
    F.sv_auto = (FcSavedRow *) (base + L.sv_auto);
    F.max_save = L.max_save;
    F.slab_base = base; F.slab_bytes = L.total;
}

/* the slab layout of one frame for capacity fs.P */
static void slot_layout(Staged *S, FrameSlot &fs)
{
    const fa_job *job = &S->jobs[fs.job];
    const fa_cparams *cp = &job->cp;
    int il = (int) cp->images_level;
    int low = cp->lc_min_level < cp->images_level;
    int NL = (int) (cp->lc_max_level - (low ? cp->lc_min_level : cp->images_level) + 1);
    int NS = (int) fa_size_of_tree(cp->products_level);
    int NA = 1 << (cp->lc_max_level - cp->images_level);
    int NI = (int) fa_size_of_tree(cp->images_level);
    size_t npix = (size_t) job->image->width * job->image->height;
    const int bands = job->image->color ? 3 : 1;
    /* states a prediction attempt can displace: the nodes of a subtree from the largest
     * predicted level down to the smallest block level */
    int max_save = 0;
    const int inter = job->frame_type;                 /* 0 I, 1 P, 2 B */
    if (cp->prediction || inter) {
        int span = (int) cp->p_max_level - (int) cp->lc_min_level + 1;
        max_save = 1 << (span < 1 ? 1 : span > 9 ? 9 : span);
    }
    fs.L = make_layout(fs.P, fs.PA, NL, NS, NA, NI, il, low, npix * bands, max_save, inter,
                       (int) cp->p_max_level - (int) cp->p_min_level + 1, job->image->color ? 1 : 0, fs.tri, fs.hm || fs.gm,
                       fs.gm ? (int) cp->limit_states : 0);
}

/* ---- frame queue: which frames may share slabs ---- */

static bool queue_eligible(const Staged *S, const FrameSlot &fs)
{
    const fa_job *job = &S->jobs[fs.job];
    /* inputs of P/B frames and the carried y_column of a colour stream live inside the slab */
    return job->frame_type == FA_I_FRAME && !job->ycol_carry && !fs.spec && !long_basis(job->wfa) && !fs.hm && !fs.gm && !fa_knob("FIASCO_AMD_NO_QUEUE");
}

/* same geometry, capacity and coder parameters as the queue's first frame: any of its slabs fits */
static bool queue_layout(const Staged *S, const FrameSlot &fs)
{
    if (S->lender0 < 0) return false;
    return fs.P == S->qP && fs.PA == S->qPA && fs.big == S->qbig && fs.tri == S->qtri
           && memcmp(&fs.L, &S->qL, sizeof(Layout)) == 0;
}

/* a frame without a slab: descriptor laid out for the slab of the queue's first frame (the
 * workgroup that takes it re-bases the pointers), pixel planes in the queue's pixel buffer */
static int stage_borrower(Staged *S, FrameSlot &fs, size_t frames_left)
{
    fa_job *job = &S->jobs[fs.job];
    const FrameSlot &ref = S->slots[S->lender0];
    const size_t npix = (size_t) job->image->width * job->image->height;
    const int bands = job->image->color ? 3 : 1;
    const size_t need = align_up(npix * bands * 2, 256);
    if (!S->qpix && !fs.ext_pix) {
        size_t bytes = need * frames_left;
        if (hipMalloc((void **) &S->qpix, bytes) != hipSuccess) { S->qpix = nullptr; (void) hipGetLastError(); return 0; }
        S->qpix_bytes = bytes; S->qpix_used = 0;
    }
    if (!fs.ext_pix && S->qpix_used + need > S->qpix_bytes) return 0;
    fs.base = ref.base;                       /* the layout reference, not an owned slab */
    fill_frame(fs, job);
    fs.base = nullptr; fs.bytes = 0;
    fs.borrow = true;
    if (fs.ext_pix) {                         /* converted from device memory: the planes are where they stay */
        fs.F.pix16 = fs.ext_pix;
        S->borrowers++;
        fs.staged = true;
        return 1;
    }
    fs.ext_pix = (const int16_t *) (S->qpix + S->qpix_used);
    fs.F.pix16 = fs.ext_pix;
    for (int b = 0; b < bands; b++)
        if (hipMemcpyAsync(S->qpix + S->qpix_used + (size_t) b * npix * 2, slot_image(S, fs)->pixels[b], npix * 2,
                           hipMemcpyHostToDevice, S->stream) != hipSuccess) {
            snprintf(job->errmsg, sizeof job->errmsg, "HIP error: pixel upload failed");
            fs.borrow = false; fs.ext_pix = nullptr;
            return 0;
        }
    S->qpix_used += need;
    S->borrowers++;
    fs.staged = true;
    return 1;
}

/* the planes of a reference frame into the slab at `off': from the copy the device decoder left on this device
 * (fa_image.dev, frame_decoder.inc), else from the host planes */
static bool upload_reference(Staged *S, const FrameSlot &fs, const fa_image *ref, size_t off, int here)
{
    const fa_job *job = &S->jobs[fs.job];
    const size_t npix = (size_t) job->image->width * job->image->height;
    const int bands = job->image->color ? 3 : 1;
    for (int b = 0; b < bands; b++)
        if ((ref->dev && ref->dev_id == here
             ? hipMemcpyAsync(fs.base + off + (size_t) b * npix * 2, (const int16_t *) ref->dev + (size_t) b * npix, npix * 2,
                              hipMemcpyDeviceToDevice, S->stream)
             : hipMemcpyAsync(fs.base + off + (size_t) b * npix * 2, ref->pixels[b], npix * 2,
                              hipMemcpyHostToDevice, S->stream)) != hipSuccess)
            return false;
    return true;
}

/* allocate the slab of one frame for capacity fs.P and upload its inputs */
static int stage_slot(Staged *S, FrameSlot &fs)
{
    fa_job *job = &S->jobs[fs.job];
    const fa_cparams *cp = &job->cp;
    const size_t npix = (size_t) job->image->width * job->image->height;
    const int bands = job->image->color ? 3 : 1;
    slot_layout(S, fs);
    fs.base = slab_acquire(fs.L.total, &fs.bytes, &fs.slab_dev);
    /* developer aid: FIASCO_AMD_POISON=<byte> fills the slab first -- the kernel must write every
     * cell before it reads it, whatever an earlier frame left there */
    if (fs.base && fa_knob("FIASCO_AMD_POISON"))
        (void) hipMemsetAsync(fs.base, (int) knob_int("FIASCO_AMD_POISON", 0), fs.L.total, S->stream);
    if (!fs.base) {
        snprintf(job->errmsg, sizeof job->errmsg, "out of HBM: frame needs %.2f GiB", fs.L.total / 1073741824.0);
        return 0;
    }
    auto give_up = [&](const char *msg) {
        snprintf(job->errmsg, sizeof job->errmsg, "%s", msg);
        slab_release(fs.base, fs.bytes, fs.slab_dev); fs.base = nullptr;
        return 0;
    };
    fill_frame(fs, job);
    const bool hmx = fs.hm || fs.gm;              /* the FC_GM build has the FC_HM build's model sizes */
    const int maxsym = hmx ? FC_MAXSYM_HM : FC_MAXSYM_STD;
    if (fs.F.coeff_size > (hmx ? FC_MAXCOEFF_HM : fs.big ? FC_MAXCOEFF_BIG_STD : FC_MAXCOEFF) || fs.F.dcs > maxsym || fs.F.sy > maxsym
        || (fs.F.pred_on && (fs.F.d_coeff_size > (hmx ? FC_MAXCOEFF_HM : FC_MAXCOEFF_BIG_STD) || fs.F.d_dcs > maxsym || fs.F.d_sy > maxsym))
        || fs.F.ML > 26) {
        snprintf(job->errmsg, sizeof job->errmsg,
                 "coefficient model too large for the device coder (levels x mantissa symbols > %d)", hmx ? FC_MAXCOEFF_HM : FC_MAXCOEFF_BIG_STD);
        slab_release(fs.base, fs.bytes, fs.slab_dev); fs.base = nullptr;
        fs.done = true; fs.rejected = true;      /* permanent: not a matter of free HBM */
        return 0;
    }
    if (fs.ext_pix) fs.F.pix16 = fs.ext_pix;       /* the planes live outside the slab already */
    for (int b = 0; b < bands && !fs.ext_pix; b++)
        if (hipMemcpyAsync(fs.base + fs.L.pix16 + (size_t) b * npix * 2, slot_image(S, fs)->pixels[b], npix * 2,
                           hipMemcpyHostToDevice, S->stream) != hipSuccess)
            return give_up("HIP error: pixel upload failed");
    int here = -1;
    if (hipGetDevice(&here) != hipSuccess) { (void) hipGetLastError(); here = -1; }
    if ((job->frame_type != FA_I_FRAME && job->past && !upload_reference(S, fs, job->past, fs.L.past, here))
        || (job->frame_type == FA_B_FRAME && job->future && !upload_reference(S, fs, job->future, fs.L.future, here)))
        return give_up("HIP error: reference frame upload failed");
    if (job->ycol_carry) {                 /* [cap][2] on the host, [2][PA] on the device */
        const fa_wfa *w = job->wfa;
        fs.ycol_host.assign((size_t) 2 * fs.PA, 0);
        for (unsigned s = 0; s < w->cap && s < (unsigned) fs.PA; s++)
            for (int l = 0; l < 2; l++) fs.ycol_host[(size_t) l * fs.PA + s] = w->y_column[s * 2 + l];
        if (hipMemcpyAsync(fs.base + fs.L.ycol0, fs.ycol_host.data(), fs.ycol_host.size(),
                           hipMemcpyHostToDevice, S->stream) != hipSuccess)
            return give_up("HIP error: y_column upload failed");
    }
    if (fs.F.lginv) {                      /* log2 (1.0 / n) as THIS host's libm gives it: uniform_bits, codec/domain-pool.c:592-615 */
        const unsigned nmax = cp->limit_states + 1;
        fs.lginv_host.assign(nmax + 1, 0.0);
        for (unsigned k = 1; k <= nmax; k++) fs.lginv_host[k] = log2(1.0 / k);
        if (hipMemcpyAsync(fs.base + fs.L.lginv, fs.lginv_host.data(), fs.lginv_host.size() * 8, hipMemcpyHostToDevice, S->stream) != hipSuccess)
            return give_up("HIP error: table upload failed");
    }
    if (fs.F.bx) {                         /* the rows of a long basis, as they lie in the host's memory (DevFrame.bx) */
        const fa_wfa *w = job->wfa;
        const unsigned nb = w->basis_states, nr = 12 * nb + 12;
        fs.bx_host.assign((bx_bytes(w) + 3) / 4, 0);
        int32_t *b = fs.bx_host.data();
        b[0] = (int32_t) nb; b[1] = (int32_t) nr;
        memcpy(b + 4, w->final_distribution, (size_t) nb * 4);
        for (unsigned s = 0; s < nb; s++) b[4 + nb + s] = w->domain_type[s];
        float *bw = (float *) (b + 4 + 2 * nb);
        int16_t *bi = (int16_t *) (b + 4 + 2 * nb + nr);
        for (unsigned k = 0; k < nr; k++) { bi[k] = k < 12 * nb ? w->into[k] : (int16_t) FA_NO_EDGE; bw[k] = k < 12 * nb ? w->weight[k] : 0.0f; }
        if (hipMemcpyAsync(fs.base + fs.L.bx, b, fs.bx_host.size() * 4, hipMemcpyHostToDevice, S->stream) != hipSuccess)
            return give_up("HIP error: basis upload failed");
    }
    fs.staged = true;
    return 1;
}

static void core1_unstage(void *h)
{
    Staged *S = (Staged *) h;
    if (!S) return;
    if (S->inflight) {                       /* a submitted launch nobody collected */
        (void) hipStreamSynchronize(S->stream);
        if (S->d_trace) (void) hipFree(S->d_trace);
    }
    for (size_t k = 0; k < S->slots.size(); k++)
        if (S->slots[k].base) slab_release(S->slots[k].base, S->slots[k].bytes, S->slots[k].slab_dev);
    for (void *p : std::initializer_list<void *>{ S->d_frames, S->qpix, S->d_ring, S->d_queue, S->d_ptrmask, S->d_vframes, S->d_spec })
        if (p) (void) hipFree(p);
    if (S->cstream) { (void) hipStreamSynchronize(S->cstream); (void) hipStreamDestroy(S->cstream); }
    for (int i = 0; i < 2; i++) if (S->d_pack[i]) (void) hipFree(S->d_pack[i]);
    if (S->pinned) (void) hipHostFree(S->pinned);
    if (S->ustream) { (void) hipStreamSynchronize(S->ustream); (void) hipStreamDestroy(S->ustream); }
    if (S->ev_up) (void) hipEventDestroy(S->ev_up);
    if (S->ev_ic) (void) hipEventDestroy(S->ev_ic);
    if (S->ic_tab) (void) hipHostFree(S->ic_tab);
    if (S->d_ic) (void) hipFree(S->d_ic);
    if (S->peer_buf) (void) hipFree(S->peer_buf);
    if (S->up_host && !S->up_host_shared) (void) hipHostFree(S->up_host);
    for (int i = 0; i < 2; i++) if (S->up_dev[i]) (void) hipFree(S->up_dev[i]);
    if (S->ev0) (void) hipEventDestroy(S->ev0);
    if (S->ev1) (void) hipEventDestroy(S->ev1);
    if (S->stream) (void) hipStreamDestroy(S->stream);
    delete S;
}

/* the slot of job i: its kernel build's geometry and the first guess of its state capacity */
static FrameSlot first_guess(const Staged *S, unsigned i)
{
    const fa_job *job = &S->jobs[i];
    const fa_cparams *cp = &job->cp;
    /* one state per bintree node above the largest block level (2 x #blocks) ... measured need at -q 20 is
     * ~1.3 x #blocks */
    const size_t blocks = top_blocks(job);
    size_t guess = blocks + blocks * 3 / 8 + 64;
    /* predicted frames: the residual of a predicted block subdivides where the block itself would not --
     * 720p colour P frames with --prediction end with 2.0 .. 2.3 table states per block (config 5) */
    if (job->frame_type != FA_I_FRAME) guess = blocks * 5 / 2 + 64;
    /* tests / experiments: FIASCO_AMD_CAP_GUESS=<states> forces the first guess (a frame that
     * outgrows it is encoded again with 1.5 x the capacity, frame_outcome) */
    const long long forced = knob_int("FIASCO_AMD_CAP_GUESS", 0);
    if (forced > 0) guess = (size_t) forced;
    /* what frames of this kind needed before (cap_hint_put): 1/16 on top, frames of a sequence drift */
    int hintP = 0, hintPA = 0;
    if (forced <= 0 && !fa_knob("FIASCO_AMD_NO_CAP_HINT")) cap_hint_get(job, &hintP, &hintPA);
    if ((size_t) hintP + hintP / 16 + 32 > guess) guess = (size_t) hintP + hintP / 16 + 32;
    if (guess > cp->limit_states) guess = cp->limit_states;
    FrameSlot fs;
    fs.job = (int) i;
    fs.P = (int) align_up(guess, 64);
    fs.big = needs_big_variant(cp, job->wfa) || job->frame_type != FA_I_FRAME
             /* a chroma dictionary of more than 63 states: the list scan of the big builds (mp_steps_list_global) */
             || (job->image->color && cp->chroma_max_states > 63);
    fs.hm = needs_hm_variant(cp);
    fs.gm = needs_gm_variant(job) || fa_knob("FIASCO_AMD_FORCE_GM") != nullptr;     /* (tests: every frame through the FC_GM build) */
    if (fs.gm) fs.big = true;
    fs.wide_only = !fs.big && needs_wide_variant(cp);
    if (S->specG && !fs.big) {
        /* the 256-thread build up to 3072 states, the 1024-thread one (4K; frames beyond the narrow
         * build's LDS pools) up to 12288 */
        const size_t withids = align_up(guess + (size_t) (S->specG - 1 - spec_workers(S->specG)) * FC_SPEC_TEMPS, 64);
        if (withids <= 12 * 1024 && withids <= align_up(cp->limit_states, 64)) { fs.spec = true; fs.P = (int) withids; }
    }
    /* tests: the triangular layout (chosen by fit_hbm for HBM-bound batches) for every default-geometry frame */
    if (!fs.big && fa_knob("FIASCO_AMD_FORCE_TRI")) fs.tri = true;
    /* colour: the two chroma bands add auxiliary states (no tables) */
    const size_t cap = align_up(cp->limit_states, 64);
    fs.PA = job->image->color ? (int) (3 * (size_t) fs.P > cap ? cap : 3 * (size_t) fs.P) : fs.P;
    if ((size_t) hintPA + hintPA / 16 + 32 > (size_t) fs.PA) {
        const size_t want = align_up((size_t) hintPA + hintPA / 16 + 32, 64);
        fs.PA = (int) (want > cap ? cap : want);
    }
    if (fs.PA < fs.P) fs.PA = fs.P;
    if (hintP) { fs.floorP = hintP + hintP / 16 + 32; fs.floorPA = hintPA + hintPA / 16 + 32; }
    return fs;
}

/* HBM-bound batches (4K: a slab is 3 GB, 97 % of it the Gram tables, quadratic in the state capacity): when the
 * slabs the chip could keep busy do not fit, the frames take the triangular Gram tables, then the capacity guess
 * drops from 1.375 to 1.15 states per block of the largest block level -- a third more frames in flight; a frame
 * that outgrows it is encoded again with 1.5 x the capacity (frame_outcome).  A batch that will queue for slabs
 * gets the pixel buffer of the queue's frames first. */
static void fit_hbm(Staged *S)
{
    FrameSlot probe = S->slots[0];
    slot_layout(S, probe);
    size_t free_b = 0, total_b = 0;
    const size_t pooled = pool_bytes();
    size_t want = S->slots.size();
    const size_t resident = (size_t) S->ncu * frames_per_cu(probe);
    if (want > resident) want = resident;
    const bool hbm_bound = hipMemGetInfo(&free_b, &total_b) == hipSuccess && probe.L.total * want > free_b + pooled;
    if ((hbm_bound || S->slots.size() > resident) && queue_eligible(S, probe) && !probe.ext_pix) {
        /* the pixel planes of the frames that will queue for a slab: set aside before the slabs
         * take what HBM has (when HBM is the limit nobody knows yet how many slabs will fit) */
        const fa_image *im = S->jobs[probe.job].image;
        const size_t need = align_up((size_t) im->width * im->height * (im->color ? 3 : 1) * 2, 256);
        const size_t frames = hbm_bound ? S->slots.size() : S->slots.size() - resident;
        if (hipMalloc((void **) &S->qpix, need * frames) == hipSuccess) { S->qpix_bytes = need * frames; S->qpix_used = 0; }
        else { S->qpix = nullptr; (void) hipGetLastError(); }
    }
    if (!hbm_bound) return;
    /* first remedy: the triangular Gram tables -- half the slab; the kernel build that reads them exists for the
     * default geometry at the wide workgroup (frames with more than 3072 states: 4K), where memory is what keeps
     * CUs idle */
    for (size_t k = 0; k < S->slots.size(); k++) {
        FrameSlot &fs = S->slots[k];
        if (!fs.big && fs.P > 12 * 256) fs.tri = true;
    }
    FrameSlot probe2 = S->slots[0];
    slot_layout(S, probe2);
    if (probe2.L.total * want <= free_b + pooled) return;
    /* then the tight capacity */
    for (size_t k = 0; k < S->slots.size(); k++) {
        FrameSlot &fs = S->slots[k];
        const fa_job *job = &S->jobs[fs.job];
        const fa_cparams *cp = &job->cp;
        const size_t blocks = top_blocks(job);
        size_t tight = align_up(blocks + blocks * 3 / 20 + 64, 64);
        if ((size_t) fs.floorP > tight) tight = align_up((size_t) fs.floorP, 64);   /* never below a known need */
        if (tight > cp->limit_states) tight = align_up(cp->limit_states, 64);
        if ((size_t) fs.P <= tight || fs.spec) continue;
        const size_t cap = align_up(cp->limit_states, 64);
        fs.P = (int) tight;
        fs.PA = job->image->color ? (int) (3 * tight > cap ? cap : 3 * tight) : fs.P;
        if ((size_t) fs.floorPA > (size_t) fs.PA) fs.PA = (int) (align_up((size_t) fs.floorPA, 64) > cap ? cap : align_up((size_t) fs.floorPA, 64));
        if (fs.PA < fs.P) fs.PA = fs.P;
    }
}

/* Stage the frames.  Every frame gets a slab of its own until the device is full -- as many frames of one layout
 * as the chip runs workgroups at once, or as HBM holds; the frames after that join the FRAME QUEUE of that layout
 * (no slab: whichever workgroup finishes its frame takes the next one into its slab).  What can neither have a
 * slab nor join the queue is staged by core1_finish2() as slabs free up. */
static void stage_frames(Staged *S)
{
    for (size_t k = 0; k < S->slots.size(); k++) {
        FrameSlot &fs = S->slots[k];
        const bool elig = queue_eligible(S, fs);
        slot_layout(S, fs);
        if (elig && queue_layout(S, fs) && S->lenders >= S->lender_cap
            && stage_borrower(S, fs, S->slots.size() - k))
            continue;
        if (stage_slot(S, fs)) {
            if (elig && S->lender0 < 0) {
                S->lender0 = (int) k; S->lenders = 1;
                S->qL = fs.L; S->qP = fs.P; S->qPA = fs.PA; S->qbig = fs.big; S->qtri = fs.tri;
                /* workgroups the chip holds at once: fc_config.inc FC_WG_PER_CU of the build the
                 * launch will use (wide build for P > 3072: one per CU) */
                S->lender_cap = (size_t) S->ncu * frames_per_cu(fs);
                const long long slabs = knob_int("FIASCO_AMD_QUEUE_SLABS", 0);     /* tests: a short queue on small batches */
                if (slabs > 0) S->lender_cap = (size_t) slabs;
            } else if (elig && queue_layout(S, fs)) S->lenders++;
            continue;
        }
        if (fs.rejected) continue;         /* outside the device scope: message recorded */
        if (elig && queue_layout(S, fs) && S->lenders >= 1) {     /* HBM is full: queue */
            S->jobs[fs.job].errmsg[0] = 0;
            if (stage_borrower(S, fs, S->slots.size() - k)) { S->lender_cap = S->lenders; continue; }
        }
        if (k == 0) continue;              /* does not fit even alone: error already recorded */
        S->jobs[fs.job].errmsg[0] = 0;     /* later wave */
        break;
    }
}

/* frames != NULL: frames->at(i) is the 8-bit picture of jobs[i] in device memory (jobs[i].image has no host planes), ready
 * once `ready' has happened */
static void *core1_stage(unsigned n, fa_job *jobs, const IcInput *frames = nullptr, hipEvent_t ready = nullptr)
{
    Staged *S = new Staged;
    int ndev = 0;
    S->n = n; S->jobs = jobs;
    for (unsigned i = 0; i < n; i++) { jobs[i].status = 0; jobs[i].errmsg[0] = 0; }
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        for (unsigned i = 0; i < n; i++)
            snprintf(jobs[i].errmsg, sizeof jobs[i].errmsg,
                     "libfiasco_amd: no HIP device available (the hot path has no CPU fallback)");
        return S;
    }
    char l2_why[200];
    if (!log2_patch_build(l2_why, sizeof l2_why)) {      /* built once per share and device, whoever comes first */
        /* frames coded without it could differ from the reference's: fail them, loudly */
        for (unsigned i = 0; i < n; i++)
            snprintf(jobs[i].errmsg, sizeof jobs[i].errmsg,
                     "libfiasco_amd: no log2 correction table, streams could differ from the reference's "
                     "(FIASCO_AMD_NO_LOG2_TABLE=1 encodes without it): %s", l2_why);
        return S;                             /* S->ok stays false: nothing of this batch runs */
    }
    {
        int dev = 0, ncu = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) ncu = 256;
        /* every frame for the 256-thread build of the speculating kernel?  (several of its workgroups fit a CU) */
        bool narrow_only = n > 0;
        for (unsigned i = 0; i < n && narrow_only; i++) {
            if (!jobs[i].image) { narrow_only = false; break; }
            const size_t blocks = top_blocks(&jobs[i]);
            if (needs_wide_variant(&jobs[i].cp) || blocks + blocks * 3 / 8 + 64 + FC_SPEC_MAXG * FC_SPEC_TEMPS > 3072) narrow_only = false;
        }
        S->specG = spec_groups(n, ncu, n > 0 && jobs[0].image && (jobs[0].image->width > 2048 || jobs[0].image->height > 2048), narrow_only);
        S->ncu = ncu;
    }
    if (hipStreamCreate(&S->stream) != hipSuccess || hipEventCreate(&S->ev0) != hipSuccess
        || hipEventCreate(&S->ev1) != hipSuccess
        || hipMalloc((void **) &S->d_frames, sizeof(DevFrame) * (n ? n : 1)) != hipSuccess) {
        for (unsigned i = 0; i < n; i++)
            snprintf(jobs[i].errmsg, sizeof jobs[i].errmsg, "HIP error: cannot create stream/events");
        return S;
    }
    for (unsigned i = 0; i < n; i++)
        if (device_supported(&jobs[i], jobs[i].errmsg, sizeof jobs[i].errmsg)) S->slots.push_back(first_guess(S, i));
    if (!frames) {
        /* frames of a video that was opened from device memory (input_convert.inc, fiasco_amd_seq_open_device): the
         * planes are read where open left them when that is this device; a frame on another device -- the device list
         * changed after open -- goes through its host planes */
        int here = -1;
        if (hipGetDevice(&here) != hipSuccess) { (void) hipGetLastError(); here = -1; }
        std::vector<FrameSlot> keep;
        for (FrameSlot &fs : S->slots) {
            const fa_image *im = jobs[fs.job].image;
            if (im->src_dev && !im->pixels[0]) {
                if (im->src_dev_id == here) fs.ext_pix = im->src_dev;
                else if (!fa_image_host_planes(im)) {
                    snprintf(jobs[fs.job].errmsg, sizeof jobs[fs.job].errmsg, "%s", fiasco_get_error_message());
                    continue;
                }
            }
            keep.push_back(fs);
        }
        S->slots.swap(keep);
    }
    if (frames && !S->slots.empty()) {
        /* the planes never pass through the host: converted into the buffer the first pass reads, before any slot is
         * staged (a slot with ext_pix uploads no pixels) */
        if (!ic_convert(S, *frames, S->up_parity, ready, false, false) || hipStreamWaitEvent(S->stream, S->ev_up, 0) != hipSuccess) {
            snprintf(S->ic_failed, sizeof S->ic_failed, "%s", fiasco_get_error_message());
            if (!S->ic_failed[0]) snprintf(S->ic_failed, sizeof S->ic_failed, "HIP error: the frames in device memory could not be converted");
            for (unsigned i = 0; i < n; i++)
                if (!jobs[i].errmsg[0]) snprintf(jobs[i].errmsg, sizeof jobs[i].errmsg, "%s", fiasco_get_error_message());
            S->slots.clear();
        }
    }
    if (!S->slots.empty()) fit_hbm(S);
    stage_frames(S);
    (void) hipStreamSynchronize(S->stream);
    S->ok = true;
    return S;
}

/* ---- replacement inputs for a staged batch (a stream of batches) ---- */

static int16_t *core1_upload_buffer(void *h, size_t bytes)
{
    Staged *S = (Staged *) h;
    if (!S || !S->ok || !bytes) return nullptr;
    /* the previous upload has left this memory long ago (a whole pass lies in between) */
    if (S->ustream) (void) hipStreamSynchronize(S->ustream);
    if (S->up_host_shared) { S->up_host = nullptr; S->up_host_bytes = 0; S->up_host_shared = false; }   /* not ours to free */
    return grow_buffer(S->up_host, S->up_host_bytes, bytes, true) ? (int16_t *) S->up_host : nullptr;
}

static int core1_upload_commit(void *h)
{
    Staged *S = (Staged *) h;
    if (!S || !S->ok || !S->up_host) return 0;
    if (!S->ustream && hipStreamCreateWithFlags(&S->ustream, hipStreamNonBlocking) != hipSuccess) {
        S->ustream = nullptr; (void) hipGetLastError(); return 0;
    }
    if (!S->ev_up && hipEventCreateWithFlags(&S->ev_up, hipEventDisableTiming) != hipSuccess) {
        S->ev_up = nullptr; (void) hipGetLastError(); return 0;
    }
    /* the buffer the RUNNING pass does not read; it holds the planes of THIS share's frames back to back (with
     * several shares the frames of a share are every D-th of the caller's buffer): one copy per frame */
    const int p = S->up_parity ^ 1;
    size_t need = 0;
    for (size_t k = 0; k < S->slots.size(); k++) {
        const fa_image *im = S->jobs[S->slots[k].job].image;
        const size_t npix = (size_t) im->width * im->height * (im->color ? 3 : 1);
        const size_t o = (size_t) ((const char *) im->pixels[0] - S->up_host);
        if ((const char *) im->pixels[0] < S->up_host || o + npix * 2 > S->up_host_bytes) {
            fa_set_error("upload: frame planes lie outside the upload buffer");
            return 0;
        }
        need += align_up(npix * 2, 256);
    }
    if (!need) return 1;                         /* nothing the device can encode */
    if (!grow_buffer(S->up_dev[p], S->up_dev_bytes[p], need)) {
        fa_set_error("out of HBM: no room for %.1f MiB of replacement frames", need / 1048576.0);
        return 0;
    }
    {
        size_t at = 0;
        bool fail = false;
        for (size_t k = 0; k < S->slots.size() && !fail; k++) {
            const fa_image *im = S->jobs[S->slots[k].job].image;
            const size_t len = (size_t) im->width * im->height * (im->color ? 3 : 1) * 2;
            fail = hipMemcpyAsync(S->up_dev[p] + at, im->pixels[0], len, hipMemcpyHostToDevice, S->ustream) != hipSuccess;
            /* taken over by the next submit: a re-encode of the RUNNING pass (capacity guess too
             * small) still reads that pass's frames */
            S->slots[k].ext_next = (const int16_t *) (S->up_dev[p] + at);
            at += align_up(len, 256);
        }
        if (fail || hipEventRecord(S->ev_up, S->ustream) != hipSuccess) {
            fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
            return 0;
        }
    }
    S->up_pending = true;
    return 1;
}
