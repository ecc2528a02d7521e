/*
 *  enc_launch.inc -- a pass over a staged batch (included by core_hip.cpp): the wave of launches (order_batch ..
 *  start_launches), its download and what became of every frame (download_wave, fetch_automata, frame_outcome,
 *  collect), and the two entries of a share, core1_submit and core1_finish2.
 */

/* copy the finished automaton of one frame back into the job's fa_wfa */
static int collect(Staged *S, FrameSlot &fs, const char *pinned)
{
    fa_job *job = &S->jobs[fs.job];
    const DevFrame &F = fs.F;
    const Layout &L = fs.L;
    const int P = fs.PA;                 /* pitch of the automaton arrays */
    fa_wfa *w = job->wfa;
    unsigned ns = (unsigned) F.states;
    size_t span = L.pool_states - L.tree;
    std::vector<char> own;
    if (!pinned) {                       /* no staging buffer: plain synchronous copy */
        own.resize(span);
        if (hipMemcpy(own.data(), fs.base + L.tree, span, hipMemcpyDeviceToHost) != hipSuccess) {
            snprintf(job->errmsg, sizeof job->errmsg, "HIP error: automaton download failed");
            return 0;
        }
        pinned = own.data();
    }
    const char *const host = pinned;
    const int16_t *tree = (const int16_t *) host;
    const int16_t *into = (const int16_t *) (host + (L.into - L.tree));
    const float *weight = (const float *) (host + (L.weight - L.tree));
    const float *fin = (const float *) (host + (L.final_d - L.tree));
    const uint8_t *los = (const uint8_t *) (host + (L.level_of_state - L.tree));
    const uint8_t *dt = (const uint8_t *) (host + (L.domain_type - L.tree));
    const uint16_t *xs = (const uint16_t *) (host + (L.x - L.tree));
    const uint16_t *ys = (const uint16_t *) (host + (L.y - L.tree));
    const uint8_t *ycol = (const uint8_t *) (host + (L.ycol - L.tree));
    const int16_t *mv = (const int16_t *) (host + (L.mv - L.tree));
    const bool inter = job->frame_type != FA_I_FRAME;
    for (unsigned s = 0; s < w->basis_states; s++) w->level_of_state[s] = 0xff;   /* codec/control.c:133-173 */
    fa_wfa_remove_states(w, w->basis_states);
    for (unsigned s = w->basis_states; s < ns; s++) {
        w->final_distribution[s] = fin[s];
        w->domain_type[s] = dt[s];
        w->level_of_state[s] = los[s];
        w->delta_state[s] = 0;
        for (int l = 0; l < 2; l++) {
            FA_TREE(w, s, l) = tree[(size_t) l * P + s];
            w->x[s * 2 + l] = xs[(size_t) l * P + s];
            w->y[s * 2 + l] = ys[(size_t) l * P + s];
            w->y_state[s * 2 + l] = FA_RANGE;
            w->y_column[s * 2 + l] = F.color ? ycol[(size_t) l * P + s] : 0;
            w->prediction[s * 2 + l] = 0;
            if (inter) {
                fa_mv *m = &w->mv[s * 2 + l];
                m->type = mv[(size_t) (0 * 2 + l) * P + s]; m->fx = mv[(size_t) (1 * 2 + l) * P + s];
                m->fy = mv[(size_t) (2 * 2 + l) * P + s]; m->bx = mv[(size_t) (3 * 2 + l) * P + s];
                m->by = mv[(size_t) (4 * 2 + l) * P + s];
            }
            for (int e = 0; e < 6; e++) {
                FA_INTO(w, s, l, e) = into[(size_t) (l * 6 + e) * P + s];
                FA_WEIGHT(w, s, l, e) = weight[(size_t) (l * 6 + e) * P + s];
                if (FA_INTO(w, s, l, e) == FA_NO_EDGE) break;
            }
        }
    }
    if (F.color)                         /* the flags of EVERY state id: the next frame of a stream
                                          * starts from them (fa_job.ycol_carry) */
        for (unsigned s = 0; s < w->cap && s < (unsigned) P; s++)
            for (int l = 0; l < 2; l++) w->y_column[s * 2 + l] = ycol[(size_t) l * P + s];
    w->states = ns;
    w->root_state = (unsigned) F.root_state;
    job->stats[0].costs = F.costs; job->stats[0].err = F.err;
    job->stats[0].tree_bits = F.tree_bits; job->stats[0].matrix_bits = F.matrix_bits;
    job->stats[0].weights_bits = F.weights_bits;
    if (F.color) {
        for (int b = 0; b < 2; b++) {
            job->stats[b + 1].costs = F.c_costs[b]; job->stats[b + 1].err = F.c_err[b];
            job->stats[b + 1].tree_bits = F.c_tree_bits[b];
            job->stats[b + 1].matrix_bits = F.c_matrix_bits[b];
            job->stats[b + 1].weights_bits = F.c_weights_bits[b];
        }
        /* co-located luminance states (codec/subdivide.c:167-173,560-567): a pure function of
         * the finished trees -- walk each chroma tree next to the luminance tree.  The root is
         * {{Y, Cb}, {Cr, -}} (codec/coder.c:803-833). */
        int ycb = FA_TREE(w, ns - 1, 0), crs = FA_TREE(w, ns - 1, 1);
        int roots[2] = { FA_TREE(w, ycb, 1), FA_TREE(w, crs, 0) };
        int yroot = FA_TREE(w, ycb, 0);
        std::vector<std::pair<int, int>> stack;
        for (int b = 0; b < 2; b++) {
            stack.push_back(std::make_pair(roots[b], yroot));
            while (!stack.empty()) {
                std::pair<int, int> t = stack.back();
                stack.pop_back();
                int s = t.first, y = t.second;
                if (s == FA_RANGE || (unsigned) s < w->basis_states) continue;
                for (int l = 0; l < 2; l++) {
                    int ny = y != FA_RANGE ? FA_TREE(w, y, l) : FA_RANGE;
                    w->y_state[s * 2 + l] = (int16_t) ny;
                    stack.push_back(std::make_pair((int) FA_TREE(w, s, l), ny));
                }
            }
        }
    }
    job->lc_min_level_out = (unsigned) F.lc_min_out;
    job->status = 1;
    stats_update([&](fiasco_amd_stats &st) {
        st.frames += 1;
        st.bytes_mp += F.bytes_mp; st.bytes_img += F.bytes_img; st.bytes_gram += F.bytes_gram;
        st.n_mp += F.n_mp; st.n_steps += F.n_steps; st.n_blocks += F.n_blocks;
        st.n_appends += F.n_appends; st.n_fulleval += F.n_fulleval;
        st.t_init += F.t_init; st.t_approx += F.t_approx; st.t_ipis += F.t_ipis;
        st.t_append += F.t_append; st.t_serial += F.t_serial; st.t_total += F.t_total;
        st.t_mpA += F.t_mpA; st.t_mpB += F.t_mpB; st.n_blockevals += F.n_blockevals;
        for (int k = 0; k < 8; k++) st.dbg[k] += F.dbg[k];
        st.states_sum += ns;
        if (ns > st.states_max) st.states_max = ns;
    });
    cap_hint_put(job, F.ystates_out, F.states);
    if (fa_knob("FIASCO_AMD_CAP_TRACE"))
        fprintf(stderr, "capacity: frame type %d used %d table states of %d, %d states of %d; %.3f s on the device\n", job->frame_type,
                F.ystates_out, fs.P, F.states, fs.PA, (double) F.t_total / 1e8);
    return 1;
}

/* device-side state of the frame queue: the ring of free slabs, the counters, and the map
 * of the descriptor's slab pointers (one bit per 8-byte word): the words that move with the base
 * when the same frame is laid out for two different slabs, plus pack_src */
static bool queue_resources(Staged *S, size_t frames)
{
    /* a ring per build that can hold a queue (B_DEFAULT .. B_WIDE_TRI), indexed by the build */
    if (!grow_buffer(S->d_ring, S->ring_n, 5 * frames)) return false;
    if (!S->d_queue && hipMalloc((void **) &S->d_queue, 2 * 5 * sizeof(unsigned)) != hipSuccess) {
        S->d_queue = nullptr; (void) hipGetLastError(); return false;
    }
    if (!S->ptrmask_ready) {
        const size_t words = FC_DESC_WORDS, mwords = (words + 31) / 32;
        std::vector<unsigned> mask(mwords, 0u);
        FrameSlot a = S->slots[S->lender0], b = S->slots[S->lender0];
        const fa_job *job = &S->jobs[a.job];
        b.base = a.base + (1u << 24);
        fill_frame(a, job); fill_frame(b, job);
        const unsigned long long *wa = (const unsigned long long *) &a.F, *wb = (const unsigned long long *) &b.F;
        for (size_t w = 0; w < sizeof(DevFrame) / 8; w++)
            if (wa[w] != wb[w]) mask[w >> 5] |= 1u << (w & 31);
        const size_t wp = offsetof(DevFrame, pack_src) / 8;
        mask[wp >> 5] |= 1u << (wp & 31);
        if (!S->d_ptrmask && hipMalloc((void **) &S->d_ptrmask, mwords * sizeof(unsigned)) != hipSuccess) {
            S->d_ptrmask = nullptr; (void) hipGetLastError(); return false;
        }
        if (hipMemcpy(S->d_ptrmask, mask.data(), mwords * sizeof(unsigned), hipMemcpyHostToDevice) != hipSuccess) return false;
        S->ptrmask_ready = true;
    }
    return true;
}

/* frames of a launch per kernel build: all, the frame queue's lenders (with a slab) and its borrowers */
struct WaveGroups { size_t n[N_BUILDS], lend[N_BUILDS], borrow[N_BUILDS]; };

/* the launch's frames (S->batch), ordered by build, then the queue's lenders, then its borrowers, then the rest,
 * each part in slot order; counts them per build.  False when nothing is left to launch. */
static bool order_batch(Staged *S, WaveGroups &g)
{
    std::vector<size_t> &batch = S->batch;
    batch.clear();
    for (size_t k = 0; k < S->slots.size(); k++)
        if (S->slots[k].staged && !S->slots[k].done) batch.push_back(k);
    if (batch.empty()) return false;
    memset(&g, 0, sizeof g);
    const bool few = batch.size() <= (size_t) S->ncu && !fa_knob("FIASCO_AMD_NO_WIDE");
    std::vector<int> key(S->slots.size());
    for (size_t k : batch) {
        const FrameSlot &fs = S->slots[k];
        const Build b = build_of(S, fs, few);
        const int part = fs.borrow ? 1 : S->borrowers && queue_eligible(S, fs) && queue_layout(S, fs) ? 0 : 2;
        key[k] = 3 * b + part;
        g.n[b]++;
        if (part == 0) g.lend[b]++; else if (part == 1) g.borrow[b]++;
    }
    stats_update([&](fiasco_amd_stats &st) {
        for (int b = 0; b < N_BUILDS; b++)
            if (k_build[b].stats_slot >= 0) st.frames_by_build[k_build[b].stats_slot] += g.n[b]; else st.spec_frames += g.n[b];
    });
    std::stable_sort(batch.begin(), batch.end(), [&](size_t a, size_t b) { return key[a] < key[b]; });
    return true;
}

/* the launch's descriptors (S->hf) and where every frame packs its finished automaton: one buffer per launch,
 * double buffered -- launch i + 1 writes the other one while the copy of launch i is on its way to the host */
static void place_packs(Staged *S)
{
    const std::vector<size_t> &batch = S->batch;
    std::vector<DevFrame> &hf = S->hf;
    hf.resize(batch.size());
    S->pack_off.assign(batch.size(), 0);
    size_t need = 0;
    for (size_t b = 0; b < batch.size(); b++) {
        const FrameSlot &fs = S->slots[batch[b]];
        hf[b] = fs.F;
        hf[b].pack_src = fs.F.slab_base + fs.L.tree;     /* a borrower's is re-based by the kernel */
        hf[b].pack_bytes = (unsigned) (fs.L.pool_states - fs.L.tree);
        S->pack_off[b] = need;
        need += align_up(fs.L.pool_states - fs.L.tree, 256);
    }
    S->pack_need = need;
    S->parity ^= 1;
    char *&pack = S->d_pack[S->parity];
    (void) grow_buffer(pack, S->d_pack_bytes[S->parity], need);      /* without it: one copy per frame */
    if (!S->cstream && hipStreamCreateWithFlags(&S->cstream, hipStreamNonBlocking) != hipSuccess) {
        S->cstream = nullptr; (void) hipGetLastError();
    }
    S->packed = pack != nullptr && S->cstream != nullptr;
    for (size_t b = 0; b < batch.size(); b++) hf[b].pack_dst = S->packed ? pack + S->pack_off[b] : nullptr;
}

/* append helpers per frame of the speculating frames, per width: only for a launch of ONE width (the residency
 * sum is per build); FIASCO_AMD_SPEC_APP=<H> asks for H, as many as the chip holds beside the frames */
static void spec_helpers(Staged *S, const WaveGroups &g, int G)
{
    S->specH[0] = S->specH[1] = 0;
    if (S->no_app || (g.n[B_SPEC] && g.n[B_SPEC_WIDE])) return;
    const int wk = g.n[B_SPEC_WIDE] ? 1 : 0;
    const size_t frames = g.n[B_SPEC + wk];
    const int occ = wk ? 1 : fc_occupancy_spec();
    const char *e = fa_knob("FIASCO_AMD_SPEC_APP");
    if (!e) { S->specH[wk] = spec_app_policy(frames, S->ncu, G, wk != 0, occ); return; }
    const size_t room = spec_app_room(frames, S->ncu, G, occ), want = (size_t) (atoi(e) > 0 ? atoi(e) : 0);
    S->specH[wk] = (int) (want < room ? want : room);
}

/* the descriptors of the verifier workgroups (table workers share the chain's; verifier v of a frame owns the
 * state ids [P - 16 v, P - 16 (v - 1)) and its private tables behind the frames' control blocks) */
static std::vector<DevFrame> spec_descriptors(Staged *S, size_t first_all, size_t nall, int G, int T, size_t span,
                                              const std::vector<size_t> &priv)
{
    const int NV = G - 1 - T;
    std::vector<DevFrame> vf(nall * (size_t) (G - 1));
    size_t o = span * nall;
    for (size_t i = 0; i < nall; i++) {
        DevFrame &C = S->hf[first_all + i];
        C.spec = (FcSpecCtl *) (S->d_spec + span * i);
        C.spec_role = 0; C.spec_G = G; C.spec_T = T;
        C.spec_cap = C.P - NV * FC_SPEC_TEMPS;
        C.spec_tb = C.P;
        for (int r = 1; r < G; r++) {
            DevFrame &V = vf[i * (size_t) (G - 1) + (size_t) (r - 1)];
            V = C;
            V.spec_role = r; V.trace = nullptr; V.trace_cap = 0; V.pack_dst = nullptr;
            if (r <= T) continue;                        /* a table worker: the chain's descriptor */
            V.spec_tb = C.P - (r - T) * FC_SPEC_TEMPS;
            const size_t P = (size_t) C.P;
            char *q = S->d_spec + o;
            V.ipis = (float *) q;  q += align_up((size_t) C.NS * P * 4, 256);
            V.d5 = (float *) q;    q += align_up((size_t) C.NA * P * 4, 256);
            V.num = (float *) q;   q += align_up(P * 4, 256);
            V.den = (float *) q;   q += align_up(P * 4, 256);
            V.est = (float *) q;   q += align_up(P * 4, 256);
            V.ipdo = (float *) q;  q += align_up((size_t) FC_MAXED * P * 4, 256);
            V.used = (uint8_t *) q; q += align_up(P, 256);
            V.pool_states = (int16_t *) q; q += align_up((P + 8) * 2, 256);
            V.hits = (int *) q;
            o += priv[i];
        }
        S->spec_frames.push_back(first_all + i);
    }
    return vf;
}

/* Block-level speculation for the launch's speculating frames (the last of the batch, 256-thread build first):
 * per frame one span of control block + checkpoint slots + block list + table ring, then per verifier its
 * private <sub-block, state> tables, scan scratch and pool list.  Without memory for them: one workgroup per
 * frame.  False when a HIP call failed. */
static bool setup_spec(Staged *S, const WaveGroups &g)
{
    S->spec_frames.clear();
    S->spec_first[0] = S->spec_first[1] = 0; S->spec_n[0] = S->spec_n[1] = 0;
    const size_t nall = g.n[B_SPEC] + g.n[B_SPEC_WIDE], first_all = S->batch.size() - nall;
    if (!nall) return true;
    std::vector<DevFrame> &hf = S->hf;
    const int G = S->specG;
    const int T = spec_workers(G), NV = G - 1 - T;           /* table workers, verifiers */
    spec_helpers(S, g, G);
    S->spec_first[0] = first_all; S->spec_n[0] = g.n[B_SPEC];
    S->spec_first[1] = first_all + g.n[B_SPEC]; S->spec_n[1] = g.n[B_SPEC_WIDE];
    /* one span for every frame of the launch (sized for the largest) */
    size_t max_blocks = 0, max_tab = 0, max_slot = 0;
    std::vector<std::vector<uint16_t>> lists(nall);
    for (size_t i = 0; i < nall; i++) {
        const DevFrame &F = hf[first_all + i];
        spec_block_list(F, lists[i]);
        if (lists[i].size() / 2 > max_blocks) max_blocks = lists[i].size() / 2;
        const size_t tab = align_up(((size_t) F.NS + (size_t) F.NA) * (size_t) F.P * 4, 256);
        if (tab > max_tab) max_tab = tab;
        const size_t slot = i < g.n[B_SPEC] ? fc_spec_slot_bytes() : fc_spec_slot_bytes_wide();
        if (slot > max_slot) max_slot = slot;
    }
    const size_t off_blocks = align_up((size_t) fc_spec_ctl_bytes() + (size_t) 2 * FC_SPEC_W * max_slot, 256);      /* checkpoint + result slots */
    const size_t off_tabs = align_up(off_blocks + max_blocks * 4, 256);
    const size_t span = align_up(off_tabs + (size_t) FC_SPEC_R * max_tab, 256);
    std::vector<size_t> priv(nall);
    size_t need = span * nall;
    for (size_t i = 0; i < nall; i++) {
        const DevFrame &F = hf[first_all + i];
        const size_t P = (size_t) F.P;
        priv[i] = align_up((size_t) F.NS * P * 4, 256)
                  + align_up((size_t) F.NA * P * 4, 256) + 3 * align_up(P * 4, 256) + align_up((size_t) FC_MAXED * P * 4, 256)
                  + align_up(P, 256) + align_up((P + 8) * 2, 256) + align_up(((size_t) F.PA + 8) * 4, 256);
        need += priv[i] * (size_t) NV;
    }
    (void) grow_buffer(S->d_spec, S->d_spec_bytes, need);
    (void) grow_buffer(S->d_vframes, S->vframes_n, nall * (size_t) (G - 1));
    S->spec_ctl_span = span;
    if (!S->d_spec || !S->d_vframes) {
        for (size_t i = 0; i < nall; i++) hf[first_all + i].spec = nullptr;      /* no memory: one workgroup per frame */
        return true;
    }
    const std::vector<DevFrame> vf = spec_descriptors(S, first_all, nall, G, T, span, priv);
    /* control blocks: zero, then what the host knows (sizes, offsets, the block list) */
    bool fail = false;
    for (size_t i = 0; i < nall && !fail; i++)
        fail = hipMemsetAsync(S->d_spec + span * i, 0, off_tabs, S->stream) != hipSuccess;
    fail = fail || hipStreamSynchronize(S->stream) != hipSuccess;
    for (size_t i = 0; i < nall && !fail; i++) {
        FcSpecCtl h;
        memset(&h, 0, sizeof h);
        h.slot_bytes = (unsigned) max_slot;
        /* a colour frame: the chroma bands' tables too, from every workgroup but the chain (even
         * without table workers for the luminance band) */
        h.n_blocks = (unsigned) (lists[i].size() / 2);
        h.n_tabs = hf[first_all + i].color ? 3u * h.n_blocks : (T ? h.n_blocks : 0u);
        h.tab_stride = (unsigned) max_tab;
        /* 120 us: about what the chain needs to build the tables itself (tests: FIASCO_AMD_SPEC_TABWAIT=0
         * makes it take the worker's tables only when they are there already) */
        h.tab_wait = (unsigned) knob_int("FIASCO_AMD_SPEC_TABWAIT", 12000);
        h.off_blocks = off_blocks; h.off_tabs = off_tabs;
        /* append helpers of the frame's width group */
        const int wk = i < g.n[B_SPEC] ? 0 : 1;
        h.app_H = (unsigned) S->specH[wk];
        h.app_min = wk ? 2048u : 512u;               /* two passes of the workgroup's lanes */
        h.app_dbg = (unsigned) knob_int("FIASCO_AMD_SPEC_APPDBG", 0);
        h.app_wait = 100000u * (unsigned) knob_int("FIASCO_AMD_SPEC_APPWAIT_MS", 2000);      /* 100 MHz ticks */
        fail = hipMemcpy(S->d_spec + span * i, &h, sizeof h, hipMemcpyHostToDevice) != hipSuccess;
        if (!fail && !lists[i].empty())
            fail = hipMemcpy(S->d_spec + span * i + off_blocks, lists[i].data(), lists[i].size() * 2, hipMemcpyHostToDevice) != hipSuccess;
    }
    fail = fail || hipMemcpy(S->d_vframes, vf.data(), sizeof(DevFrame) * vf.size(), hipMemcpyHostToDevice) != hipSuccess;
    return !fail;
}

/* Big frames that leave the chip empty (a step of a video: 30 GOPs): W workgroups build the tables of a frame
 * (frame_coder.h FcCoop), one of 512 threads per CU, all resident: W x frames <= CUs, nothing else beside them.
 * Returns W (1: off) for the `plain' frames of build b at batch position `at' and writes their control blocks. */
static unsigned setup_coop(Staged *S, Build b, size_t at, size_t plain, bool &fail)
{
    const std::vector<DevFrame> &hf = S->hf;
    unsigned W = 1;
    bool any_bx = false;                /* a long basis: its table rows are built by the frame's own workgroup */
    for (size_t i = at; i < at + plain; i++) any_bx = any_bx || hf[i].bx != nullptr;
    if (b == B_BIG_WIDE && S->batch.size() == plain && !S->no_coop && !any_bx) W = coop_policy(plain, S->ncu);
    if (S->no_coop) S->no_coop_done = true;
    if (W == 1) return W;
    FcCoop &hdr = S->coop_hdr;
    memset(&hdr, 0, sizeof hdr);
    for (hdr.depth = 1; (1u << hdr.depth) < W; hdr.depth++) {}
    /* tests: FIASCO_AMD_COOP_WAIT_MS shortens the frame's wait, FIASCO_AMD_COOP_DEAF=1 sends the helpers
     * home at once (the frame then fails with FC_ERR_COOP and is searched again by one workgroup) */
    hdr.done_ticks = 100000ull * (unsigned long long) knob_int("FIASCO_AMD_COOP_WAIT_MS", FC_COOP_DONE_TICKS / 100000);
    hdr.quit = fa_knob("FIASCO_AMD_COOP_DEAF") ? 1u : 0u;
    hdr.minsub = 1;
    for (size_t i = at; i < at + plain && !fail; i++)
        fail = hipMemcpyAsync(hf[i].coop, &hdr, sizeof(FcCoop), hipMemcpyHostToDevice, S->stream) != hipSuccess;
    stats_update([&](fiasco_amd_stats &st) { st.coop_frames += plain; st.coop_workgroups = W; });
    return W;
}

/* one persistent launch per kernel build, speculating builds first; the queue's frames with their ring */
static bool start_launches(Staged *S, const WaveGroups &g, bool fail)
{
    std::vector<DevFrame> &hf = S->hf;
    const size_t frames = S->batch.size();
    /* bound of a queued frame's wait for a slab (frame_coder.hip); tests shorten it */
    const unsigned long long qwait = 100000ull * (unsigned long long) knob_int("FIASCO_AMD_QUEUE_WAIT_MS", FC_QUEUE_WAIT_TICKS / 100000);
    for (int k = 0; k < 2 && !fail; k++) {
        if (!S->spec_n[k]) continue;
        /* without the verifiers' buffers: G = 1, the chain alone */
        const bool on = S->d_spec && S->d_vframes && !S->spec_frames.empty();
        DevFrame *vfr = S->d_vframes ? S->d_vframes + (S->spec_first[k] - S->spec_first[0]) * (size_t) (S->specG - 1) : nullptr;
        k_build[B_SPEC + k].spec_launch(S->d_frames + S->spec_first[k], vfr, (unsigned) S->spec_n[k],
                                        on ? (unsigned) S->specG : 1u, on ? (unsigned) S->specH[k] : 0u, S->stream);
    }
    size_t first = 0;
    for (int b = 0; b < B_SPEC && !fail; b++) {
        launch_fn *const launch = k_build[b].launch;
        size_t plain = g.n[b], at = first;
        if (g.borrow[b]) {
            /* the queue: g.lend[b] frames with slabs first, then the frames that borrow one */
            const size_t nq = g.lend[b] + g.borrow[b];
            if (!g.lend[b] || !S->packed || !queue_resources(S, frames)) {
                for (size_t i = at + g.lend[b]; i < at + nq; i++) hf[i].status = FC_ERR_INTERNAL;
                fail = fail || hipMemcpyAsync(S->d_frames + at, hf.data() + at, sizeof(DevFrame) * nq,
                                              hipMemcpyHostToDevice, S->stream) != hipSuccess;
                if (g.lend[b])
                    launch(S->d_frames + at, (unsigned) g.lend[b], (unsigned) g.lend[b], nullptr, nullptr, nullptr, qwait, 1u, S->stream);
            } else {
                unsigned long long *ring = S->d_ring + (size_t) b * frames;
                fail = fail || hipMemsetAsync(S->d_queue + 2 * b, 0, 2 * sizeof(unsigned), S->stream) != hipSuccess;
                fail = fail || hipMemsetAsync(ring, 0, nq * sizeof(unsigned long long), S->stream) != hipSuccess;
                launch(S->d_frames + at, (unsigned) nq, (unsigned) g.lend[b], ring, S->d_queue + 2 * b,
                       S->d_ptrmask, qwait, 1u, S->stream);
            }
            at += nq; plain -= nq;
        }
        if (plain) {
            const unsigned W = setup_coop(S, (Build) b, at, plain, fail);
            launch(S->d_frames + at, (unsigned) plain, (unsigned) plain, nullptr, nullptr, nullptr, qwait, W, S->stream);
        }
        first += g.n[b];
    }
    return fail;
}

/* build the next launch, upload its descriptors and start the kernel(s); nothing is waited for.  Returns false
 * when there is nothing to launch. */
static bool launch_wave(Staged *S)
{
    WaveGroups g;
    if (!order_batch(S, g)) return false;
    place_packs(S);
    S->d_trace = nullptr;
    const int trace_cap = 400000;
    if (fa_knob("FIASCO_AMD_TRACE") && hipMalloc((void **) &S->d_trace, sizeof(FcTrace) * trace_cap) == hipSuccess) {
        S->hf[0].trace = S->d_trace; S->hf[0].trace_cap = trace_cap;
    }
    bool fail = !setup_spec(S, g);
    fail = fail || hipMemcpyAsync(S->d_frames, S->hf.data(), sizeof(DevFrame) * S->batch.size(),
                                  hipMemcpyHostToDevice, S->stream) != hipSuccess;
    fail = fail || hipEventRecord(S->ev0, S->stream) != hipSuccess;
    fail = start_launches(S, g, fail);
    fail = fail || hipGetLastError() != hipSuccess;
    fail = fail || hipEventRecord(S->ev1, S->stream) != hipSuccess;
    S->launch_failed = fail;
    return true;
}

/* wait for the launch, download the descriptors (S->hf) and the counters of speculation, write the trace.  False
 * when the launch or the download failed. */
static bool download_wave(Staged *S)
{
    std::vector<DevFrame> &hf = S->hf;
    bool fail = S->launch_failed;
    fail = fail || hipStreamSynchronize(S->stream) != hipSuccess;
    if (!fail) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, S->ev0, S->ev1) == hipSuccess) {
            stats_update([&](fiasco_amd_stats &st) { st.kernel_ms += ms; st.launches += 1; });
        }
        fail = hipMemcpy(hf.data(), S->d_frames, sizeof(DevFrame) * S->batch.size(),
                         hipMemcpyDeviceToHost) != hipSuccess;
    }
    if (!fail && !S->spec_frames.empty() && S->d_spec) {
        std::vector<FcSpecCtl> ctl(S->spec_frames.size());
        if (hipMemcpy2D(ctl.data(), sizeof(FcSpecCtl), S->d_spec, S->spec_ctl_span, sizeof(FcSpecCtl), ctl.size(),
                        hipMemcpyDeviceToHost) == hipSuccess)
            stats_update([&](fiasco_amd_stats &st) {
                for (size_t i = 0; i < ctl.size(); i++) {
                    st.spec_tasks += ctl[i].n_tasks; st.spec_confirmed += ctl[i].n_confirmed;
                    st.spec_wrong += ctl[i].n_wrong; st.spec_timeout += ctl[i].n_timeout;
                    st.spec_inline += ctl[i].n_inline; st.spec_wait += ctl[i].t_wait;
                    st.spec_tab_used += ctl[i].n_tab_used; st.spec_tab_missed += ctl[i].n_tab_missed;
                    st.spec_adopted += ctl[i].n_adopted;
                    st.spec_app_rows += ctl[i].n_app_dealt; st.spec_app_wait += ctl[i].t_app_wait;
                }
            });
        else (void) hipGetLastError();
    }
    const char *trace_path = fa_knob("FIASCO_AMD_TRACE");
    if (S->d_trace && !fail && trace_path) {
        std::vector<FcTrace> tr((size_t) hf[0].trace_n);
        if (hipMemcpy(tr.data(), S->d_trace, sizeof(FcTrace) * tr.size(), hipMemcpyDeviceToHost) == hipSuccess) {
            FILE *tf = fopen(trace_path, "wb");
            if (tf) { fwrite(tr.data(), sizeof(FcTrace), tr.size(), tf); fclose(tf); }
        }
    }
    if (S->d_trace) { (void) hipFree(S->d_trace); S->d_trace = nullptr; }
    return !fail;
}

/* All automata of the launch come down into one pinned buffer: one copy of the packed buffer on the copy stream
 * (not waited for here: the next launch may start first), or -- without a packed buffer -- one async copy per
 * frame.  Returns every frame's offset in S->pinned ((size_t) -1: not there, collect() copies it itself). */
static std::vector<size_t> fetch_automata(Staged *S)
{
    const std::vector<size_t> &batch = S->batch;
    const std::vector<DevFrame> &hf = S->hf;
    std::vector<size_t> off(batch.size(), (size_t) -1);
    size_t need = 0;
    if (S->packed) {
        need = S->pack_need;
        for (size_t b = 0; b < batch.size(); b++) if (hf[b].status == FC_OK) off[b] = S->pack_off[b];
    } else
        for (size_t b = 0; b < batch.size(); b++)
            if (hf[b].status == FC_OK) {
                const Layout &L = S->slots[batch[b]].L;
                off[b] = need;
                need += align_up(L.pool_states - L.tree, 256);
            }
    if (S->copy_pending) { (void) hipStreamSynchronize(S->cstream); S->copy_pending = false; }
    (void) grow_buffer(S->pinned, S->pinned_bytes, need, true);
    if (S->pinned && S->packed) {
        if (hipMemcpyAsync(S->pinned, S->d_pack[S->parity], need, hipMemcpyDeviceToHost, S->cstream) == hipSuccess)
            S->copy_pending = true;
        else {
            (void) hipGetLastError();
            off.assign(batch.size(), (size_t) -1);
        }
    } else if (S->pinned) {
        for (size_t b = 0; b < batch.size(); b++)
            if (off[b] != (size_t) -1) {
                const FrameSlot &fs = S->slots[batch[b]];
                if (hipMemcpyAsync(S->pinned + off[b], fs.base + fs.L.tree, fs.L.pool_states - fs.L.tree,
                                   hipMemcpyDeviceToHost, S->stream) != hipSuccess)
                    off[b] = (size_t) -1;
            }
        (void) hipStreamSynchronize(S->stream);
    }
    return off;
}

/* What becomes of the frame at batch position b, by its status, in this order: a capacity guess that was too small
 * (a bigger slab, encoded again), append helpers that did not answer (again without helpers), table helpers that
 * did not answer (again by one workgroup), a queued frame that got no slab (a slab of its own), else done: collected
 * (`off': its automaton in S->pinned) or failed with a message. */
static void frame_outcome(Staged *S, size_t b, size_t off)
{
    FrameSlot &fs = S->slots[S->batch[b]];
    fa_job *job = &S->jobs[fs.job];
    const int st = S->hf[b].status;
    void *tr_keep = fs.F.trace;
    fs.F = S->hf[b];
    fs.F.trace = (FcTrace *) tr_keep; fs.F.trace_cap = 0;
    if (fs.ext_pix) fs.F.pix16 = fs.ext_pix;
    const size_t cap = align_up(job->cp.limit_states, 64);
    /* (a frame that shares its slab with verifiers has less than fs.P for itself -- their private
     * state ids lie at the top of the capacity --: at the state limit it is encoded once more by one
     * workgroup with all of it, like the reference would, before "Maximum number of states" is said) */
    if (st == FC_ERR_CAPACITY && ((size_t) fs.P < cap || (size_t) fs.PA < cap || fs.spec)) {
        /* capacity guess too small: bigger slab, same inputs, encode again */
        stats_update([](fiasco_amd_stats &st) { st.reencodes += 1; });
        size_t np = align_up((size_t) fs.P + (size_t) fs.P / 2, 64);
        size_t npa = align_up((size_t) fs.PA + (size_t) fs.PA / 2, 64);
        if ((size_t) fs.P >= cap || np >= cap) fs.spec = false;
        /* a frame of a launch with more workgroups than CUs that outgrows the 256-thread build would come
         * back in the 1024-thread speculating build, one workgroup per CU: its verifiers might not be
         * resident (the chain's waits are bounded, but slow) -- one workgroup for such a frame */
        if (np > 3072 && S->specG > 1 && (size_t) S->specG * S->n > (size_t) S->ncu) fs.spec = false;
        if (fs.base) slab_release(fs.base, fs.bytes, fs.slab_dev);
        /* a borrower gets a slab of its own; its pixel planes stay where they are (the queue's
         * pixel buffer or an upload buffer): the host copy may belong to the next pass by now */
        if (fs.borrow) { fs.borrow = false; S->borrowers--; }
        fs.base = nullptr; fs.staged = false;
        fs.P = (int) (np > cap ? cap : np);
        fs.PA = (int) (npa > cap ? cap : npa);
        if (fs.PA < fs.P) fs.PA = fs.P;
        if (fs.P > 12 * 1024) fs.spec = false;     /* beyond the speculating builds: one (wide) workgroup */
        if (!stage_slot(S, fs)) fs.done = true;
        return;
    }
    if (st == FC_ERR_COOP && fs.spec && !S->no_app) {
        /* the append helpers of a speculating frame did not answer in time: again without helpers */
        S->no_app = true;
        return;
    }
    if (st == FC_ERR_COOP && !S->no_coop_done) {
        /* the helper workgroups of the frame were not there in time (not resident: masked CUs, a busy device):
         * the frame keeps its slab and is searched again by one workgroup -- a retry instead of a failure */
        S->no_coop = true;
        return;
    }
    if (st == FC_ERR_QUEUE && fs.borrow) {
        /* the frame never got a slab from the queue (bounded wait in the kernel): a slab of its
         * own in the next launch; its pixel planes stay where they are */
        fs.borrow = false; S->borrowers--;
        fs.base = nullptr; fs.staged = false;
        if (!stage_slot(S, fs)) fs.done = true;
        return;
    }
    fs.done = true;
    if (st == FC_OK) {
        /* unpacking into the job's fa_wfa is host work on host memory: deferred so that
         * a following submit can start the device first (flush_unpack) */
        if (S->pinned && off != (size_t) -1) S->to_unpack.push_back(std::make_pair(S->batch[b], off));
        else S->good += collect(S, fs, nullptr);
        return;
    }
    const char *msg = "device coder failed";
    if (st == FC_ERR_STATES || st == FC_ERR_CAPACITY) msg = "Maximum number of states reached!";
    else if (st == FC_ERR_NOROOT) msg = "No root state generated!";
    else if (st == FC_ERR_QUEUE) msg = "device coder: frame queue gave no slab";
    else if (st == FC_ERR_COOP) msg = "device coder: the helper workgroups of the frame did not answer";
    else if (st == FC_ERR_INTERNAL) msg = "device coder: frame exceeds a built-in capacity (recursion depth, snapshot stack or 16384 states)";
    if (st > FC_ERR_QUEUE) snprintf(job->errmsg, sizeof job->errmsg, "%s (status %d)", msg, st);
    else snprintf(job->errmsg, sizeof job->errmsg, "%s", msg);
}

/* wait for the launch and settle every frame of it (frame_outcome) */
static void complete_wave(Staged *S)
{
    if (!download_wave(S)) {
        const char *why = hipGetErrorString(hipGetLastError());   /* reading it clears it: once */
        for (size_t b = 0; b < S->batch.size(); b++) {
            FrameSlot &fs = S->slots[S->batch[b]];
            snprintf(S->jobs[fs.job].errmsg, sizeof S->jobs[fs.job].errmsg, "HIP error: %s", why);
            fs.done = true;
        }
        S->broken = true;
        return;
    }
    const std::vector<size_t> off = fetch_automata(S);
    for (size_t b = 0; b < S->batch.size(); b++) frame_outcome(S, b, off[b]);
    (void) hipStreamSynchronize(S->stream);
}

static void flush_unpack(Staged *S)
{
    if (S->copy_pending) { (void) hipStreamSynchronize(S->cstream); S->copy_pending = false; }
    for (size_t i = 0; i < S->to_unpack.size(); i++)
        S->good += collect(S, S->slots[S->to_unpack[i].first], S->pinned + S->to_unpack[i].second);
    S->to_unpack.clear();
}

/* start encoding every staged frame; returns immediately (the kernel runs) */
static int core1_submit(void *h)
{
    Staged *S = (Staged *) h;
    if (!S || !S->ok) return 0;
    if (S->inflight) return 1;
    /* job status / automata of the previous pass stay readable until fa_core_finish() */
    for (size_t k = 0; k < S->slots.size(); k++) {
        S->slots[k].done = false;
        S->slots[k].src = S->jobs[S->slots[k].job].image;      /* see FrameSlot::src */
    }
    S->good = 0; S->broken = false;
    if (S->up_pending) {
        /* a new pass takes over the replacement inputs: the launch waits for their transfer,
         * descriptors are uploaded by every launch anyway */
        (void) hipStreamWaitEvent(S->stream, S->ev_up, 0);
        for (size_t k = 0; k < S->slots.size(); k++) {
            FrameSlot &fs = S->slots[k];
            if (fs.ext_next) { fs.ext_pix = fs.ext_next; fs.F.pix16 = fs.ext_pix; }
        }
        S->up_parity ^= 1;
        S->up_pending = false;
    }
    S->inflight = launch_wave(S);
    return 1;
}

/* wait for the submitted launch and bring every frame to completion (re-encodes with larger
 * slabs, later waves of a batch that did not fit into HBM at once).  After it returns the
 * jobs' automata are in host memory and the device is free for the next submit. */
static int core1_finish2(void *h, int resubmit)
{
    Staged *S = (Staged *) h;
    if (!S || !S->ok) return 0;
    if (!S->inflight) { core1_submit(h); }
    for (size_t k = 0; k < S->slots.size(); k++) S->jobs[S->slots[k].job].status = 0;
    for (;;) {
        if (S->inflight) { complete_wave(S); S->inflight = false; if (S->broken) break; }
        {   /* anything left to encode (bigger slabs, later waves)?  then the staging buffer
             * is needed again: unpack first */
            bool more = false;
            for (size_t k = 0; k < S->slots.size(); k++) if (!S->slots[k].done) more = true;
            if (more) flush_unpack(S);
        }
        if (launch_wave(S)) { S->inflight = true; continue; }
        /* stage a later wave (frames that did not fit while others held their slabs):
         * finished frames give their slabs back first (they are re-staged by the next
         * run if the batch is encoded again) */
        bool any = false, pending = false;
        for (size_t k = 0; k < S->slots.size(); k++) {
            FrameSlot &fs = S->slots[k];
            if (!fs.staged && !fs.done && !S->jobs[fs.job].errmsg[0]) pending = true;
        }
        if (!pending) break;
        for (size_t k = 0; k < S->slots.size(); k++) {
            FrameSlot &fs = S->slots[k];
            if (fs.done && fs.base) { slab_release(fs.base, fs.bytes, fs.slab_dev); fs.base = nullptr; fs.staged = false; }
        }
        for (size_t k = 0; k < S->slots.size(); k++) {
            FrameSlot &fs = S->slots[k];
            if (fs.staged || fs.done || S->jobs[fs.job].errmsg[0]) continue;
            if (stage_slot(S, fs)) any = true; else if (!fs.rejected) break;
        }
        if (!any) break;
    }
    int good_before = S->good;
    if (resubmit && !S->broken) {
        /* next pass on the device first, then the host-side unpacking of this one */
        std::vector<std::pair<size_t, size_t>> keep;
        keep.swap(S->to_unpack);
        core1_submit(h);                           /* resets S->good */
        S->to_unpack.swap(keep);
        int g = S->good;
        S->good = good_before;
        flush_unpack(S);
        good_before = S->good;
        S->good = g;
        return good_before;
    }
    flush_unpack(S);
    return S->good;
}
