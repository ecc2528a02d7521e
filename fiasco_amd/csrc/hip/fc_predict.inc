/*
 *  fc_predict.inc -- prediction and motion compensation, big build only: block norms and the
 *  motion search (op_norms, op_mc_search), the start and the end of a predicted range
 *  (op_pred_setup, op_pred_finish) and what they put aside (pred_save_tables, subtract_mc_dev).
 *
 *  Reference: codec/prediction.c (predict_range :96-208), codec/mwfa.c.
 *
 *  Part of the frame kernel: frame_coder.hip includes it (see the map there); it does not
 *  compile alone.
 */

#if FC_VARIANT_BIG
/* ------------------------------------------------------------------ prediction (codec/prediction.c)
 *
 * predict_range (:96-208) tries a third alternative for a range after its linear combination
 * and its subdivision: approximate the range coarsely (its DC part for an intra frame, a motion
 * compensated block of the reference frame otherwise), run the SAME partition search on the
 * residual (`delta' = YES: delta pool, delta coefficient model), keep what is cheapest.  The
 * states the subdivision appended are put aside meanwhile (store_state_data, :502-565) and the
 * residual search re-uses their ids.  Here:
 *   OP_PRED_SETUP   block pixels + norms -> F.pix_save, residual -> sh.pixels, tables of the
 *                   residual block into the SECOND table set (ipis_alt / d5_alt / d4_alt: the
 *                   reference swaps the per-state table pointers, :302-309,443-450), automaton
 *                   rows of the displaced states -> F.sv_auto, delta models become active
 *   op_append       copies the table rows of a displaced id to F.sv_gram / F.sv_img the first
 *                   time the residual search appends a state with that id (copy on write)
 *   OP_PRED_FINISH  everything back; on failure the saved rows return, on success the new
 *                   states get zeroed <sub-block, state> rows (:342-345,481-484)
 */

/* squared norms of the sub-blocks of a block of 2^level pixels in sh.pixels, heap order */
__device__ void block_norms(Sh &sh, int level, int ns)
{
    const int tid = threadIdx.x;
    for (int slot = tid; slot < ns; slot += B) {
        int depth = 31 - __clz(slot + 1);
        int lv = level - depth, size = 1 << lv;
        int adr = slot + 1 - (1 << depth);
        float nrm = 0;
        const float *px = sh.pixels + adr * size;
        for (int k = 0; k < size; k++) nrm += px[k] * px[k];      /* sequential, codec/approx.c:388-389 */
        sh.norms[slot] = nrm;
    }
}

/* exchange the active and the resting model set (all lanes; barriers by the caller) */
__device__ void swap_model_sets(Sh &sh)
{
    const int tid = threadIdx.x;
#if FC_HM           /* models of more 16-byte units than lanes */
    for (int i = tid; i < sh.n16; i += B) {
        uint4 a = ((uint4 *) &sh.cb)[i], b = ((uint4 *) &sh.dcb)[i];
        ((uint4 *) &sh.cb)[i] = b; ((uint4 *) &sh.dcb)[i] = a;
    }
    if (tid == 128) {
#else
    if (tid < sh.n16) {
        uint4 a = ((uint4 *) &sh.cb)[tid], b = ((uint4 *) &sh.dcb)[tid];
        ((uint4 *) &sh.cb)[tid] = b; ((uint4 *) &sh.dcb)[tid] = a;
    } else if (tid == 128) {
#endif
        Pool t = sh.pool; sh.pool = sh.dpool; sh.dpool = t;
#if FC_GM
        { int k = sh.gm.pk[0]; sh.gm.pk[0] = sh.gm.pk[1]; sh.gm.pk[1] = k; k = sh.gm.ck[0]; sh.gm.ck[0] = sh.gm.ck[1]; sh.gm.ck[1] = k; }
        sh.gm.qa ^= 1;
#endif
    } else if (tid == 129) {
        int i; float f;
        i = sh.par.rpf_mant; sh.par.rpf_mant = sh.dq.rpf_mant; sh.dq.rpf_mant = i;
        i = sh.par.dc_mant; sh.par.dc_mant = sh.dq.dc_mant; sh.dq.dc_mant = i;
        i = sh.par.sy; sh.par.sy = sh.dq.sy; sh.dq.sy = i;
        i = sh.par.dcs; sh.par.dcs = sh.dq.dcs; sh.dq.dcs = i;
        f = sh.par.rpf_range; sh.par.rpf_range = sh.dq.rpf_range; sh.dq.rpf_range = f;
        f = sh.par.dc_range; sh.par.dc_range = sh.dq.dc_range; sh.dq.dc_range = f;
        i = sh.par.half_nd; sh.par.half_nd = sh.dq.half_nd; sh.dq.half_nd = i;
        i = sh.par.half_dc; sh.par.half_dc = sh.dq.half_dc; sh.dq.half_dc = i;
    }
}

/* ---- motion compensation (codec/mwfa.c; P frames, full-pixel vectors) ---- */

/* MPEG's vector-component code lengths (mv_code_table[][1], codec/mwfa.c:40-50) */
__device__ __forceinline__ float mv_bits(int v, int sr)
{
    /* lengths 11 11 11 11 11 11 10 10 10 8 8 8 7 5 4 3 | 1 | mirrored: one nibble per code */
    const unsigned long long len = 0xbbbbbbaaa8887543ull;
    const int i = v + sr;
    if (i == 16) return 1.0f;
    return (float) ((len >> (4 * (i < 16 ? 15 - i : i - 17))) & 15u);
}

/* fill_norms_table (codec/mwfa.c:545-602): squared norm of original - displaced reference block
 * for every displacement of the search window, 0 outside the frame.  One displacement per lane
 * and pass; per displacement the pixels are summed in raster order like mcpe_norm (:658-684). */
__device__ void fill_norms(const DevFrame &__restrict__ F, int x0, int y0, int level)
{
    const int tid = threadIdx.x, sr = F.search_range, n = 4 * sr * sr;
    const int bw = (int) width_of_level(level), bh = (int) height_of_level(level), W = F.width, H = F.height;
    float *dst = F.mc_fwd + (size_t) (level - F.p_min) * n;
    float *dstb = F.mc_bwd + (size_t) (level - F.p_min) * n;
    const int16_t *orig = F.pix16 + (size_t) y0 * W + x0;
    const bool bframe = F.frame_type == 2;
    for (int idx = tid; idx < n; idx += B) {
        const int mx = idx % (2 * sr) - sr, my = idx / (2 * sr) - sr;
        float norm = 0.0f, normb = 0.0f;
        if (!(x0 + mx < 0 || x0 + mx + bw > W || y0 + my < 0 || y0 + my + bh > H)) {
            const int16_t *ref = F.past + (size_t) (y0 + my) * W + (x0 + mx);
            for (int y = 0; y < bh; y++)
                for (int x = 0; x < bw; x++) {
                    const int q = (int) (short) (orig[(size_t) y * W + x] - ref[(size_t) y * W + x]) / 16;
                    norm += (float) (q * q);
                }
            if (bframe) {
                const int16_t *reb = F.future + (size_t) (y0 + my) * W + (x0 + mx);
                for (int y = 0; y < bh; y++)
                    for (int x = 0; x < bw; x++) {
                        const int q = (int) (short) (orig[(size_t) y * W + x] - reb[(size_t) y * W + x]) / 16;
                        normb += (float) (q * q);
                    }
            }
            dst[idx] = norm;
            if (bframe) dstb[idx] = normb;
        } else {
            dst[idx] = 0.0f;                 /* both tables, whatever the frame type (:576-577) */
            if (F.mc_bwd) dstb[idx] = 0.0f;
        }
    }
}

/* after a child of a motion compensated node: table of the child's level if the child was not
 * searched (subdivide.c:311-315), then update_norms_table (prediction.c:229-254); `first`
 * stands for the clear_norms_table at the node's entry (0 + x == x) */
__device__ __noinline__ void op_norms(DevFrame &__restrict__ F, Sh &__restrict__ sh, int level, int first,
                                      int fill_level, int xy)
{
    const int tid = threadIdx.x, n = 4 * F.search_range * F.search_range;
    if (fill_level >= 0) {
        fill_norms(F, xy & 0xffff, xy >> 16, fill_level);
        __syncthreads();
    }
    if (level > F.p_min) {
        float *dst = F.mc_fwd + (size_t) (level - F.p_min) * n;
        const float *src = dst - n;
        for (int i = tid; i < n; i += B) dst[i] = first ? 0.0f + src[i] : dst[i] + src[i];
        if (F.frame_type == 2) {
            float *dstb = F.mc_bwd + (size_t) (level - F.p_min) * n;
            const float *srcb = dstb - n;
            for (int i = tid; i < n; i += B) dstb[i] = first ? 0.0f + srcb[i] : dstb[i] + srcb[i];
        } else if (first && F.mc_bwd) {      /* clear_norms_table clears both */
            float *dstb = F.mc_bwd + (size_t) (level - F.p_min) * n;
            for (int i = tid; i < n; i += B) dstb[i] = 0.0f;
        }
    }
}

/* find_best_mv (codec/mwfa.c:686-798): first displacement, in scan order, with the smallest
 * costs norm + (bits_x + bits_y) * price.  All lanes; result on lane 0. */
__device__ void best_mv(const DevFrame &__restrict__ F, Sh &__restrict__ sh, const float *norms, int x0, int y0,
                        int bw, int bh, float price, int &mx_out, int &my_out, float &bits, float &costs_out)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, sr = F.search_range, n = 4 * sr * sr;
    const int W = F.width, H = F.height;
    unsigned long long best = ~0ull;
    for (int idx = tid; idx < n; idx += B) {
        const int mx = idx % (2 * sr) - sr, my = idx / (2 * sr) - sr;
        if (x0 + mx >= 0 && y0 + my >= 0 && x0 + mx + bw <= W && y0 + my + bh <= H) {
            const float costs = norms[idx] + (mv_bits(mx, sr) + mv_bits(my, sr)) * price;
            /* costs >= 0: the float's bit pattern orders like the value */
            const unsigned long long key = ((unsigned long long) __float_as_uint(costs) << 32) | (unsigned) idx;
            if (key < best) best = key;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long t = __shfl_xor(best, o);
        if (t < best) best = t;
    }
    __syncthreads();                         /* sh.mcred of an earlier call has been read */
    if (lane == 0) sh.mcred[wave] = best;
    __syncthreads();
    unsigned long long g = sh.mcred[0];
    for (int i = 1; i < B / 64; i++) if (sh.mcred[i] < g) g = sh.mcred[i];
    mx_out = my_out = 0;
    costs_out = MAXCOSTS;
    if (g != ~0ull && __uint_as_float((unsigned) (g >> 32)) < MAXCOSTS) {
        const int idx = (int) (g & 0xffffffffu);
        mx_out = idx % (2 * sr) - sr; my_out = idx / (2 * sr) - sr;
        costs_out = __uint_as_float((unsigned) (g >> 32));
    }
    bits = mv_bits(mx_out, sr) + mv_bits(my_out, sr);
}

/* find_P_frame_mc / find_B_frame_mc (codec/mwfa.c:302-543; cross_B_search is never set: the
 * reference copies it from half_pixel_prediction, codec/coder.c:359, and half-pixel vectors are
 * refused by the host).  Result in sh.mc. */
__device__ __noinline__ void op_mc_search(DevFrame &__restrict__ F, Sh &__restrict__ sh, int level, int xy, int fill)
{
    const int tid = threadIdx.x, sr = F.search_range, n = 4 * sr * sr;
    const int x0 = xy & 0xffff, y0 = xy >> 16;
    const int bw = (int) width_of_level(level), bh = (int) height_of_level(level), W = F.width;
    const float price = sh.st[sh.sp].price;
    if (fill & 1) { fill_norms(F, x0, y0, level); __syncthreads(); }
    if (fill & 2) {
        /* a node above p_min_level whose children were never visited (its level is not above the
         * smallest block level, which a colour stream ratchets upwards, codec/coder.c:785-797):
         * the table is what clear_norms_table left at the entry (prediction.c:210-227) */
        float *t = F.mc_fwd + (size_t) (level - F.p_min) * n;
        for (int i = tid; i < n; i += B) t[i] = 0.0f;
        if (F.mc_bwd) { t = F.mc_bwd + (size_t) (level - F.p_min) * n; for (int i = tid; i < n; i += B) t[i] = 0.0f; }
        __syncthreads();
    }
    int fx, fy, bx = 0, by = 0;
    float fbits, bbits = 0, fcosts, bcosts = 0;
    best_mv(F, sh, F.mc_fwd + (size_t) (level - F.p_min) * n, x0, y0, bw, bh, price, fx, fy, fbits, fcosts);
    if (F.frame_type != 2) {
        if (tid == 0) { sh.mc.type = MV_FORWARD; sh.mc.fx = fx; sh.mc.fy = fy; sh.mc.bx = sh.mc.by = 0;
                        sh.mc.bits = fbits; sh.mc.tree_bits = 1.0f; }
        return;
    }
    best_mv(F, sh, F.mc_bwd + (size_t) (level - F.p_min) * n, x0, y0, bw, bh, price, bx, by, bbits, bcosts);
    /* both vectors together: norm of original - (forward block + backward block) / 2, summed in
     * raster order (mcpe_norm :658-684).  The terms are integers: as long as the total stays
     * below 2^24 every partial sum is exact and the order does not matter -- summed in parallel;
     * otherwise lane 0 repeats the sum in order. */
    const int16_t *orig = F.pix16 + (size_t) y0 * W + x0;
    const int16_t *r1 = F.past + (size_t) (y0 + fy) * W + (x0 + fx);
    const int16_t *r2 = F.future + (size_t) (y0 + by) * W + (x0 + bx);
    unsigned long long part = 0;
    for (int i = tid; i < bw * bh; i += B) {
        const int x = i % bw, y = i / bw;
        const int q = (int) (short) (orig[(size_t) y * W + x] - ((int) r1[(size_t) y * W + x] + (int) r2[(size_t) y * W + x]) / 2) / 16;
        part += (unsigned long long) (q * q);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    __syncthreads();
    if ((tid & 63) == 0) sh.mcred[tid >> 6] = part;
    __syncthreads();
    if (tid == 0) {
        unsigned long long total = 0;
        for (int i = 0; i < B / 64; i++) total += sh.mcred[i];
        float inorm;
        if (total < (1ull << 24)) inorm = (float) total;
        else {
            inorm = 0.0f;
            for (int y = 0; y < bh; y++)
                for (int x = 0; x < bw; x++) {
                    const int q = (int) (short) (orig[(size_t) y * W + x] - ((int) r1[(size_t) y * W + x] + (int) r2[(size_t) y * W + x]) / 2) / 16;
                    inorm += (float) (q * q);
                }
        }
        const float forward_costs = fcosts + 3 * price, backward_costs = bcosts + 3 * price;
        const float interp_bits = fbits + bbits;
        const float interp_costs = inorm + (interp_bits + 2) * price;
        int type;
        if (forward_costs <= interp_costs) type = forward_costs <= backward_costs ? MV_FORWARD : MV_BACKWARD;
        else type = backward_costs <= interp_costs ? MV_BACKWARD : MV_INTERPOLATED;
        sh.mc.type = type;
        sh.mc.fx = type != MV_BACKWARD ? fx : 0; sh.mc.fy = type != MV_BACKWARD ? fy : 0;
        sh.mc.bx = type != MV_FORWARD ? bx : 0; sh.mc.by = type != MV_FORWARD ? by : 0;
        sh.mc.tree_bits = type == MV_INTERPOLATED ? 2.0f : 3.0f;
        sh.mc.bits = type == MV_FORWARD ? fbits : type == MV_BACKWARD ? bbits : interp_bits;
    }
}

/* subtract_mc (codec/mwfa.c:156-300): private chroma planes = original chroma - luminance motion
 * compensation with the vector components rounded to even; called once, at the first chroma band */
__device__ void subtract_mc_dev(DevFrame &__restrict__ F, Sh &__restrict__ sh)
{
    const int tid = threadIdx.x, W = F.width;
    const size_t npix = (size_t) F.plane;
    for (size_t i = tid; i < 2 * npix; i += B) F.pix_chroma[i] = F.pix16[npix + i];
    __syncthreads();
    for (int s = F.basis_states; s < sh.states; s++)                 /* blocks do not overlap */
        for (int l = 0; l < 2; l++) {
            const int type = F.mv[(0 * 2 + l) * F.PA + s];
            if (type == MV_NONE) continue;       /* uniform */
            const int lv = (int) F.level_of_state[s] - 1;
            const int bw = (int) width_of_level(lv), bh = (int) height_of_level(lv);
            const int x0 = F.x[l * F.PA + s], y0 = F.y[l * F.PA + s];
            const int fx = (F.mv[(1 * 2 + l) * F.PA + s] / 2) * 2, fy = (F.mv[(2 * 2 + l) * F.PA + s] / 2) * 2;
            const int bx = (F.mv[(3 * 2 + l) * F.PA + s] / 2) * 2, by = (F.mv[(4 * 2 + l) * F.PA + s] / 2) * 2;
            for (int b = 0; b < 2; b++) {
                int16_t *o = F.pix_chroma + (size_t) b * npix + (size_t) y0 * W + x0;
                const int16_t *r1 = type == MV_BACKWARD ? F.future + (size_t) (b + 1) * npix + (size_t) (y0 + by) * W + (x0 + bx)
                                                        : F.past + (size_t) (b + 1) * npix + (size_t) (y0 + fy) * W + (x0 + fx);
                const int16_t *r2 = type == MV_INTERPOLATED ? F.future + (size_t) (b + 1) * npix + (size_t) (y0 + by) * W + (x0 + bx) : r1;
                for (int i = tid; i < bw * bh; i += B) {
                    const size_t p = (size_t) (i / bw) * W + (i % bw);
                    o[p] = (int16_t) (o[p] - (type == MV_INTERPOLATED ? ((int) r1[p] + (int) r2[p]) / 2 : (int) r1[p]));
                }
            }
        }
}

/* a0 = level of the range, a1 = its address in the block; the frame on top of the stack holds
 * the DC weight (nd_w).  States [fr.states, fr.rec_states) are the ones the subdivision made. */
__device__ __noinline__ void op_pred_setup(DevFrame &__restrict__ F, Sh &__restrict__ sh, int level, int address)
{
    const bool mc = sh.st[sh.sp].try_pred == 2;
    const int tid = threadIdx.x, il = F.images_level;
    SFrame &fr = sh.st[sh.sp];
    const int size = 1 << level, npx = 1 << F.lc_max;
    /* block pixels and norms aside */
    for (int i = tid; i < npx; i += B) F.pix_save[i] = sh.pixels[i];
    for (int i = tid; i < FC_PIXELS / 32; i += B) F.pix_save[FC_PIXELS + i] = sh.norms[i];
    /* automaton rows of the displaced states aside (store_state_data) */
    for (int s = fr.states + tid; s < fr.rec_states; s += B) {
        FcSavedRow &r = F.sv_auto[s - fr.states];
        for (int l = 0; l < 2; l++) {
            r.tree[l] = TREE(F, s, l);
            r.x[l] = F.x[l * F.PA + s]; r.y[l] = F.y[l * F.PA + s];
            r.ycol[l] = F.color ? F.ycol[l * F.PA + s] : 0;
            for (int e = 0; e < 6; e++) { r.into[l][e] = INTO(F, s, l, e); r.weight[l][e] = WEIGHT(F, s, l, e); }
        }
        r.final_d = F.final_d[s]; r.level = F.level_of_state[s]; r.dtype = F.domain_type[s];
        r.pos = F.pos[s]; r.tables = 0;
        if (F.frame_type)
            for (int l = 0; l < 2; l++)
                for (int k = 0; k < 5; k++) r.mv[l][k] = F.mv[(k * 2 + l) * F.PA + s];
    }
    /* residual: range pixels + w, w = - weight * <image of state 0 at level 0> (:417-427) */
    if (mc) {
        /* motion compensated prediction error of the range, bintree order, / 16 truncated
         * (get_mcpe + cut_to_bintree, codec/mwfa.c:610-656, codec/subdivide.c:504-541) */
        const Range &rg = fr.rg;
        const int W = F.width, type = fr.prange.mv[0];
        const int16_t *orig = F.pix16 + (size_t) rg.y * W + rg.x;
        const int16_t *r1 = type == MV_BACKWARD ? F.future + (size_t) (rg.y + fr.prange.mv[4]) * W + (rg.x + fr.prange.mv[3])
                                                : F.past + (size_t) (rg.y + fr.prange.mv[2]) * W + (rg.x + fr.prange.mv[1]);
        const int16_t *r2 = type == MV_INTERPOLATED ? F.future + (size_t) (rg.y + fr.prange.mv[4]) * W + (rg.x + fr.prange.mv[3]) : r1;
        for (int i = tid; i < size; i += B) {
            unsigned xo = 0, yo = 0;
#pragma unroll
            for (int b = 0; b < 13; b++) {
                yo |= ((i >> (2 * b)) & 1u) << b;
                xo |= ((i >> (2 * b + 1)) & 1u) << b;
            }
            const size_t o = (size_t) yo * W + xo;
            const short d = type == MV_INTERPOLATED ? (short) (orig[o] - ((int) r1[o] + (int) r2[o]) / 2)
                                                    : (short) (orig[o] - r1[o]);
            sh.pixels[i] = (float) ((int) d / 16);
        }
    } else {
        const float w = -fr.nd_w * F.img[0];
        float v[FC_PIXELS / B];
#pragma unroll
        for (int it = 0; it < FC_PIXELS / B; it++) {
            const int i = tid + it * B;
            v[it] = i < size ? sh.pixels[address * size + i] + w : 0.0f;
        }
        __syncthreads();
#pragma unroll
        for (int it = 0; it < FC_PIXELS / B; it++) {
            const int i = tid + it * B;
            if (i < size) sh.pixels[i] = v[it];
        }
    }
    if (tid == 0) {
        sh.par.ipis = F.ipis_alt; sh.par.d5 = F.d5_alt; sh.par.d4 = F.d4_alt;
        sh.pred_active = 1; sh.pred_lo = fr.states; sh.pred_rec = fr.rec_states;
        for (int i = 0; i < FC_MAXSAVE / 32; i++) sh.pred_saved[i] = 0;
    }
    swap_model_sets(sh);
    __syncthreads();
    /* tables of the residual block for every state (compute_ip_images_state(0, 0, level, 1, 0)) */
    {
        const int coopD = coop_publish(F, sh, level, 0);
        if (level > il) block_norms(sh, level, (1 << (level - il)) - 1);
        if (coopD) {
            coop_finish(F, sh, level, 0, coopD);
            op_ipis(F, sh, 0, 0, level, 0, level - coopD + 1);
            return;
        }
    }
    op_d5(F, sh, 0, table_states(sh), level >= il ? 1 << (level - il) : 0, level >= il - 1 ? 1 << (level - il + 1) : 0);
    __syncthreads();
    if (level > il) op_ipis(F, sh, 0, 0, level, 0);
}

/* copy-on-write of the table rows of a displaced state id (called by all lanes from op_append) */
__device__ void pred_save_tables(DevFrame &__restrict__ F, Sh &__restrict__ sh, int s)
{
    const int tid = threadIdx.x, P = F.P, idx = s - sh.pred_lo;
    if (!sh.pred_active || s < sh.pred_lo || s >= sh.pred_rec || idx >= F.max_save) return;   /* uniform */
    if ((sh.pred_saved[idx >> 5] >> (idx & 31)) & 1u) return;
    if (!F.sv_auto[idx].dtype) return;                 /* the displaced state had no tables */
    for (int q = 0; q < F.NL; q++) {
        const float *G = GRAM(F, q) + GROW(s, P);
        float *dst = F.sv_gram + ((size_t) idx * F.NL + q) * P;
        for (int t = tid; t <= s; t += B) dst[t] = G[t];
    }
    {
        float *dst = F.sv_img + (size_t) idx * (F.NI + 48 + F.NL);
        for (int i = tid; i < F.NI; i += B) dst[i] = F.img[(size_t) s * F.NI + i];
        if (tid < 32) dst[F.NI + tid] = F.imgT[(size_t) tid * P + s];
        else if (tid < 48 && F.gl0 < F.images_level) dst[F.NI + tid] = F.imgT4[(size_t) (tid - 32) * P + s];
        else if (tid >= 64 && tid < 64 + F.NL) dst[F.NI + 48 + tid - 64] = F.diag[(size_t) (tid - 64) * P + s];
    }
    __syncthreads();
    if (tid == 0) { sh.pred_saved[idx >> 5] |= 1u << (idx & 31); F.sv_auto[idx].tables = 1; }
    __syncthreads();
}

/* a0 = the prediction is kept */
__device__ __noinline__ void op_pred_finish(DevFrame &__restrict__ F, Sh &__restrict__ sh, int keep)
{
    const int tid = threadIdx.x, P = F.P;
    SFrame &fr = sh.st[sh.sp];
    const int npx = 1 << F.lc_max;
    const int new_states = sh.states;           /* states of the residual search */
    swap_model_sets(sh);
    for (int i = tid; i < npx; i += B) sh.pixels[i] = F.pix_save[i];
    for (int i = tid; i < FC_PIXELS / 32; i += B) sh.norms[i] = F.pix_save[FC_PIXELS + i];
    if (tid == 0) {
        sh.par.ipis = F.ipis; sh.par.d5 = F.d5; sh.par.d4 = F.d4;
        sh.pred_active = 0;
    }
    __syncthreads();
    if (keep) {
        /* the delta pool saw every append; the normal pool holds the same list */
#if !FC_GM              /* (generic models: both pools were offered every state, each by its own rule -- gm_offer) */
        if (tid == 0) { sh.pool.n = sh.dpool.n; }
#endif
        /* rows of the new states in the block's tables: zero (:342-345,481-484); their level-5
         * dots with the block are what later table updates start from */
        for (int s = fr.states + tid; s < new_states; s += B)
            if (F.domain_type[s])
                for (int slot = 0; slot < F.NS; slot++) F.ipis[(size_t) slot * P + s] = 0.0f;
        op_d5(F, sh, fr.states, new_states, F.NA, 2 * F.NA);
    } else {
        /* restore_state_data (:567-625) */
        for (int s = fr.states + tid; s < fr.rec_states; s += B) {
            const FcSavedRow &r = F.sv_auto[s - fr.states];
            for (int l = 0; l < 2; l++) {
                TREE(F, s, l) = r.tree[l];
                F.x[l * F.PA + s] = r.x[l]; F.y[l * F.PA + s] = r.y[l];
                if (F.color) F.ycol[l * F.PA + s] = r.ycol[l];
                for (int e = 0; e < 6; e++) { INTO(F, s, l, e) = r.into[l][e]; WEIGHT(F, s, l, e) = r.weight[l][e]; }
            }
            F.final_d[s] = r.final_d; F.level_of_state[s] = r.level; F.domain_type[s] = r.dtype;
            F.pos[s] = r.pos;
            if (r.pos >= 0) F.pool_states[r.pos] = (short) s;
            if (F.frame_type)
                for (int l = 0; l < 2; l++)
                    for (int k = 0; k < 5; k++) F.mv[(k * 2 + l) * F.PA + s] = r.mv[l][k];
        }
        for (int idx = 0; idx < fr.rec_states - fr.states && idx < F.max_save; idx++) {
            if (!((sh.pred_saved[idx >> 5] >> (idx & 31)) & 1u)) continue;      /* uniform */
            const int s = fr.states + idx;
            for (int q = 0; q < F.NL; q++) {
                float *G = GRAM(F, q) + GROW(s, P);
                const float *src = F.sv_gram + ((size_t) idx * F.NL + q) * P;
                for (int t = tid; t <= s; t += B) G[t] = src[t];
            }
            const float *src = F.sv_img + (size_t) idx * (F.NI + 48 + F.NL);
            for (int i = tid; i < F.NI; i += B) F.img[(size_t) s * F.NI + i] = src[i];
            if (tid < 32) F.imgT[(size_t) tid * P + s] = src[F.NI + tid];
            else if (tid < 48 && F.gl0 < F.images_level) F.imgT4[(size_t) (tid - 32) * P + s] = src[F.NI + tid];
            else if (tid >= 64 && tid < 64 + F.NL) F.diag[(size_t) (tid - 64) * P + s] = src[F.NI + 48 + tid - 64];
        }
    }
}
#endif
