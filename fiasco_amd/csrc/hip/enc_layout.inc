/*
 *  enc_layout.inc -- what a frame needs of the device (included by core_hip.cpp): the predicates that route it to a
 *  kernel build, the layout of its slab (Layout, make_layout: frame_coder.h names the arrays) and what the device
 *  coder refuses (device_supported).
 */

/* A basis the rows inside DevFrame cannot hold: more than FC_MAXBASIS states, or a label with more than
 * MAXEDGES edges (data/medium.fco, large.fco: the reference's append_edge runs on into the next row,
 * fa_wfa_append_edge).  It travels as the memory image of its rows (DevFrame.bx); big kernel builds only. */
static bool long_basis(const fa_wfa *w)
{
    if (!w) return false;
    if (w->basis_states > FC_MAXBASIS) return true;
    for (unsigned s = 0; s < w->basis_states; s++)
        for (unsigned l = 0; l < 2; l++) {
            unsigned e = 0;
            while (e < 6 && FA_INTO(w, s, l, e) != FA_NO_EDGE) e++;
            if (e > FA_MAXEDGES) return true;
        }
    return false;
}
static size_t bx_bytes(const fa_wfa *w) { return 16 + (size_t) w->basis_states * 80 + 72; }

/* RPF mantissas of more than 5 bits (cfiasco --rpf-mantissa / --dc-rpf-mantissa 6 .. 8): the FC_HM build */
static bool needs_hm_variant(const fa_cparams *cp)
{
    return cp->rpf.mantissa_bits > 5 || cp->dc_rpf.mantissa_bits > 5 || cp->d_rpf.mantissa_bits > 5 || cp->d_dc_rpf.mantissa_bits > 5;
}

/* models other than the `rle' pools and the `adaptive' coefficients that fiasco.h can ask for
 * (fiasco_amd_c_options_set_models; the delta set counts when it is used: prediction, P / B frames): the FC_GM build */
static bool needs_gm_variant(const fa_job *job)
{
    const fa_cparams *cp = &job->cp;
    const bool delta_used = cp->prediction || job->frame_type != FA_I_FRAME;
    return cp->pool_kind != FA_POOL_RLE || cp->coeff_kind != FA_COEFF_ADAPTIVE
           || (delta_used && (cp->d_pool_kind != FA_POOL_RLE || cp->d_coeff_kind != FA_COEFF_ADAPTIVE));
}

/* the default builds cover the CLI's -z 0 geometry, the big ones block levels 4..12, up to 5 vectors and the
 * second-domain retry */
static bool needs_big_variant(const fa_cparams *cp, const fa_wfa *basis)
{
    if (needs_hm_variant(cp)) return true;
    if (cp->prediction) return true;         /* second model set, residual search: big build only */
    if (long_basis(basis)) return true;
    /* the default build reads 3 edge slots per label (fc_config.inc FC_MAXE): a basis file
     * whose states have more goes to the big build */
    if (basis)
        for (unsigned s = 0; s < basis->basis_states; s++)
            for (unsigned l = 0; l < 2; l++)
                for (unsigned e = 0; e < 6 && FA_INTO(basis, s, l, e) != FA_NO_EDGE; e++)
                    if (e >= 3) return true;
    unsigned dcs = 1u << (1 + cp->dc_rpf.mantissa_bits), sy = 1u << (1 + cp->rpf.mantissa_bits);
    return cp->lc_min_level <= cp->images_level || cp->lc_max_level > 10 || cp->max_elements > 3
           || cp->second_domain_block || cp->check_for_underflow || cp->check_for_overflow || cp->full_search
           || (cp->lc_max_level - cp->lc_min_level + 1) * sy + dcs > FC_MAXCOEFF
           /* aac snapshots beyond the default build's LDS pool (fc_lds.inc SNAP_POOL16; one per
            * depth + one per block level with children): the big build parks them in HBM */
           || (cp->level - cp->lc_min_level + 3 + cp->lc_max_level - cp->lc_min_level)
              * ((32 + 2 * ((cp->lc_max_level - cp->lc_min_level + 1) * sy + dcs) + 15) / 16) > FC_SNAP16_WIDE;
}

/* The 256-thread default build keeps a shorter stack and smaller snapshot pools in LDS than the
 * wide one (frame_coder.h: FC_MAXDEPTH_NARROW, FC_SNAP16_NARROW, FC_SNAPTM_NARROW -- sized
 * for what the stock reference accepts, level <= 22); a frame beyond them is given to the
 * wide build whatever the size of the launch. */
static bool needs_wide_variant(const fa_cparams *cp)
{
    unsigned dcs = 1u << (1 + cp->dc_rpf.mantissa_bits), sy = 1u << (1 + cp->rpf.mantissa_bits);
    const unsigned n16 = (32 + 2 * ((cp->lc_max_level - cp->lc_min_level + 1) * sy + dcs) + 15) / 16;
    const unsigned depths = cp->level - cp->lc_min_level + 3;
    return depths - 1 > FC_MAXDEPTH_NARROW
           || (depths + cp->lc_max_level - cp->lc_min_level) * n16 > FC_SNAP16_NARROW
           || depths * 4 * ((2 * cp->limit_level + 3) / 4) > FC_SNAPTM_NARROW;
}

/* ------------------------------------------------------------------ layout */

struct Layout {
    size_t gram, gcol, diag, ipis, d5, ipt, d4, img, imgT, imgT4, norms, num, den, est, ipdo, used, tree, into, weight,
           final_d, level_of_state, domain_type, x, y, ycol, pool_states, pos, hits, ycol0, snap, pix16, total;
    size_t ipis_alt, d5_alt, d4_alt, pix_save, sv_gram, sv_img, sv_auto;   /* prediction only */
    size_t mv, past, future, mc_fwd, mc_bwd, pix_chroma;                    /* P frames only */
    size_t coop;                                                            /* FcCoop: header + the block's pixels */
    size_t bx;                                                              /* DevFrame.bx: rows of a long basis */
    size_t gq, lginv;                                                       /* FC_GM build: DevFrame.gq, DevFrame.lginv */
    int    max_save;
};

/* P: capacity for states with tables; PA >= P: capacity of the automaton arrays (chroma
 * states of a colour frame never own tables) */
static Layout make_layout(int P, int PA, int NL, int NS, int NA, int NI, int il, int low, size_t npix,
                          int max_save, int inter, int plevels, int color, bool tri, bool hm, int gm_states = 0)
{
    Layout L;
    memset(&L, 0, sizeof L);             /* compared with memcmp (frame queue) */
    size_t o = 0;
    L.max_save = max_save;
#define CARVE(field, bytes) do { L.field = o; o = align_up(o + (bytes), 256); } while (0)
    /* Gram tables: full symmetric, or (tri) the lower triangle with packed rows + a row of slack */
    CARVE(gram, tri ? (size_t) NL * ((size_t) P * (P + 1) / 2 + P) * 4 : (size_t) NL * P * P * 4);
    CARVE(gcol, tri ? (size_t) NL * FC_TRI_HOT * P * 4 : 0);      /* columns of the first states as rows (frame_coder.h) */
    CARVE(diag, (size_t) NL * P * 4);
    CARVE(ipis, (size_t) NS * P * 4);
    CARVE(d5, (size_t) NA * P * 4);
    CARVE(ipt, (size_t) NA * P * 4);                 /* NA floats per state, one table per level (ipt_layout.h) */
    CARVE(d4, low ? (size_t) 2 * NA * P * 4 : 0);
    CARVE(img, (size_t) P * NI * 4);
    CARVE(imgT, ((size_t) 1 << il) * P * 4);
    CARVE(imgT4, low ? ((size_t) 1 << (il - 1)) * P * 4 : 0);
    CARVE(norms, (size_t) NS * 4);
    CARVE(num, (size_t) P * 4);
    CARVE(den, (size_t) P * 4);
    CARVE(est, (size_t) P * 4);
    CARVE(ipdo, (size_t) FC_MAXED * P * 4);
    CARVE(used, (size_t) P);
    /* tree .. y are downloaded with ONE copy: keep them adjacent */
    CARVE(tree, (size_t) 2 * PA * 2);
    CARVE(into, (size_t) 12 * PA * 2);
    CARVE(weight, (size_t) 12 * PA * 4);
    CARVE(final_d, (size_t) PA * 4);
    CARVE(level_of_state, (size_t) PA);
    CARVE(domain_type, (size_t) PA);
    CARVE(x, (size_t) 2 * PA * 2);
    CARVE(y, (size_t) 2 * PA * 2);
    CARVE(ycol, (size_t) 2 * PA);
    CARVE(mv, inter ? (size_t) 10 * PA * 2 : 0);     /* downloaded with the automaton */
    CARVE(pool_states, (size_t) (P + 8) * 2);
    CARVE(pos, (size_t) (PA + 8) * 2);
    CARVE(hits, (size_t) (PA + 8) * 4);
    CARVE(ycol0, (size_t) 2 * PA);                   /* initial y_column flags (colour streams) */
    /* model snapshots of the big build: aac [depth][slots][n16] x 16 bytes, with prediction 5
     * slots per depth and the tree-model snapshots [depth][2][28] behind them */
    const size_t n16max = FC_N16(hm ? FC_MAXCOEFF_HM : FC_MAXCOEFF_BIG_STD);        /* the kernel build's FC_N16MAX */
    CARVE(snap, max_save ? (size_t) (FC_MAXDEPTH_BIG * 5 * n16max + FC_MAXDEPTH_BIG * 2 * 28) * 16
                         : (size_t) 26 * 2 * n16max * 16);
    /* prediction: second table set for residual blocks, block pixels + norms, displaced rows */
    CARVE(ipis_alt, max_save ? (size_t) NS * P * 4 : 0);
    CARVE(d5_alt, max_save ? (size_t) NA * P * 4 : 0);
    CARVE(d4_alt, max_save && low ? (size_t) 2 * NA * P * 4 : 0);
    CARVE(pix_save, max_save ? (size_t) (4096 + 128) * 4 : 0);
    CARVE(sv_gram, (size_t) max_save * NL * P * 4);
    CARVE(sv_img, (size_t) max_save * (NI + 48 + NL) * 4);
    CARVE(sv_auto, (size_t) max_save * sizeof(FcSavedRow));
    /* P frames: reference frame planes, displacement cost tables, private chroma planes */
    CARVE(past, inter ? npix * 2 : 0);
    CARVE(future, inter == 2 ? npix * 2 : 0);
    CARVE(mc_fwd, inter ? (size_t) plevels * 1024 * 4 : 0);
    CARVE(mc_bwd, inter ? (size_t) plevels * 1024 * 4 : 0);
    CARVE(pix_chroma, inter && color ? npix / 3 * 2 * 2 : 0);
    CARVE(coop, FC_COOP_HDR + ((size_t) (NS + 1) << il) * 4);
    CARVE(bx, FC_BX_BYTES);
    CARVE(gq, gm_states ? (size_t) FC_GQ_SLOTS * P * 2 : 0);
    CARVE(lginv, gm_states ? ((size_t) gm_states + 2) * 8 : 0);
    CARVE(pix16, npix * 2);
#undef CARVE
    L.total = o;
    return L;
}

static int device_supported(const fa_job *job, char *why, size_t n)
{
    const fa_cparams *cp = &job->cp;
    /* a P / B frame whose reference frame is missing (e.g. an I frame coded between a B frame and its past reference:
     * the reference coder drops both references at an I frame, codec/coder.c:580-628, and dereferences a null frame at
     * its first motion search) -- IF a motion search can happen: the searches run on ranges of the prediction window
     * (codec/prediction.c:96-208), and a minimum block level that a colour frame has ratcheted above the window's top
     * (codec/coder.c:785-797) leaves no such range.  The reference then codes the frame without ever looking at the
     * missing frame, and so does the device (tests/test_gpu_fuzz_reference.py, seed 71136: pattern `ipb', 4 frames). */
    const bool window_reachable = (int) cp->p_max_level >= (int) cp->lc_min_level;
    if (job->frame_type != FA_I_FRAME && window_reachable
        && (!job->past || (job->frame_type == FA_B_FRAME && !job->future) || cp->search_range != 16)) {
        snprintf(why, n, "Motion search without a reference frame (frame pattern).");
        return 0;
    }
    /* (signed: after a colour frame the minimum block level may have been ratcheted ABOVE the prediction window --
     * codec/coder.c:785-797 -- which then holds no level at all; found by tests/test_gpu_fuzz_reference.py, seed 71064:
     * the unsigned difference refused a P frame the reference codes) */
    if ((cp->prediction || job->frame_type != FA_I_FRAME) && (int) cp->p_max_level - (int) cp->lc_min_level + 1 > 9) {
        snprintf(why, n, "prediction over more than 9 block levels is not supported by the device coder (levels %u .. %u, frame type %d)",
                 cp->lc_min_level, cp->p_max_level, job->frame_type);
        return 0;
    }
    if (cp->images_level != 5 || cp->lc_min_level < 4) {
        snprintf(why, n, "device coder needs images_level 5 and min block level >= 4");
        return 0;
    }
    if (cp->lc_max_level > 12) { snprintf(why, n, "max block level > 12 is not supported by the device coder"); return 0; }
    if (cp->max_elements > 5) { snprintf(why, n, "more than 5 vectors per block are not supported by the device coder"); return 0; }
    {
        unsigned dcs = 1u << (1 + cp->dc_rpf.mantissa_bits), sy = 1u << (1 + cp->rpf.mantissa_bits);
        if ((cp->lc_max_level - cp->lc_min_level + 1) * sy + dcs > FC_MAXCOEFF_HM) {
            snprintf(why, n, "coefficient model too large for the device coder "
                             "(block levels x mantissa symbols > %d)", FC_MAXCOEFF_HM);
            return 0;
        }
    }
    if (cp->rpf.mantissa_bits > 8 || cp->dc_rpf.mantissa_bits > 8 || cp->d_rpf.mantissa_bits > 8 || cp->d_dc_rpf.mantissa_bits > 8) {
        snprintf(why, n, "RPF mantissa > 8 bits is not supported by the device coder");      /* (alloc_rpf never makes one) */
        return 0;
    }
    if (long_basis(job->wfa)) {
        const fa_wfa *w = job->wfa;
        if (bx_bytes(w) > FC_BX_BYTES) { snprintf(why, n, "initial basis too large for the device coder"); return 0; }
        /* every edge list must end inside the rows of the basis (the device takes a copy of those rows; a list that
         * ran on into the rows of the coder's own states would change while the frame is coded) */
        for (unsigned r = 0; r < w->basis_states * 2; r++) {
            unsigned e = r * 6;
            while (e < w->basis_states * 12 && w->into[e] != FA_NO_EDGE) e++;
            if (e >= w->basis_states * 12) { snprintf(why, n, "edge lists of the initial basis run on into the coder's states"); return 0; }
        }
    }
    /* (every entry of the reference's model registries runs on the device since round 5: the `rle' pools and the
     * `adaptive' coefficients of fiasco.h in the fast builds, the others in the FC_GM build) */
    return 1;
}
