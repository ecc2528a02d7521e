/*
 *  fa_reader.c -- .fco stream reader: the inverse of fa_writer.c, section by section.
 *
 *  What the sections hold follows the reference's reader:
 *    header           input/read.c:57-217
 *    frame            input/read.c:344-451
 *    tree             input/tree.c:52-301        (binary adaptive arithmetic decoder, breadth first -> depth first)
 *    matrices         input/matrices.c:53-642    (column 0 QAC, #edges AC, index bin codes, chroma QAC columns)
 *    weights          input/weights.c:37-199     + lib/arith.c:474-587 (decode_array)
 *    interval rescale lib/arith.h:67-91
 *    nd               input/nd.c:49-237
 *    mc               input/mc.c:80-280
 *
 *  A stream is untrusted: every read is checked against the buffer (fa_bitio.c), every symbol against its alphabet,
 *  and every index a decoder will follow -- tree, into, levels, coordinates, vectors -- is either made here from
 *  checked values or checked before it is stored.  A frame that fails gives NULL and a message.
 */
#include <stdlib.h>
#include <string.h>
#include "fa_host.h"

/* ------------------------------------------------------------ 16-bit interval decoder */

typedef struct ad16 {
    uint16_t low, high, code;
    fa_bitr *in;
} ad16;

static void ad_init(ad16 *a, fa_bitr *in)
{
    a->low = 0; a->high = 0xffff; a->in = in;
    a->code = (uint16_t) fa_br_get_bits(in, 16);
}

/* drop settled leading bits and underflow bits, one new bit of the stream for each (lib/arith.h:67-91) */
static void ad_rescale(ad16 *a)
{
    for (;;) {
        if (a->high < 0x8000 || a->low >= 0x8000) {
            /* nothing to undo */
        } else if (a->high < 0xc000 && a->low >= 0x4000) {
            a->code ^= 0x4000;
            a->low  &= 0x3fff;
            a->high |= 0x4000;
        } else
            break;
        a->low  = (uint16_t) (a->low << 1);
        a->high = (uint16_t) ((a->high << 1) | 1);
        a->code = (uint16_t) ((a->code << 1) | fa_br_get_bit(a->in));
        if (a->in->over) break;                /* the caller refuses: no endless walk behind the end */
    }
}

/* where the code lies in [0, scale); scale for a code that left its interval (a stream no coder wrote) */
static unsigned ad_count(const ad16 *a, unsigned scale)
{
    const unsigned range = (unsigned) (a->high - a->low) + 1;
    if (a->code < a->low || a->code > a->high) return scale;
    return (((unsigned) (a->code - a->low) + 1) * scale - 1) / range;
}

/* narrow to the sub-interval [lo_c, hi_c) / scale: ac_encode of the writer */
static void ad_narrow(ad16 *a, unsigned lo_c, unsigned hi_c, unsigned scale)
{
    const unsigned range = (unsigned) (a->high - a->low) + 1;
    const uint16_t base = a->low;
    a->high = (uint16_t) (base + (uint16_t) ((range * hi_c) / scale - 1));
    a->low  = (uint16_t) (base + (uint16_t) ((range * lo_c) / scale));
    ad_rescale(a);
}

/* one decision of the binary adaptive model of the tree and the nd tree (sum0 of sum1 for '0') */
static unsigned ad_binary(ad16 *a, unsigned *sum0, unsigned *sum1, unsigned scaling)
{
    const unsigned count = ad_count(a, *sum1);
    unsigned bit;
    if (count < *sum0) { ad_narrow(a, 0, *sum0, *sum1); *sum0 = (uint16_t) (*sum0 + 1); bit = 0; }
    else { ad_narrow(a, *sum0, *sum1, *sum1); bit = 1; }
    *sum1 = (uint16_t) (*sum1 + 1);
    if (*sum1 > scaling) {
        *sum0 >>= 1; *sum1 >>= 1;
        if (!*sum0) *sum0 = 1;
        if (*sum0 >= *sum1) *sum1 = *sum0 + 1;
    }
    return bit;
}

/* the quasi-arithmetic binary decoder with shift probabilities (qac_put of the writer) */
typedef struct qad {
    ad16 ad;
    unsigned index;
} qad;

static unsigned qad_shift(unsigned index)
{
    unsigned n = 1, start = 0;
    while (index >= start + (1u << n)) { start += 1u << n; n++; }
    return n;
}

static int qad_get(qad *q)
{
    ad16 *a = &q->ad;
    const unsigned count = (unsigned) a->high - (((unsigned) a->high - a->low) >> qad_shift(q->index));
    if (a->code < count) {
        a->high = (uint16_t) (count - 1);
        ad_rescale(a);
        if (q->index < 1020) q->index++;
        return 0;
    }
    a->low = (uint16_t) count;
    ad_rescale(a);
    q->index >>= 1;
    return 1;
}

static unsigned ilog2u(unsigned v) { unsigned k = 0; while (v >>= 1) k++; return k; }

/* an edge of a state of the frame: never more than FA_MAXEDGES on a label, never twice into one state */
static int add_edge(fa_wfa *wfa, unsigned from, unsigned into, unsigned label)
{
    unsigned e;
    if (into >= wfa->states) { fa_set_error("Stream error: an edge of state %u leads to state %u of %u.", from, into, wfa->states); return 0; }
    for (e = 0; FA_INTO(wfa, from, label, e) != FA_NO_EDGE; e++)
        if ((unsigned) FA_INTO(wfa, from, label, e) == into) {
            fa_set_error("Stream error: two edges of state %u, label %u lead to state %u.", from, label, into);
            return 0;
        }
    if (e >= FA_MAXEDGES) { fa_set_error("Stream error: more than %d edges at state %u, label %u.", FA_MAXEDGES, from, label); return 0; }
    if (!fa_wfa_append_edge(wfa, from, into, -1.0f, label)) { fa_set_error("Stream error: no room for an edge of state %u.", from); return 0; }
    return 1;
}

static int truncated(const fa_bitr *in, const char *what)
{
    if (!in->over) return 0;
    fa_set_error("Can't read next bit from the stream: it is truncated (%s).", what);
    return 1;
}

/* ------------------------------------------------------------ header */

static char *get_string(fa_bitr *in)
{
    char buf[1024];
    unsigned n = 0;
    for (;;) {
        const unsigned c = fa_br_get_bits(in, 8);
        if (in->over || n >= sizeof buf - 1) return NULL;
        buf[n++] = (char) c;
        if (!c) break;
    }
    return strdup(buf);
}

static int get_rpf(fa_bitr *in, fa_rpf *r)
{
    const unsigned mantissa = fa_br_get_bits(in, 3) + 2, range = fa_br_get_bits(in, 2);
    if (mantissa > 8) { fa_set_error("Stream error: a mantissa of %u bits is outside the interval [2,8].", mantissa); return 0; }
    fa_rpf_init(r, mantissa, (int) range);
    return 1;
}

int fa_read_header(fa_bitr *in, const char *name, fa_info *wi)
{
    const unsigned k = 8;
    const char *p;
    unsigned release, type, max_states, max_level;
    memset(wi, 0, sizeof *wi);
    for (p = "FIASCO"; *p; p++)
        if (fa_br_get_bits(in, 8) != (unsigned char) *p || in->over) {
            fa_set_error("Input file %s is not a valid FIASCO file!", name);
            return 0;
        }
    (void) fa_br_get_bits(in, 8);                           /* the newline */
    if (!(wi->basis_name = get_string(in))) {
        if (!truncated(in, "header")) fa_set_error("Input file %s is not a valid FIASCO file!", name);
        return 0;
    }
    release = fa_br_rice(in, k);
    if (truncated(in, "header")) goto bad;
    if (release != 2) {
        if (release > 2)
            fa_set_error("Can't decode FIASCO files of file format release `%d'.\nCurrent file format release is `%d'.", (int) release, 2);
        else
            fa_set_error("Can't decode FIASCO files of file format release `%d': only release `%d' is read.", (int) release, 2);
        goto bad;
    }
    while ((type = fa_br_rice(in, k)) != 0) {               /* HEADER_END */
        char **slot = type == 1 ? &wi->title : type == 2 ? &wi->comment : NULL;
        if (truncated(in, "header")) goto bad;
        if (!slot) { fa_set_error("Stream error: header item of unknown type %u.", type); goto bad; }
        free(*slot);
        if (!(*slot = get_string(in))) {
            if (!truncated(in, "header")) fa_set_error("Stream error: a header string of more than 1022 characters.");
            goto bad;
        }
    }
    wi->max_states = fa_br_rice(in, k);
    wi->color      = (int) fa_br_get_bit(in);
    wi->width      = fa_br_rice(in, k);
    wi->height     = fa_br_rice(in, k);
    if (wi->color) wi->chroma_max_states = fa_br_rice(in, k);
    wi->p_min_level = fa_br_rice(in, k);
    wi->p_max_level = fa_br_rice(in, k);
    wi->frames      = fa_br_rice(in, k);
    wi->smoothing   = fa_br_rice(in, k);
    if (truncated(in, "header")) goto bad;
    if (!get_rpf(in, &wi->rpf)) goto bad;
    if (fa_br_get_bit(in)) { if (!get_rpf(in, &wi->dc_rpf)) goto bad; } else wi->dc_rpf = wi->rpf;
    if (fa_br_get_bit(in)) { if (!get_rpf(in, &wi->d_rpf)) goto bad; } else wi->d_rpf = wi->rpf;
    if (fa_br_get_bit(in)) { if (!get_rpf(in, &wi->d_dc_rpf)) goto bad; } else wi->d_dc_rpf = wi->dc_rpf;
    if (wi->frames > 1) {
        wi->fps           = fa_br_rice(in, k);
        wi->search_range  = fa_br_rice(in, k);
        wi->half_pixel    = (int) fa_br_get_bit(in);
        wi->B_as_past_ref = (int) fa_br_get_bit(in);
    }
    fa_br_align(in);
    if (truncated(in, "header")) goto bad;
    /* what the frames are checked against */
    fa_limits(&max_states, &max_level);
    if (wi->width < 2 || wi->height < 2 || wi->width > (1u << (FA_CAP_LEVEL / 2)) || wi->height > (1u << (FA_CAP_LEVEL / 2))) {
        fa_set_error("Stream error: a frame of %u x %u pixels (2 .. %u a side).", wi->width, wi->height, 1u << (FA_CAP_LEVEL / 2));
        goto bad;
    }
    {
        const unsigned lx = ilog2u(wi->width - 1) + 1, ly = ilog2u(wi->height - 1) + 1, m = lx > ly ? lx : ly;
        wi->level = m * 2 - (ly == lx + 1 ? 1 : 0);
    }
    if (wi->level > max_level) {
        fa_set_error("Image level %d exceeds MAXLEVEL %d (use fiasco_amd_set_limits).", (int) wi->level, (int) max_level);
        goto bad;
    }
    if (!wi->frames) { fa_set_error("Stream error: a stream of 0 frames."); goto bad; }
    if (wi->p_min_level > wi->p_max_level || wi->p_max_level > wi->level) {
        fa_set_error("Stream error: prediction levels %u .. %u of a frame of level %u.", wi->p_min_level, wi->p_max_level, wi->level);
        goto bad;
    }
    if (wi->frames > 1 && (wi->search_range < 1 || wi->search_range > 16)) {
        fa_set_error("Stream error: a search range of %u pixels (1 .. 16).", wi->search_range);
        goto bad;
    }
    return 1;
bad:
    fa_info_free(wi);
    return 0;
}

/* ------------------------------------------------------------ tree */

typedef struct tree_walk {
    fa_wfa *wfa;
    const fa_info *wi;
    const int32_t *bfo;          /* [node][2]: node numbers in breadth first order, -1 = range */
    unsigned next;               /* next state in depth first order */
    int bad;
} tree_walk;

/* restore_depth_first_order (input/tree.c:116-201) without tiling: the state of node `src' and, before it, those of
 * its subtrees; x, y: where it lies in its band.  A node of level 0 cannot be divided */
static int restore_dfo(tree_walk *t, unsigned src, unsigned level, unsigned x, unsigned y)
{
    unsigned newx[2], newy[2], label, state;
    int child[2];
    if (level == 0) { t->bad = 1; return FA_RANGE; }
    if (t->wi->color && level == t->wi->level + 1)
        newx[0] = newy[0] = newx[1] = newy[1] = 0;
    else {
        newx[0] = x; newy[0] = y;
        newx[1] = (level & 1) ? x : x + fa_width_of_level(level - 1);
        newy[1] = (level & 1) ? y + fa_height_of_level(level - 1) : y;
    }
    for (label = 0; label < 2; label++) {
        const int32_t node = t->bfo[src * 2 + label];
        child[label] = node < 0 ? FA_RANGE : restore_dfo(t, (unsigned) node, level - 1, newx[label], newy[label]);
        if (t->bad) return FA_RANGE;
    }
    state = t->next++;
    for (label = 0; label < 2; label++) {
        FA_TREE(t->wfa, state, label) = (int16_t) child[label];
        t->wfa->x[state * 2 + label] = (uint16_t) newx[label];
        t->wfa->y[state * 2 + label] = (uint16_t) newy[label];
    }
    t->wfa->level_of_state[state] = (uint8_t) level;
    return (int) state;
}

static int read_tree(fa_wfa *wfa, const fa_info *wi, fa_bitr *in)
{
    const unsigned nodes = wfa->states - wfa->basis_states, total = nodes * 2, scaling = total / 20;
    int32_t *bfo = (int32_t *) malloc(sizeof(int32_t) * ((size_t) total + 2));
    unsigned sum0 = 1, sum1 = 11, node, next = 1, label;
    tree_walk t;
    ad16 a;
    int ok = 0;
    if (!bfo) { fa_set_error("Out of memory!"); return 0; }
    ad_init(&a, in);
    /* one symbol per (node, label) in breadth first order: the nodes it makes must be the frame's states exactly */
    for (node = 0; node < next && node < nodes; node++)
        for (label = 0; label < 2; label++) {
            const unsigned bit = ad_binary(&a, &sum0, &sum1, scaling);
            if (in->over) goto out;
            bfo[node * 2 + label] = bit ? (next < nodes ? (int32_t) next : -2) : -1;
            if (bit) next++;
        }
    fa_br_align(in);
    if (next != nodes) {
        fa_set_error("Stream error: the bintree has %s nodes than the frame has states.", next > nodes ? "more" : "fewer");
        goto out0;
    }
    t.wfa = wfa; t.wi = wi; t.bfo = bfo; t.next = wfa->basis_states; t.bad = 0;
    wfa->root_state = (unsigned) restore_dfo(&t, 0, wi->level + (wi->color ? 2u : 0u), 0, 0);
    if (t.bad || t.next != wfa->states) { fa_set_error("Stream error: the bintree divides a range of level 0."); goto out0; }
    if (wi->color) {
        /* the three states that join the bands */
        const int r0 = FA_TREE(wfa, wfa->root_state, 0), r1 = FA_TREE(wfa, wfa->root_state, 1);
        if (r0 == FA_RANGE || r1 == FA_RANGE || FA_TREE(wfa, (unsigned) r0, 0) == FA_RANGE || FA_TREE(wfa, (unsigned) r0, 1) == FA_RANGE
            || FA_TREE(wfa, (unsigned) r1, 0) == FA_RANGE) {
            fa_set_error("Stream error: the bintree of a colour frame lacks a band.");
            goto out0;
        }
    }
    ok = 1;
out:
    if (!ok) (void) truncated(in, "bintree");
out0:
    free(bfo);
    return ok;
}

static unsigned y_root_of(const fa_wfa *wfa)
{
    return (unsigned) FA_TREE(wfa, (unsigned) FA_TREE(wfa, wfa->root_state, 0), 0);
}

/* ------------------------------------------------------------ decode_array (lib/arith.c:474-587) */

static int decode_array(fa_bitr *in, unsigned *data, const unsigned *context, const unsigned *c_symbols,
                        unsigned n_context, unsigned n_data, unsigned scaling, const char *what)
{
    uint16_t **totals;
    unsigned c, n, i;
    ad16 a;
    int ok = 0;
    if (!n_context) n_context = 1;
    totals = (uint16_t **) calloc(n_context, sizeof *totals);
    if (!totals) { fa_set_error("Out of memory!"); return 0; }
    for (c = 0; c < n_context; c++) {
        totals[c] = (uint16_t *) calloc(c_symbols[c] + 1, sizeof(uint16_t));
        if (!totals[c]) { fa_set_error("Out of memory!"); goto out; }
        for (i = 0; i < c_symbols[c]; i++) totals[c][i + 1] = (uint16_t) (totals[c][i] + 1);
    }
    ad_init(&a, in);
    for (n = 0; n < n_data; n++) {
        uint16_t *t;
        unsigned count, d, m;
        c = n_context > 1 ? context[n] : 0;
        t = totals[c]; m = c_symbols[c];
        count = ad_count(&a, t[m]);
        if (in->over) { (void) truncated(in, what); goto out; }
        if (count >= t[m]) { fa_set_error("Stream error: a symbol outside its alphabet (%s).", what); goto out; }
        for (d = m - 1; count < t[d]; d--)
            ;
        ad_narrow(&a, t[d], t[d + 1], t[m]);
        for (i = d + 1; i < m + 1; i++) t[i]++;
        if (t[m] > scaling)
            for (i = 1; i < m + 1; i++) {
                t[i] >>= 1;
                if (t[i] <= t[i - 1]) t[i] = (uint16_t) (t[i - 1] + 1);
            }
        data[n] = d;
    }
    fa_br_align(in);
    ok = !truncated(in, what);
out:
    for (c = 0; c < n_context; c++) free(totals[c]);
    free(totals);
    return ok;
}

/* ------------------------------------------------------------ prediction (input/nd.c) */

static int read_nd(fa_wfa *wfa, const fa_info *wi, fa_bitr *in)
{
    unsigned *queue = (unsigned *) malloc(sizeof(unsigned) * (wfa->states + 1));
    unsigned head = 0, tail = 0, total = 0, label, state, n = 0;
    unsigned sum0 = 1, sum1 = 11, c_symbols = 1u << (wi->dc_rpf.mantissa_bits + 1);
    unsigned *coeff;
    ad16 a;
    if (!queue) { fa_set_error("Out of memory!"); return 0; }
    ad_init(&a, in);
    queue[tail++] = wfa->root_state;
    while (head < tail) {
        const unsigned next = queue[head++];
        if (wfa->level_of_state[next] > wi->p_max_level + 1) {
            for (label = 0; label < 2; label++)
                if (FA_TREE(wfa, next, label) != FA_RANGE) queue[tail++] = (unsigned) FA_TREE(wfa, next, label);
        } else if (wfa->level_of_state[next] > wi->p_min_level) {
            for (label = 0; label < 2; label++) {
                const int child = FA_TREE(wfa, next, label);
                if (child == FA_RANGE) continue;
                if (ad_binary(&a, &sum0, &sum1, 50)) {                  /* '1': the child's range is predicted */
                    if (in->over || !add_edge(wfa, next, 0, label)) { free(queue); (void) truncated(in, "nd tree"); return 0; }
                    total++;
                } else if (wfa->level_of_state[child] > wi->p_min_level)
                    queue[tail++] = (unsigned) child;
                if (in->over) { free(queue); (void) truncated(in, "nd tree"); return 0; }
            }
        }
    }
    free(queue);
    fa_br_align(in);
    if (truncated(in, "nd tree")) return 0;
    if (!total) return 1;
    coeff = (unsigned *) calloc(total, sizeof(unsigned));
    if (!coeff) { fa_set_error("Out of memory!"); return 0; }
    if (!decode_array(in, coeff, NULL, &c_symbols, 1, total, 50, "nd coefficients")) { free(coeff); return 0; }
    for (state = wfa->basis_states; state < wfa->states; state++)
        for (label = 0; label < 2; label++)
            if (FA_TREE(wfa, state, label) != FA_RANGE && FA_INTO(wfa, state, label, 0) != FA_NO_EDGE && n < total)
                FA_WEIGHT(wfa, state, label, 0) = fa_btor((int) coeff[n++], &wi->dc_rpf);
    free(coeff);
    return 1;
}

/* ------------------------------------------------------------ motion compensation (input/mc.c) */

/* one vector component: the code word, bit by bit against the table; the index is component + search range */
static int get_mv(fa_bitr *in, unsigned sr, int16_t *v)
{
    unsigned code = 0, len, i;
    for (len = 1; len <= 11; len++) {
        code = (code << 1) | fa_br_get_bit(in);
        if (in->over) return truncated(in, "motion vectors"), 0;
        for (i = 0; i < 33; i++)
            if (fa_mv_code[i][1] == len && fa_mv_code[i][0] == code) {
                if (i > 2 * sr) { fa_set_error("Stream error: a motion vector outside the search range of %u pixels.", sr); return 0; }
                *v = (int16_t) ((int) i - (int) sr);
                return 1;
            }
    }
    fa_set_error("wrong huffman code !");
    return 0;
}

/* a block of bw x bh pixels at (x0, y0) moved by (mx, my) stays inside the plane the decoder addresses linearly
 * (extract_mc_block, codec/motion.c:231-261: a block may leave the frame on the right and come back on the left of the
 * next row, never leave the plane) */
static int mv_inside(const fa_info *wi, unsigned x0, unsigned y0, unsigned bw, unsigned bh, int mx, int my)
{
    const long long W = wi->width, first = ((long long) y0 + my) * W + (long long) x0 + mx;
    const long long last = first + (long long) (bh - 1) * W + (bw - 1);
    return first >= 0 && last < W * (long long) wi->height;
}

static int read_mc(int frame_type, fa_wfa *wfa, const fa_info *wi, fa_bitr *in)
{
    const unsigned max_state = wi->color ? y_root_of(wfa) : wfa->states;
    unsigned *queue = (unsigned *) malloc(sizeof(unsigned) * (wfa->states + 1));
    unsigned last = 0, cur, state, label;
    if (!queue) { fa_set_error("Out of memory!"); return 0; }
    for (state = wfa->basis_states; state < max_state; state++)
        if ((unsigned) wfa->level_of_state[state] == wi->p_max_level + 1) queue[last++] = state;
    for (cur = 0; cur < last; cur++)
        for (label = 0; label < 2; label++) {
            const unsigned lv = (unsigned) wfa->level_of_state[queue[cur]] - 1;
            int type = FA_MV_NONE;
            state = queue[cur];
            if (wfa->x[state * 2 + label] + fa_width_of_level(lv) <= wi->width
                && wfa->y[state * 2 + label] + fa_height_of_level(lv) <= wi->height) {
                if (frame_type == FA_P_FRAME) type = fa_br_get_bit(in) ? FA_MV_NONE : FA_MV_FORWARD;
                else if (fa_br_get_bit(in)) type = FA_MV_NONE;                   /* 1   */
                else if (fa_br_get_bit(in)) type = FA_MV_INTERPOLATED;           /* 01  */
                else if (fa_br_get_bit(in)) type = FA_MV_BACKWARD;               /* 001 */
                else type = FA_MV_FORWARD;                                       /* 000 */
            }
            wfa->mv[state * 2 + label].type = (int16_t) type;
            if (type == FA_MV_NONE && FA_TREE(wfa, state, label) != FA_RANGE && lv >= wi->p_min_level && lv > 0)
                queue[last++] = (unsigned) FA_TREE(wfa, state, label);
        }
    free(queue);
    fa_br_align(in);
    if (truncated(in, "motion tree")) return 0;
    for (state = wfa->basis_states; state < max_state; state++)
        for (label = 0; label < 2; label++) {
            fa_mv *mv = &wfa->mv[state * 2 + label];
            const unsigned lv = (unsigned) wfa->level_of_state[state] - 1;
            const unsigned x0 = wfa->x[state * 2 + label], y0 = wfa->y[state * 2 + label];
            const unsigned bw = fa_width_of_level(lv), bh = fa_height_of_level(lv);
            if (mv->type == FA_MV_FORWARD || mv->type == FA_MV_INTERPOLATED) {
                if (!get_mv(in, wi->search_range, &mv->fx) || !get_mv(in, wi->search_range, &mv->fy)) return 0;
                if (!wi->half_pixel && !mv_inside(wi, x0, y0, bw, bh, mv->fx, mv->fy)) goto outside;
            }
            if (mv->type == FA_MV_BACKWARD || mv->type == FA_MV_INTERPOLATED) {
                if (!get_mv(in, wi->search_range, &mv->bx) || !get_mv(in, wi->search_range, &mv->by)) return 0;
                if (!wi->half_pixel && !mv_inside(wi, x0, y0, bw, bh, mv->bx, mv->by)) goto outside;
            }
            continue;
        outside:
            fa_set_error("Stream error: the motion vector of state %u, label %u leaves the reference frame.", state, label);
            return 0;
        }
    fa_br_align(in);
    return !truncated(in, "motion vectors");
}

/* codec/wfalib.c:698-732, as the writer has it */
static void locate_delta_images(fa_wfa *wfa)
{
    int state;
    unsigned label;
    for (state = (int) wfa->root_state; state >= (int) wfa->basis_states; state--)
        wfa->delta_state[state] = 0;
    for (state = (int) wfa->root_state; state >= (int) wfa->basis_states; state--)
        for (label = 0; label < 2; label++)
            if (FA_TREE(wfa, state, label) != FA_RANGE)
                if (wfa->mv[state * 2 + label].type != FA_MV_NONE
                    || FA_INTO(wfa, state, label, 0) != FA_NO_EDGE || wfa->delta_state[state])
                    wfa->delta_state[FA_TREE(wfa, state, label)] = 1;
}

/* ------------------------------------------------------------ matrices */

typedef struct rsort {
    uint16_t *state; uint8_t *label; uint16_t *max_domain; uint8_t *subdivided;
    unsigned n;
} rsort;

/* ranges in the order the coder visited them (codec/wfalib.c:658-696) */
static void sort_ranges(unsigned state, unsigned *domain, rsort *rs, const fa_wfa *wfa)
{
    unsigned label;
    for (label = 0; label < 2; label++) {
        if (FA_TREE(wfa, state, label) == FA_RANGE)
            rs->subdivided[rs->n] = 0;
        else {
            sort_ranges((unsigned) FA_TREE(wfa, state, label), domain, rs, wfa);
            rs->subdivided[rs->n] = 1;
        }
        rs->state[rs->n] = (uint16_t) state;
        rs->label[rs->n] = (uint8_t) label;
        rs->max_domain[rs->n] = (uint16_t) *domain;
        while (!(wfa->domain_type[rs->max_domain[rs->n]] & FA_USE_DOMAIN))
            rs->max_domain[rs->n]--;
        if (label == 1 || !rs->subdivided[rs->n]) rs->n++;
    }
    (*domain)++;
}

static int column0_decoding(fa_wfa *wfa, unsigned last_row, fa_bitr *in, unsigned *total)
{
    qad q;
    unsigned row, label;
    ad_init(&q.ad, in); q.index = 0;
    for (row = wfa->basis_states; row <= last_row; row++)
        for (label = 0; label < 2; label++)
            if (FA_TREE(wfa, row, label) == FA_RANGE && qad_get(&q)) {
                if (in->over || !add_edge(wfa, row, 0, label)) return truncated(in, "column 0"), 0;
                (*total)++;
            }
    fa_br_align(in);
    return !truncated(in, "column 0");
}

static int delta_decoding(fa_wfa *wfa, unsigned last_domain, fa_bitr *in, unsigned *total, int flags[3])
{
    rsort rs;
    unsigned max_domain, nslots = (last_domain + 1) * 2, r, row = 0, n, M;
    unsigned count[FA_MAXEDGES + 1] = {0}, cum[FA_MAXEDGES + 2];
    unsigned *n_edges = NULL;
    uint16_t *map1 = NULL, *map2 = NULL, *coder1 = NULL, *coder2 = NULL;
    int ok = 0, k;
    ad16 a;
    rs.state      = (uint16_t *) calloc(nslots, sizeof(uint16_t));
    rs.label      = (uint8_t *)  calloc(nslots, 1);
    rs.max_domain = (uint16_t *) calloc(nslots, sizeof(uint16_t));
    rs.subdivided = (uint8_t *)  calloc(nslots, 1);
    rs.n = 0;
    n_edges = (unsigned *) calloc(nslots, sizeof(unsigned));
    map1 = (uint16_t *) calloc(wfa->states + 1, sizeof(uint16_t)); coder1 = (uint16_t *) calloc(wfa->states + 1, sizeof(uint16_t));
    map2 = (uint16_t *) calloc(wfa->states + 1, sizeof(uint16_t)); coder2 = (uint16_t *) calloc(wfa->states + 1, sizeof(uint16_t));
    if (!rs.state || !rs.label || !rs.max_domain || !rs.subdivided || !n_edges || !map1 || !map2 || !coder1 || !coder2) {
        fa_set_error("Out of memory!");
        goto out;
    }
    max_domain = wfa->basis_states - 1;
    sort_ranges(last_domain, &max_domain, &rs, wfa);

    /* the distribution of the number of edges, then the numbers through that static model */
    M = fa_br_rice(in, 3);
    k = (int) ilog2u(last_domain) - 2;
    if (in->over) { (void) truncated(in, "edge counts"); goto out; }
    if (M > FA_MAXEDGES || k < 0) { fa_set_error("Stream error: up to %u edges per range, %u states (at most %d, at least 4).", M, last_domain, FA_MAXEDGES); goto out; }
    for (n = 0; n <= M; n++) count[n] = fa_br_rice(in, (unsigned) k);
    cum[0] = 0;
    for (n = 1; n <= M + 1; n++) cum[n] = cum[n - 1] + count[n - 1];
    if (in->over) { (void) truncated(in, "edge counts"); goto out; }
    if (!cum[M + 1] || cum[M + 1] > 0xffff) { fa_set_error("Stream error: the edge counts of %u ranges.", cum[M + 1]); goto out; }
    ad_init(&a, in);
    for (r = 0; r < rs.n; r++)
        if (!rs.subdivided[r]) {
            const unsigned cnt = ad_count(&a, cum[M + 1]), col0 = FA_INTO(wfa, rs.state[r], rs.label[r], 0) != FA_NO_EDGE;
            unsigned e;
            if (in->over) { (void) truncated(in, "edge counts"); goto out; }
            if (cnt >= cum[M + 1]) { fa_set_error("Stream error: a symbol outside its alphabet (edge counts)."); goto out; }
            for (e = M; cnt < cum[e]; e--)
                ;
            ad_narrow(&a, cum[e], cum[e + 1], cum[M + 1]);
            if (e < col0) { fa_set_error("Stream error: state %u has an edge into state 0 and no edge at all.", (unsigned) rs.state[r]); goto out; }
            n_edges[row++] = e - col0;
        }
    fa_br_align(in);
    if (truncated(in, "edge counts")) goto out;

    /* the domains: adjusted binary codes of the distance to the last one, in the numbering of the admitted domains */
    flags[1] = (int) fa_br_get_bit(in);
    flags[2] = (int) fa_br_get_bit(in);
    {
        unsigned n1 = 0, n2 = 0, state;
        for (state = 0; state < wfa->states; state++) {
            const int usable = wfa->domain_type[state] & FA_USE_DOMAIN;
            map1[n1] = (uint16_t) state; coder1[state] = (uint16_t) n1;
            if (usable && (state < wfa->basis_states || flags[2] || !wfa->delta_state[state])) n1++;
            map2[n2] = (uint16_t) state; coder2[state] = (uint16_t) n2;
            if (usable && (state < wfa->basis_states || flags[1] || wfa->delta_state[state])) n2++;
        }
    }
    for (r = 0, row = 0; r < rs.n; r++)
        if (!rs.subdivided[r]) {
            const unsigned s = rs.state[r], l = rs.label[r];
            const int second = wfa->delta_state[s] || wfa->mv[s * 2 + l].type != FA_MV_NONE;      /* input/matrices.c:219-229 */
            const uint16_t *map = second ? map2 : map1, *coder = second ? coder2 : coder1;
            const unsigned max_value = coder[rs.max_domain[r]];
            unsigned last = 1, e;
            for (e = n_edges[row]; e; e--) {
                unsigned domain;
                if (last > max_value) { fa_set_error("Stream error: state %u has more edges than admitted domains.", s); goto out; }
                domain = max_value - last ? fa_br_bincode(in, max_value - last) + last : max_value;
                if (in->over) { (void) truncated(in, "domains"); goto out; }
                if (domain > max_value || map[domain] > rs.max_domain[r]) {
                    fa_set_error("Stream error: an edge of state %u leads to a domain behind the last one admitted.", s);
                    goto out;
                }
                if (!add_edge(wfa, s, map[domain], l)) goto out;
                last = domain + 1;
                (*total)++;
            }
            row++;
        }
    ok = 1;
out:
    free(rs.state); free(rs.label); free(rs.max_domain); free(rs.subdivided);
    free(n_edges); free(map1); free(map2); free(coder1); free(coder2);
    return ok;
}

/* compute_y_state (input/matrices.c:614-642): the states of the Y band at the place of the states of a chroma band */
static void compute_y_state(fa_wfa *wfa, int state, int y_state)
{
    unsigned label;
    for (label = 0; label < 2; label++)
        if (y_state == FA_RANGE)
            wfa->y_state[state * 2 + label] = FA_RANGE;
        else {
            wfa->y_state[state * 2 + label] = FA_TREE(wfa, y_state, label);
            if (FA_TREE(wfa, state, label) != FA_RANGE)
                compute_y_state(wfa, FA_TREE(wfa, state, label), wfa->y_state[state * 2 + label]);
        }
}

static int chroma_decoding(fa_wfa *wfa, const fa_info *wi, fa_bitr *in, unsigned *total)
{
    const unsigned y_root = y_root_of(wfa);
    int16_t *y_domains = fa_compute_hits(wfa->basis_states, y_root, wi->chroma_max_states, wfa);
    qad q;
    unsigned d, row, label, next_index = 0;
    if (!y_domains) { fa_set_error("Out of memory!"); return 0; }
    ad_init(&q.ad, in); q.index = 0;
    for (d = 0; y_domains[d] != -1; d++) {
        int save = 1;
        q.index = next_index;
        for (row = y_root + 1; row < wfa->states; row++) {
            for (label = 0; label < 2; label++)
                if (FA_TREE(wfa, row, label) == FA_RANGE && qad_get(&q)) {
                    if (in->over || !add_edge(wfa, row, (unsigned) y_domains[d], label)) { free(y_domains); return truncated(in, "chroma matrices"), 0; }
                    (*total)++;
                }
            if (save) { next_index = q.index; save = 0; }
            if (in->over) { free(y_domains); return truncated(in, "chroma matrices"), 0; }
        }
    }
    free(y_domains);
    compute_y_state(wfa, FA_TREE(wfa, (unsigned) FA_TREE(wfa, wfa->root_state, 0), 1), (int) y_root);
    compute_y_state(wfa, FA_TREE(wfa, (unsigned) FA_TREE(wfa, wfa->root_state, 1), 0), (int) y_root);
    /* the column of the Y state at the same place */
    q.index = 0;
    for (row = y_root + 1; row < wfa->states; row++)
        for (label = 0; label < 2; label++) {
            const int yc = qad_get(&q);
            if (in->over) return truncated(in, "chroma matrices"), 0;
            wfa->y_column[row * 2 + label] = (uint8_t) yc;
            if (!yc) continue;
            /* A flag where there is no luminance state: the reference's coder keeps ONE automaton for a stream and the
             * flags of an earlier frame show through on the three states that join the bands (fa_job.ycol_carry).  Its
             * reader appends an edge into RANGE there -- nothing -- and counts it: one weight more than edges */
            if (wfa->y_state[row * 2 + label] == FA_RANGE) { (*total)++; continue; }
            if (FA_TREE(wfa, row, label) != FA_RANGE) {
                fa_set_error("Stream error: state %u, label %u has no luminance state at its place.", row, label);
                return 0;
            }
            if (!add_edge(wfa, row, (unsigned) wfa->y_state[row * 2 + label], label)) return 0;
            (*total)++;
        }
    fa_br_align(in);
    return !truncated(in, "chroma matrices");
}

/* ------------------------------------------------------------ weights */

static int read_weights(unsigned total, fa_wfa *wfa, const fa_info *wi, fa_bitr *in)
{
    unsigned state, label, off1, off2, off3, off4, nw = 0, i, e;
    int min_level = FA_CAP_LEVEL + 8, max_level = 0, d_min = FA_CAP_LEVEL + 8, d_max = 0;
    int dc = 0, d_dc = 0, delta_approx = 0, dom, ok = 0;
    unsigned *w_arr = NULL, *l_arr = NULL, *c_symbols = NULL;

    for (state = wfa->basis_states; state < wfa->states; state++)
        if (wfa->delta_state[state]) { delta_approx = 1; break; }
    for (state = wfa->basis_states; state < wfa->states; state++)
        for (label = 0; label < 2; label++)
            if (FA_TREE(wfa, state, label) == FA_RANGE) {
                const int lv = (int) wfa->level_of_state[state] - 1;
                if (delta_approx && wfa->delta_state[state]) {
                    if (lv < d_min) d_min = lv;
                    if (lv > d_max) d_max = lv;
                    if (FA_INTO(wfa, state, label, 0) == 0) d_dc = 1;
                } else {
                    if (lv < min_level) min_level = lv;
                    if (lv > max_level) max_level = lv;
                    if (FA_INTO(wfa, state, label, 0) == 0) dc = 1;
                }
            }
    if (min_level > max_level) max_level = min_level - 1;
    if (d_min > d_max) d_max = d_min - 1;
    off1 = dc ? 1 : 0;
    off2 = off1 + (d_dc ? 1 : 0);
    off3 = off2 + (unsigned) (max_level - min_level + 1);
    off4 = off3 + (unsigned) (d_max - d_min + 1);

    w_arr = (unsigned *) calloc(total, sizeof(unsigned));
    l_arr = (unsigned *) calloc(total, sizeof(unsigned));
    c_symbols = (unsigned *) calloc(off4 ? off4 : 1, sizeof(unsigned));
    if (!w_arr || !l_arr || !c_symbols) { fa_set_error("Out of memory!"); goto out; }
    for (state = wfa->basis_states; state < wfa->states; state++)
        for (label = 0; label < 2; label++)
            if (FA_TREE(wfa, state, label) == FA_RANGE)
                for (e = 0; (dom = FA_INTO(wfa, state, label, e)) != FA_NO_EDGE; e++) {
                    const int is_delta = delta_approx && wfa->delta_state[state];
                    if (nw >= total) { fa_set_error("Can't read more than %d weights.", (int) total); goto out; }
                    if (dom) l_arr[nw++] = is_delta ? off3 + wfa->level_of_state[state] - 1 - (unsigned) d_min
                                                    : off2 + wfa->level_of_state[state] - 1 - (unsigned) min_level;
                    else l_arr[nw++] = is_delta ? off1 : 0;
                }
    /* nw < total: the flags counted without an edge (chroma_decoding); their symbols come last, in context 0 */
    c_symbols[0] = 1u << (wi->dc_rpf.mantissa_bits + 1);
    if (off1 != off2) c_symbols[off1] = 1u << (wi->d_dc_rpf.mantissa_bits + 1);
    for (i = off2; i < off3; i++) c_symbols[i] = 1u << (wi->rpf.mantissa_bits + 1);
    for (; i < off4; i++) c_symbols[i] = 1u << (wi->d_rpf.mantissa_bits + 1);
    if (!decode_array(in, w_arr, l_arr, c_symbols, off4, total, 500, "weights")) goto out;
    nw = 0;
    for (state = wfa->basis_states; state < wfa->states; state++)
        for (label = 0; label < 2; label++)
            if (FA_TREE(wfa, state, label) == FA_RANGE)
                for (e = 0; (dom = FA_INTO(wfa, state, label, e)) != FA_NO_EDGE; e++) {
                    const int is_delta = delta_approx && wfa->delta_state[state];
                    const fa_rpf *r = dom ? (is_delta ? &wi->d_rpf : &wi->rpf) : (is_delta ? &wi->d_dc_rpf : &wi->dc_rpf);
                    FA_WEIGHT(wfa, state, label, e) = fa_btor((int) w_arr[nw++], r);
                }
    ok = 1;
out:
    free(w_arr); free(l_arr); free(c_symbols);
    return ok;
}

/* ------------------------------------------------------------ frame */

/* the basis in front of a fresh automaton.  The lists of a long basis run on behind the row of their label
 * (fa_wfa_append_edge): everything up to the end of the last list is copied, and a basis whose last list runs on
 * into the rows of the frame's first state is refused */
static int copy_basis(fa_wfa *w, const fa_wfa *basis)
{
    const size_t bs = basis->basis_states, rows = bs * 12;
    size_t i;
    if (basis->into[rows] != FA_NO_EDGE) { fa_set_error("The edges of the initial basis run on behind its last state."); return 0; }
    memcpy(w->final_distribution, basis->final_distribution, bs * sizeof(float));
    memcpy(w->level_of_state, basis->level_of_state, bs);
    memcpy(w->domain_type, basis->domain_type, bs);
    memcpy(w->into, basis->into, rows * sizeof(int16_t));
    memcpy(w->weight, basis->weight, rows * sizeof(float));
    for (i = 0; i < bs * 2; i++) w->tree[i] = basis->tree[i];
    w->basis_states = w->states = basis->basis_states;
    return 1;
}

fa_wfa *fa_read_frame(fa_bitr *in, const fa_info *wi, const fa_wfa *basis, unsigned *number, int flags[3])
{
    unsigned states, type, max_states, max_level, state, edges = 0, root;
    fa_wfa *wfa;
    states  = fa_br_rice(in, 8);
    type    = fa_br_rice(in, 8);
    *number = fa_br_rice(in, 8);
    fa_br_align(in);
    if (truncated(in, "frame header")) return NULL;
    fa_limits(&max_states, &max_level);
    if (states <= basis->basis_states || states > max_states || states > FA_CAP_STATES) {
        fa_set_error("Stream error: a frame of %u states (more than the %u of the basis, at most %u; fiasco_amd_set_limits).", states,
                     basis->basis_states, max_states < FA_CAP_STATES ? max_states : FA_CAP_STATES);
        return NULL;
    }
    if (type > FA_B_FRAME || (type != FA_I_FRAME && wi->frames < 2)) { fa_set_error("Stream error: frame type %u.", type); return NULL; }
    if (*number >= wi->frames) { fa_set_error("Stream error: frame number %u of %u frames.", *number, wi->frames); return NULL; }
    if (fa_br_get_bit(in)) {
        fa_set_error("Image tiling is not supported: no coder writes it (the tiling flag of frame %u is set).", *number);
        return NULL;
    }
    fa_br_align(in);
    if (truncated(in, "frame header")) return NULL;
    wfa = fa_wfa_alloc(states + 8);
    if (!wfa) { fa_set_error("Out of memory!"); return NULL; }
    if (!copy_basis(wfa, basis)) goto bad;
    wfa->states = states;
    wfa->frame_type = (int) type;
    if (!read_tree(wfa, wi, in)) goto bad;
    root = wi->color ? y_root_of(wfa) : wfa->root_state;
    if (root < 4) { fa_set_error("Stream error: a luminance band of %u states.", root); goto bad; }
    /* the domain pool as read_next_wfa computes it (input/read.c:393-416) */
    for (state = wfa->basis_states; state < wfa->states; state++) {
        const unsigned lv = wfa->level_of_state[state];
        wfa->domain_type[state] = (!wi->color || state <= root)
                                  && wfa->x[state * 2] + fa_width_of_level(lv) <= wi->width
                                  && wfa->y[state * 2] + fa_height_of_level(lv) <= wi->height ? FA_USE_DOMAIN : 0;
    }
    flags[0] = (int) fa_br_get_bit(in);
    if (truncated(in, "prediction flag")) goto bad;
    if (flags[0] && !read_nd(wfa, wi, in)) goto bad;
    if (type != FA_I_FRAME && !read_mc((int) type, wfa, wi, in)) goto bad;
    locate_delta_images(wfa);
    if (!column0_decoding(wfa, root, in, &edges)) goto bad;
    if (!delta_decoding(wfa, root, in, &edges, flags)) goto bad;
    if (wi->color && !chroma_decoding(wfa, wi, in, &edges)) goto bad;
    if (edges && !read_weights(edges, wfa, wi, in)) goto bad;
    /* compute_final_distribution (codec/wfalib.c:155-180); the decoder turns it into a pixel: a value no frame has
     * is refused before it gets there */
    for (state = wfa->basis_states; state < wfa->states; state++) {
        float final = 0;
        unsigned label, e;
        int dom;
        for (label = 0; label < 2; label++) {
            if ((dom = FA_TREE(wfa, state, label)) != FA_RANGE) final += wfa->final_distribution[dom];
            for (e = 0; (dom = FA_INTO(wfa, state, label, e)) != FA_NO_EDGE; e++)
                final += FA_WEIGHT(wfa, state, label, e) * wfa->final_distribution[dom];
        }
        final /= 2;
        if (!(final > -1e6f && final < 1e6f)) { fa_set_error("Stream error: the final distribution of state %u is out of range.", state); goto bad; }
        wfa->final_distribution[state] = final;
    }
    return wfa;
bad:
    fa_wfa_free(wfa);
    return NULL;
}
