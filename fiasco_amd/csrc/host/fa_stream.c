/*
 *  fa_stream.c -- a .fco stream that was read (include/libfiasco_amd_stream.h): its frames as automata, which frame is
 *  predicted from which, the frames written again, and the walk that decodes them.
 *
 *  Open reads everything (fa_reader.c).  Which frames serve as past and future of which follows get_next_frame
 *  (codec/decoder.c:160-410); fa_sequence.c holds the coder-side twin of that rule.  The walk hands the frames to the
 *  core's decoder (fa_core_decode_frames: the device) as jobs with from_stream set: the reference frames of a stream
 *  that is walked live at the magnification and in the format shown.  Its state is a cursor (fa_cursor) that may be
 *  kept between calls: fa_stream_walk() is one open, one advance and one close; the decoder objects (fa_decoder.c)
 *  advance one display frame per call.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fa_host.h"
#include "libfiasco_amd_stream.h"

struct fiasco_amd_stream {
    fa_info   wi;
    fa_wfa   *basis;
    unsigned  n;                /* frames, == wi.frames */
    fa_wfa  **wfa;              /* [n] coding order */
    unsigned *number;           /* [n] display number */
    int     (*flags)[3];        /* [n] prediction, use_normal, use_delta */
    int      *past, *future;    /* [n] coded index of the reference frames, -1: none */
    unsigned *coded_of;         /* [n] display number -> coded index */
};

const fa_info *fa_stream_info(const struct fiasco_amd_stream *s) { return &s->wi; }

void fiasco_amd_stream_free(fiasco_amd_stream_t *s)
{
    unsigned k;
    if (!s) return;
    for (k = 0; s->wfa && k < s->n; k++) fa_wfa_free(s->wfa[k]);
    fa_wfa_free(s->basis);
    free(s->wfa); free(s->number); free(s->flags); free(s->past); free(s->future); free(s->coded_of);
    fa_info_free(&s->wi);
    free(s);
}

/* get_next_frame's bookkeeping over the frames in coding order: the reference frames of each, and that every frame is
 * shown exactly once, in display order.  0 + message for an order no coder writes */
static int assign_references(fiasco_amd_stream_t *s)
{
    int frame = -1, past = -1, future = -1, pending = -1, is_future = 0;
    unsigned display = 0, k;
    for (k = 0; k < s->n; k++) {
        const int type = s->wfa[k]->frame_type;
        if (!k && s->number[0]) goto bad;                            /* the header goes in front of frame 0 */
        if (type == FA_I_FRAME) past = future = frame = -1;
        else if (type == FA_P_FRAME) { past = frame; frame = -1; future = -1; }
        else if (is_future) { future = pending; frame = -1; }
        else { if (s->wi.B_as_past_ref) past = frame; frame = -1; }
        is_future = 0;
        s->past[k] = past; s->future[k] = future;
        if (s->number[k] == display) { frame = (int) k; s->coded_of[display++] = k; }
        else if (s->number[k] > display && pending < 0) { pending = (int) k; is_future = 1; continue; }
        else goto bad;
        if (pending >= 0 && s->number[pending] == display) {        /* the future frame is shown behind its B frames */
            frame = pending; future = -1; pending = -1;
            s->coded_of[display++] = (unsigned) frame;
        }
    }
    if (display == s->n && pending < 0) return 1;
bad:
    fa_set_error("Stream error: the frames are not in an order a coder writes (frame %u is coded where frame %u is shown).",
                 k < s->n ? s->number[k] : s->n, display);
    return 0;
}

static fiasco_amd_stream_t *stream_open(const unsigned char *data, size_t len, const char *name)
{
    fiasco_amd_stream_t *s = (fiasco_amd_stream_t *) calloc(1, sizeof *s);
    unsigned max_states, max_level, k;
    fa_bitr in;
    if (!s) { fa_set_error("Out of memory!"); return NULL; }
    fa_br_init(&in, data, len);
    if (!fa_read_header(&in, name, &s->wi)) goto bad;
    fa_limits(&max_states, &max_level);
    s->basis = fa_wfa_alloc(max_states + 8);
    if (!s->basis) { fa_set_error("Out of memory!"); goto bad; }
    if (!fa_load_basis(s->wi.basis_name, s->basis)) goto bad;
    s->n = s->wi.frames;
    if ((size_t) s->n > len) { fa_set_error("Can't read next bit from the stream: it is truncated (%u frames in %lu bytes).", s->n, (unsigned long) len); goto bad; }
    s->wfa = (fa_wfa **) calloc(s->n, sizeof *s->wfa);
    s->number = (unsigned *) calloc(s->n, sizeof *s->number);
    s->flags = (int (*)[3]) calloc(s->n, sizeof *s->flags);
    s->past = (int *) calloc(s->n, sizeof *s->past);
    s->future = (int *) calloc(s->n, sizeof *s->future);
    s->coded_of = (unsigned *) calloc(s->n, sizeof *s->coded_of);
    if (!s->wfa || !s->number || !s->flags || !s->past || !s->future || !s->coded_of) { fa_set_error("Out of memory!"); goto bad; }
    for (k = 0; k < s->n; k++)
        if (!(s->wfa[k] = fa_read_frame(&in, &s->wi, s->basis, &s->number[k], s->flags[k]))) goto bad;
    if (!assign_references(s)) goto bad;
    return s;
bad:
    fiasco_amd_stream_free(s);
    return NULL;
}

struct fiasco_amd_stream *fa_stream_open_named(const unsigned char *data, size_t len, const char *name) { return stream_open(data, len, name); }

fiasco_amd_stream_t *fiasco_amd_stream_open(const unsigned char *data, size_t len)
{
    if (!data) { fa_set_error("fiasco_amd_stream_open: no stream"); return NULL; }
    return stream_open(data, len, "<memory>");
}

fiasco_amd_stream_t *fiasco_amd_stream_open_file(const char *name)
{
    unsigned char *data;
    size_t len = 0;
    fiasco_amd_stream_t *s;
    if (!name) { fa_set_error("fiasco_amd_stream_open_file: no file name"); return NULL; }
    data = fa_read_whole_file(name, "FIASCO_DATA", &len);
    if (!data) return NULL;
    s = stream_open(data, len, name);
    free(data);
    return s;
}

int fiasco_amd_stream_get_info(const fiasco_amd_stream_t *s, fiasco_amd_stream_info *info)
{
    if (!s || !info) { fa_set_error("fiasco_amd_stream_get_info: no stream or no place for the information"); return 0; }
    memset(info, 0, sizeof *info);
    info->width = s->wi.width; info->height = s->wi.height; info->color = s->wi.color;
    info->frames = s->wi.frames; info->fps = s->wi.fps; info->smoothing = s->wi.smoothing;
    info->title = s->wi.title ? s->wi.title : ""; info->comment = s->wi.comment ? s->wi.comment : "";
    info->basis_name = s->wi.basis_name;
    info->rpf_mantissa = s->wi.rpf.mantissa_bits; info->dc_rpf_mantissa = s->wi.dc_rpf.mantissa_bits;
    info->d_rpf_mantissa = s->wi.d_rpf.mantissa_bits; info->d_dc_rpf_mantissa = s->wi.d_dc_rpf.mantissa_bits;
    info->B_as_past_ref = s->wi.B_as_past_ref; info->half_pixel = s->wi.half_pixel;
    return 1;
}

int fiasco_amd_stream_frame_type(const fiasco_amd_stream_t *s, unsigned display)
{
    if (!s || display >= s->n) { fa_set_error("fiasco_amd_stream_frame_type: no frame %u", display); return -1; }
    return s->wfa[s->coded_of[display]]->frame_type;
}

int fiasco_amd_stream_coding_order(const fiasco_amd_stream_t *s, unsigned *order, unsigned cap)
{
    unsigned k;
    if (!s) { fa_set_error("fiasco_amd_stream_coding_order: no stream"); return 0; }
    if (order && cap < s->n) { fa_set_error("fiasco_amd_stream_coding_order: room for %u of %u frames", cap, s->n); return 0; }
    for (k = 0; order && k < s->n; k++) order[k] = s->number[k];
    return (int) s->n;
}

int fiasco_amd_stream_rewrite(const fiasco_amd_stream_t *s, unsigned char **out, size_t *out_len)
{
    fa_bitw bw;
    unsigned k;
    if (!out || !out_len) { fa_set_error("fiasco_amd_stream_rewrite: no place for the stream"); return 0; }
    *out = NULL; *out_len = 0;
    if (!s) { fa_set_error("fiasco_amd_stream_rewrite: no stream"); return 0; }
    fa_bw_init(&bw);
    for (k = 0; k < s->n; k++)
        if (!fa_write_frame(s->wfa[k], &s->wi, s->wfa[k]->frame_type, s->number[k], s->flags[k][0], s->flags[k][1], s->flags[k][2], &bw)) {
            fa_bw_free(&bw);
            return 0;
        }
    *out_len = fa_bw_finish(&bw);
    *out = (unsigned char *) malloc(*out_len ? *out_len : 1);
    if (!*out) { fa_bw_free(&bw); *out_len = 0; fa_set_error("Out of memory!"); return 0; }
    memcpy(*out, bw.buf, *out_len);
    fa_bw_free(&bw);
    return 1;
}

int fiasco_amd_stream_smoothing_borders(const fiasco_amd_stream_t *s, unsigned display, int magnify, int format_420,
                                        fiasco_amd_border *out, unsigned cap)
{
    const fa_wfa *w;
    if (!s || display >= s->n) { fa_set_error("fiasco_amd_stream_smoothing_borders: no frame %u", display); return 0; }
    w = s->wfa[s->coded_of[display]];
    if (format_420 && w->frame_type != FA_I_FRAME) return (int) fa_smoothing_borders_420_residual(w, s->wi.width, s->wi.height, s->wi.color, magnify, out, cap);
    if (format_420) return (int) fa_smoothing_borders_420(w, s->wi.width, s->wi.height, s->wi.color, magnify, out, cap);
    if (magnify) return (int) fa_smoothing_borders_magnified(w, s->wi.width, s->wi.height, s->wi.color, magnify, out, cap);
    return (int) fa_smoothing_borders(w, s->wi.width, s->wi.height, s->wi.color, out, cap);
}

/* ---------------------------------------------------------------- the cursor, and the walk over it */

/* The state of get_next_frame's walk, kept between calls (fa_host.h).  Everything is indexed by coded frame.  need,
 * isref, wanted and last_use are fixed at open: what the wanted frames of the range are predicted from.  images[] holds
 * the decoded frames a frame still to come is predicted from -- unsmoothed, with their device planes (keep_dev) --, and
 * with keep_images the wanted ones until they are taken; next is the position in coding order */
struct fa_cursor {
    const struct fiasco_amd_stream *s;
    char       who[64];
    unsigned   first, count;
    int        magnify, smoothing, format_420, keep_images;
    unsigned   next;
    uint8_t   *need, *isref, *failed, *wanted, *done;
    int       *last_use;
    fa_image **images;
    char     (*cause)[160];
    fa_dec_job *jobs;
    unsigned  *batch, *disp;
    uint8_t   *bw;
};

void fa_cursor_close(fa_cursor *c)
{
    unsigned k;
    if (!c) return;
    for (k = 0; c->images && k < c->s->n; k++) fa_image_free(c->images[k]);
    free(c->need); free(c->isref); free(c->failed); free(c->wanted); free(c->done); free(c->last_use); free(c->images); free(c->cause);
    free(c->jobs); free(c->batch); free(c->disp); free(c->bw);
    free(c);
}

fa_cursor *fa_cursor_open(const struct fiasco_amd_stream *s, const char *who, unsigned first, unsigned count, const uint8_t *mask, int magnify,
                          int smoothing, int format_420, int keep_images)
{
    const unsigned n = s->n;
    fa_cursor *c;
    unsigned k, i;
    int video = 0;

    if (!count || first >= n || count > n - first) { fa_set_error("%s: frames %u .. %u of a stream of %u frames", who, first, first + count - 1, n); return NULL; }
    if (smoothing < -1 || smoothing > 100) { fa_set_error("%s: smoothing out of range (-1: the header's value, 0: none, 1 .. 100 per cent)", who); return NULL; }
    if (smoothing < 0) smoothing = s->wi.smoothing <= 100 ? (int) s->wi.smoothing : 0;      /* get_next_frame :372-374 */
    c = (fa_cursor *) calloc(1, sizeof *c);
    if (!c) { fa_set_error("Out of memory!"); return NULL; }
    c->s = s; c->first = first; c->count = count; c->magnify = magnify; c->smoothing = smoothing; c->format_420 = format_420; c->keep_images = keep_images;
    snprintf(c->who, sizeof c->who, "%s", who);
    c->need = (uint8_t *) calloc(n, 1); c->isref = (uint8_t *) calloc(n, 1); c->failed = (uint8_t *) calloc(n, 1); c->wanted = (uint8_t *) calloc(n, 1);
    c->done = (uint8_t *) calloc(n, 1);
    c->last_use = (int *) calloc(n, sizeof *c->last_use);
    c->images = (fa_image **) calloc(n, sizeof *c->images);
    c->cause = (char (*)[160]) calloc(n, 160);
    c->jobs = (fa_dec_job *) calloc(n, sizeof *c->jobs);
    c->batch = (unsigned *) calloc(n, sizeof *c->batch); c->disp = (unsigned *) calloc(n, sizeof *c->disp); c->bw = (uint8_t *) calloc(n, 1);
    if (!c->need || !c->isref || !c->failed || !c->wanted || !c->done || !c->last_use || !c->images || !c->cause || !c->jobs || !c->batch || !c->disp || !c->bw) {
        fa_set_error("Out of memory!");
        goto bad;
    }
    for (i = first; i < first + count; i++) if (!mask || mask[i - first]) { c->need[s->coded_of[i]] = 1; c->wanted[s->coded_of[i]] = 1; }
    for (k = n; k-- > 0; ) {
        c->last_use[k] = -1;
        if (!c->need[k]) continue;
        video = video || s->wfa[k]->frame_type != FA_I_FRAME;
    }
    for (k = n; k-- > 0; ) {
        int r;
        if (!c->need[k]) continue;
        for (r = 0; r < 2; r++) {
            const int ref = r ? s->future[k] : s->past[k];
            if (ref < 0 || s->wfa[k]->frame_type == FA_I_FRAME) continue;
            c->need[ref] = 1; c->isref[ref] = 1;
            if (c->last_use[ref] < (int) k) c->last_use[ref] = (int) k;
        }
    }
    if (video && s->wi.half_pixel) {
        fa_set_error("Half-pixel motion vectors are not supported (the reference coder's half-pixel "
                     "path reads outside the reference frame).");
        goto bad;
    }
    return c;
bad:
    fa_cursor_close(c);
    return NULL;
}

/* the frames gathered go to run() as one call; then what nobody still to come (from coded frame k on) is predicted from goes */
static void cursor_flush(fa_cursor *c, unsigned nb, unsigned k, fa_stream_run run, void *ctx)
{
    const struct fiasco_amd_stream *s = c->s;
    unsigned nj = 0, i, j;
    unsigned *owner = c->batch;                    /* jobs[j] is frame owner[j]: compacted in place */
    for (i = 0; i < nb; i++) {
        const unsigned f = c->batch[i];
        const fa_wfa *w = s->wfa[f];
        fa_dec_job *d = &c->jobs[nj];
        int r, dead = 0;
        c->done[f] = 1;
        for (r = 0; r < 2 && !dead && w->frame_type != FA_I_FRAME; r++) {
            const int ref = r ? s->future[f] : s->past[f];
            if (ref >= 0 && c->failed[ref]) {
                snprintf(c->cause[f], 160, "display frame %u is predicted from frame %u, which failed: %.90s", s->number[f], s->number[ref], c->cause[ref]);
                c->failed[f] = 1; dead = 1;
            }
        }
        if (dead) continue;
        memset(d, 0, sizeof *d);
        d->wfa = w; d->width = s->wi.width; d->height = s->wi.height; d->color = s->wi.color; d->frame_type = w->frame_type;
        if (w->frame_type != FA_I_FRAME) {
            d->past = s->past[f] >= 0 ? c->images[s->past[f]] : NULL;
            d->future = s->future[f] >= 0 ? c->images[s->future[f]] : NULL;
        }
        d->p_max_level = s->wi.p_max_level;
        d->keep_dev = c->isref[f]; d->share_key = 1;        /* one share: the references never change device */
        d->magnify = c->magnify; d->format_420 = c->format_420; d->from_stream = 1;
        d->smoothing = c->wanted[f] ? c->smoothing : 0;
        c->disp[nj] = s->number[f]; c->bw[nj] = c->wanted[f]; owner[nj] = f;
        nj++;
    }
    if (nj) run(ctx, nj, c->jobs, c->disp, c->bw);
    for (j = 0; j < nj; j++) {
        const unsigned f = owner[j];
        if (c->jobs[j].out) c->images[f] = c->jobs[j].out;
        else { c->failed[f] = 1; snprintf(c->cause[f], 160, "%s", c->jobs[j].errmsg[0] ? c->jobs[j].errmsg : "decoder failed"); }
    }
    for (j = 0; j < s->n; j++)
        if (c->images[j] && c->last_use[j] < (int) k && !(c->keep_images && c->wanted[j])) { fa_image_free(c->images[j]); c->images[j] = NULL; }
}

void fa_cursor_advance(fa_cursor *c, unsigned display, unsigned ahead, fa_stream_run run, void *ctx)
{
    const struct fiasco_amd_stream *s = c->s;
    const unsigned end = c->first + c->count;
    unsigned nb = 0, k, i, to = 0;
    /* one behind the last coded frame among the wanted display frames display .. display + ahead - 1 */
    for (i = display < c->first ? c->first : display; i < end && i - display < ahead; i++)
        if (c->wanted[s->coded_of[i]] && s->coded_of[i] + 1 > to) to = s->coded_of[i] + 1;
    if (to <= c->next) return;
    for (k = c->next; k <= to; k++) {
        int flush = k == to;
        if (!flush && !c->need[k]) continue;
        for (i = 0; !flush && i < nb; i++)
            flush = s->wfa[k]->frame_type != FA_I_FRAME && ((int) c->batch[i] == s->past[k] || (int) c->batch[i] == s->future[k]);
        if (flush && nb) { cursor_flush(c, nb, k, run, ctx); nb = 0; }
        if (k < to) c->batch[nb++] = k;
    }
    c->next = to;
}

int fa_cursor_status(const fa_cursor *c, unsigned display, const char **cause)
{
    const unsigned f = display < c->s->n ? c->s->coded_of[display] : 0;
    if (cause) *cause = "";
    if (display >= c->s->n || !c->done[f]) return -1;
    if (cause && c->failed[f]) *cause = c->cause[f];
    return !c->failed[f];
}

fa_image *fa_cursor_take(fa_cursor *c, unsigned display)
{
    const unsigned f = display < c->s->n ? c->s->coded_of[display] : 0;
    fa_image *im;
    if (display >= c->s->n || !c->keep_images || !c->wanted[f] || c->last_use[f] >= (int) c->next) return NULL;
    im = c->images[f]; c->images[f] = NULL;
    return im;
}

unsigned fa_cursor_held(const fa_cursor *c)
{
    unsigned k, held = 0;
    for (k = 0; k < c->s->n; k++) held += c->images[k] != NULL;
    return held;
}

int fa_stream_walk(const struct fiasco_amd_stream *s, const char *who, unsigned first, unsigned count, const uint8_t *mask, int magnify, int smoothing,
                   int format_420, fa_stream_run run, void *ctx, int keep_images, fa_image **result, char (*errs)[160])
{
    fa_cursor *c = fa_cursor_open(s, who, first, count, mask, magnify, smoothing, format_420, keep_images);
    int good = 0, named = 0;
    unsigned i;
    if (!c) return 0;
    fa_cursor_advance(c, first, count, run, ctx);
    for (i = first; i < first + count; i++) {
        const char *cause;
        const int st = fa_cursor_status(c, i, &cause);
        if (errs) snprintf(errs[i - first], 160, "%s", cause);
        if (keep_images && result) result[i - first] = fa_cursor_take(c, i);
        if (!c->wanted[s->coded_of[i]]) continue;
        good += st == 1;
        if (!st && !named) { fa_set_error("%s: display frame %u: %s", who, i, cause); named = 1; }
    }
    fa_cursor_close(c);
    return good;
}

/* ---------------------------------------------------------------- the host outlets */

static void run_seam(void *ctx, unsigned n, fa_dec_job *jobs, const unsigned *display, const uint8_t *wanted)
{
    (void) ctx; (void) display; (void) wanted;
    (void) fa_core_decode_frames(n, jobs);
}

static int decode_planes(const char *who, const fiasco_amd_stream_t *s, unsigned display, int magnify, int format_420, int16_t *out)
{
    unsigned w, h, b;
    size_t npix, cpix;
    fa_image *im = NULL;
    if (!s || !out) { fa_set_error("%s: no stream or no place for the planes", who); return 0; }
    if (display >= s->n) { fa_set_error("%s: no frame %u", who, display); return 0; }
    w = s->wi.width; h = s->wi.height;
    if (magnify && !fiasco_amd_magnified_size(w, h, magnify, &w, &h)) return 0;
    if (format_420 && !s->wi.color) { fa_set_error("%s: 4:2:0: a gray frame has no chroma bands", who); return 0; }
    if (fa_stream_walk(s, who, display, 1, NULL, magnify, 0, format_420, run_seam, NULL, 1, &im, NULL) != 1 || !im) { fa_image_free(im); return 0; }
    if (im->width != w || im->height != h || !im->pixels[0]) {
        fa_set_error("%s: the decoder of this library (%s) handed back a frame of %u x %u pixels where %u x %u are shown", who, fa_core_name(),
                     im->width, im->height, w, h);
        fa_image_free(im);
        return 0;
    }
    npix = (size_t) w * h; cpix = format_420 ? (size_t) (w >> 1) * (h >> 1) : npix;
    memcpy(out, im->pixels[0], npix * 2);
    for (b = 1; b < (s->wi.color ? 3u : 1u); b++) memcpy(out + npix + (b - 1) * cpix, im->pixels[b], cpix * 2);
    fa_image_free(im);
    return 1;
}

int fiasco_amd_stream_decode_planes(const fiasco_amd_stream_t *s, unsigned display, int magnify, int16_t *out)
{
    return decode_planes("fiasco_amd_stream_decode_planes", s, display, magnify, 0, out);
}

int fiasco_amd_stream_decode_planes_420(const fiasco_amd_stream_t *s, unsigned display, int magnify, int16_t *out)
{
    return decode_planes("fiasco_amd_stream_decode_planes_420", s, display, magnify, 1, out);
}
