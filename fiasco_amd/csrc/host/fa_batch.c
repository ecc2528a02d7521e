/*
 *  fa_batch.c -- the batch entry points: independent stills side by side through the core.
 *
 *  The life cycle of a staged batch (include/libfiasco_amd.h): stage parses the frames and makes them resident where
 *  the core computes, submit / collect / encode run passes over them and write the streams, upload replaces the
 *  frames while a pass runs, free releases everything.  The search itself runs behind fa_core_*(); what the host
 *  adds is the PNM reader in front of it and the entropy writer (output/write.c:53-119 in the reference) behind it,
 *  both on a few threads (fa_fan_out).  The outlets of the decoder on a finished batch: fa_batch_decode.c.
 */
#include <stdlib.h>
#include <string.h>
#include "fa_host.h"
#include "libfiasco_amd_ycbcr.h"

/* struct fiasco_amd_batch: fa_host.h (the device-input entry points of the core fill one too) */

int fiasco_amd_batch_stats(const fiasco_amd_batch_t *b, unsigned i, unsigned band,
                           float *costs, float *err, unsigned *width, unsigned *height)
{
    if (!b || i >= b->n || band > 2 || !b->jobs[i].status) return 0;
    if (band && !b->jobs[i].image->color) return 0;
    if (costs)  *costs  = b->jobs[i].stats[band].costs;
    if (err)    *err    = b->jobs[i].stats[band].err;
    if (width)  *width  = b->jobs[i].image->width;
    if (height) *height = b->jobs[i].image->height;
    return 1;
}

/* include/libfiasco_amd_hip.h: the planes the coder sees for frame i, all bands back to back; a frame that lives on
 * the device is fetched (fa_image_host_planes) */
int fiasco_amd_batch_input_planes(const fiasco_amd_batch_t *b, unsigned i, int16_t *out)
{
    const fa_image *im;
    size_t npix;
    int band;
    if (!b || i >= b->n || !out) { fa_set_error("fiasco_amd_batch_input_planes: no frame %u", i); return 0; }
    im = b->ims[i];
    npix = (size_t) im->width * im->height;
    if (!fa_image_host_planes(im)) return 0;
    for (band = 0; band < (im->color ? 3 : 1); band++) memcpy(out + (size_t) band * npix, im->pixels[band], npix * 2);
    return 1;
}

void fiasco_amd_batch_free(fiasco_amd_batch_t *b)
{
    unsigned i;
    if (!b) return;
    if (b->staged) fa_core_unstage(b->staged);
    for (i = 0; i < b->n; i++) {
        if (b->jobs && b->jobs[i].wfa) fa_wfa_free(b->jobs[i].wfa);
        if (b->ims) fa_image_free(b->ims[i]);
        if (b->prev_ims) fa_image_free(b->prev_ims[i]);
        if (b->infos) fa_info_free(&b->infos[i]);
    }
    free(b->jobs); free(b->ims); free(b->prev_ims); free(b->infos);
    free(b);
}

/* a staged batch of n frames, frame i being make(ctx, i) (NULL + message: the batch is refused) */
static fiasco_amd_batch_t *stage_images(unsigned n, fa_image *(*make)(const void *ctx, unsigned i), const void *ctx, float quality,
                                        const fiasco_c_options_t *options)
{
    fiasco_c_options_t *defaults = NULL;
    const fa_options *op;
    fiasco_amd_batch_t *b;
    unsigned i;

    if (quality <= 0) { fa_set_error("Compression quality has to be positive."); return NULL; }
    if (options) { op = fa_cast_options(options); if (!op) return NULL; }
    else { defaults = fiasco_c_options_new(); if (!defaults) return NULL; op = fa_cast_options(defaults); }
    b = (fiasco_amd_batch_t *) calloc(1, sizeof *b);
    if (b) {
        b->jobs  = (fa_job *) calloc(n ? n : 1, sizeof *b->jobs);
        b->ims   = (fa_image **) calloc(n ? n : 1, sizeof *b->ims);
        b->infos = (fa_info *) calloc(n ? n : 1, sizeof *b->infos);
    }
    if (!b || !b->jobs || !b->ims || !b->infos) {
        fa_set_error("Out of memory!");
        if (defaults) fiasco_c_options_delete(defaults);
        fiasco_amd_batch_free(b);
        return NULL;
    }
    b->n = n;
    b->normal_domains = op->normal_domains;
    b->delta_domains  = op->delta_domains;
    b->prediction     = op->prediction;
    for (i = 0; i < n; i++) {
        fa_cparams cp;
        b->ims[i] = make(ctx, i);
        if (!b->ims[i] || !fa_setup_params(op, quality, b->ims[i]->width, b->ims[i]->height,
                                          b->ims[i]->color, 1, &b->infos[i], &cp)
            || !fa_prepare_job(&b->jobs[i], b->ims[i], &cp, op->basis_name)) {
            if (defaults) fiasco_c_options_delete(defaults);
            fiasco_amd_batch_free(b);
            return NULL;
        }
    }
    if (defaults) fiasco_c_options_delete(defaults);
    b->staged = fa_core_stage(n, b->jobs);
    return b;
}

typedef struct { const unsigned char *const *pnm; const size_t *len; } pnm_frames;
static fa_image *make_from_pnm(const void *ctx, unsigned i)
{
    const pnm_frames *f = (const pnm_frames *) ctx;
    return fa_image_from_pnm(f->pnm[i], f->len[i], "<memory>");
}

fiasco_amd_batch_t *fiasco_amd_batch_stage(unsigned n, const unsigned char *const *pnm,
                                           const size_t *pnm_len, float quality,
                                           const fiasco_c_options_t *options)
{
    pnm_frames f;
    f.pnm = pnm; f.len = pnm_len;
    return stage_images(n, make_from_pnm, &f, quality, options);
}

/* include/libfiasco_amd_ycbcr.h: the same with YCbCr bytes in host memory; every frame is checked before anything is
 * allocated */
static fa_image *make_from_ycbcr(const void *ctx, unsigned i)
{
    return fa_image_from_ycbcr((const fiasco_amd_ycbcr_frame *) ctx + i, NULL);
}

fiasco_amd_batch_t *fiasco_amd_batch_stage_ycbcr(unsigned n, const fiasco_amd_ycbcr_frame *frames, float quality,
                                                 const fiasco_c_options_t *options)
{
    fiasco_amd_ycbcr_frame *fr;
    fiasco_amd_batch_t *b = NULL;
    unsigned i;
    if (!n || !frames) { fa_set_error("No frames to stage."); return NULL; }
    fr = (fiasco_amd_ycbcr_frame *) calloc(n, sizeof *fr);
    if (!fr) { fa_set_error("Out of memory!"); return NULL; }
    for (i = 0; i < n; i++) if (!fa_ycbcr_check(i, &frames[i], &fr[i])) break;
    if (i == n) b = stage_images(n, make_from_ycbcr, fr, quality, options);
    free(fr);
    return b;
}

/* ---------------------------------------------------------------- the streams of a finished pass */

/* developer aid: FIASCO_DUMP_WFA=<file> appends a text dump of every automaton handed to the
 * writer (diff the dumps of two cores to find what the per-call traces cannot show) */
static void dump_wfa(const fa_wfa *w)
{
    const char *path = fa_knob("FIASCO_DUMP_WFA");
    FILE *f;
    unsigned s, l, e;
    if (!path || !(f = fopen(path, "a"))) return;
    fprintf(f, "wfa states %u basis %u root %u\n", w->states, w->basis_states, w->root_state);
    for (s = 0; s < w->states; s++) {
        fprintf(f, "%u: fd %.9g lvl %u dt %u", s, w->final_distribution[s], w->level_of_state[s], w->domain_type[s]);
        for (l = 0; l < 2; l++) {
            fprintf(f, " | t %d xy %u,%u ys %d yc %u :", FA_TREE(w, s, l), w->x[s * 2 + l], w->y[s * 2 + l],
                    w->y_state[s * 2 + l], w->y_column[s * 2 + l]);
            for (e = 0; e < 6 && FA_INTO(w, s, l, e) != FA_NO_EDGE; e++)
                fprintf(f, " %d*%.9g", FA_INTO(w, s, l, e), FA_WEIGHT(w, s, l, e));
        }
        fprintf(f, "\n");
    }
    fclose(f);
}

/* the entropy writer of every finished frame (output/write.c:53-119 in the reference): a pure
 * function of the frame's automaton, so the frames of a batch are written by a few host
 * threads */
typedef struct { fiasco_amd_batch_t *b; unsigned char **outv; size_t *out_len; unsigned good[FA_FAN_MAX];
                 char err[FA_FAN_MAX][256]; } wr_task;

static void wr_share(void *ctx, unsigned t, unsigned nt)
{
    wr_task *w = (wr_task *) ctx;
    fiasco_amd_batch_t *b = w->b;
    unsigned i;
    for (i = t; i < b->n; i += nt) {
        fa_bitw out;
        if (!b->jobs[i].status) continue;
        if (b->n == 1) dump_wfa(b->jobs[i].wfa);
        fa_bw_init(&out);
        if (fa_write_frame(b->jobs[i].wfa, &b->infos[i], FA_I_FRAME, 0, b->prediction, b->normal_domains,
                           b->delta_domains, &out)) {
            w->out_len[i] = fa_bw_finish(&out);
            w->outv[i] = (unsigned char *) malloc(w->out_len[i]);
            if (w->outv[i]) {
                memcpy(w->outv[i], out.buf, w->out_len[i]);
                w->good[t]++;
            } else {
                w->out_len[i] = 0;
                snprintf(w->err[t], sizeof w->err[t], "Out of memory!");
            }
        } else if (!w->err[t][0])    /* the last-error string is per thread: hand it to the caller */
            snprintf(w->err[t], sizeof w->err[t], "%s", fiasco_get_error_message());
        fa_bw_free(&out);
    }
}

static unsigned write_streams(fiasco_amd_batch_t *b, unsigned char **outv, size_t *out_len)
{
    wr_task task;
    const unsigned cpus = fa_online_cpus();
    unsigned nt = b->n / 16, t, good = 0, i;
    if (nt > 16) nt = 16;
    if (nt > cpus) nt = cpus;
    if (nt < 1) nt = 1;
    task.b = b; task.outv = outv; task.out_len = out_len;
    for (t = 0; t < nt; t++) { task.good[t] = 0; task.err[t][0] = 0; }
    fa_fan_out(nt, wr_share, &task);
    for (t = 0; t < nt; t++) {
        good += task.good[t];
        if (task.err[t][0]) fa_set_error("%s", task.err[t]);     /* published after the join */
    }
    for (i = 0; i < b->n; i++)
        if (!b->jobs[i].status) fa_set_error("%s", b->jobs[i].errmsg);
    return good;
}

/* one pass to its streams: the core brings every frame to completion -- a whole pass (resubmit < 0), or the submitted
 * one, after which it may start the next -- and then the host writes */
static int pass_streams(fiasco_amd_batch_t *b, unsigned char **outv, size_t *out_len, int resubmit)
{
    unsigned i;
    if (!b) return 0;
    for (i = 0; i < b->n; i++) { outv[i] = NULL; out_len[i] = 0; }
    if (resubmit < 0) fa_core_run(b->staged);
    else fa_core_finish2(b->staged, resubmit);
    return (int) write_streams(b, outv, out_len);
}

int fiasco_amd_batch_submit(fiasco_amd_batch_t *b)
{
    return b ? fa_core_submit(b->staged) : 0;
}

/* finish the submitted pass; with `resubmit` the next pass over the same resident inputs is
 * started before the host writes the streams of this one, so that the entropy writer of pass
 * i overlaps the device search of pass i+1 (the next pass touches device memory only) */
int fiasco_amd_batch_collect(fiasco_amd_batch_t *b, unsigned char **outv, size_t *out_len, int resubmit)
{
    return pass_streams(b, outv, out_len, resubmit != 0);
}

int fiasco_amd_batch_encode(fiasco_amd_batch_t *b, unsigned char **outv, size_t *out_len)
{
    return pass_streams(b, outv, out_len, -1);
}

int fiasco_amd_encode_batch(unsigned n, const unsigned char *const *pnm, const size_t *pnm_len,
                            float quality, const fiasco_c_options_t *options,
                            unsigned char **outv, size_t *out_len)
{
    unsigned i;
    int good;
    fiasco_amd_batch_t *b = fiasco_amd_batch_stage(n, pnm, pnm_len, quality, options);
    if (!b) {
        for (i = 0; i < n; i++) { outv[i] = NULL; out_len[i] = 0; }
        return 0;
    }
    good = fiasco_amd_batch_encode(b, outv, out_len);
    fiasco_amd_batch_free(b);
    return good;
}

/* ---- replacing the inputs of a staged batch while a pass runs (a stream of batches) ---- */

typedef struct { fiasco_amd_batch_t *b; const unsigned char *const *pnm; const size_t *len;
                 int16_t *buf; const size_t *off; fa_image **out; unsigned bad[FA_FAN_MAX]; char err[FA_FAN_MAX][256]; } up_task;

static void up_share(void *ctx, unsigned t, unsigned nt)
{
    up_task *u = (up_task *) ctx;
    fiasco_amd_batch_t *b = u->b;
    unsigned i;
    for (i = t; i < b->n; i += nt) {
        const fa_image *old = b->ims[i];
        u->out[i] = fa_image_from_pnm_into(u->pnm[i], u->len[i], "<memory>", old->width, old->height,
                                           old->color, u->buf + u->off[i]);
        if (!u->out[i]) {
            if (!u->bad[t]) snprintf(u->err[t], sizeof u->err[t], "%s", fiasco_get_error_message());
            u->bad[t]++;
        }
    }
}

/* New frames for every slot of a staged batch (same sizes, colour model and options): parsed
 * by a few host threads straight into the core's upload staging memory and copied to the
 * device without waiting -- call it between submit and collect and the transfer overlaps the
 * pass that is running; the NEXT submit (or collect with resubmit) encodes the new frames. */
int fiasco_amd_batch_upload(fiasco_amd_batch_t *b, const unsigned char *const *pnm, const size_t *pnm_len)
{
    up_task task;
    const unsigned cpus = fa_online_cpus();
    unsigned nt, t, i, bad = 0;
    size_t total = 0, *off;
    int16_t *buf;
    fa_image **nims;

    if (!b || !b->staged || !b->n) { fa_set_error("Batch is not staged."); return 0; }
    off = (size_t *) malloc(b->n * sizeof *off);
    nims = (fa_image **) calloc(b->n, sizeof *nims);
    if (!off || !nims) { free(off); free(nims); fa_set_error("Out of memory!"); return 0; }
    for (i = 0; i < b->n; i++) {
        off[i] = total;
        total += (size_t) b->ims[i]->width * b->ims[i]->height * (b->ims[i]->color ? 3 : 1);
    }
    buf = fa_core_upload_buffer(b->staged, total * sizeof(int16_t));
    if (!buf) {
        free(off); free(nims);
        fa_set_error("No staging memory for %.1f MiB of frames.",
                     total * 2 / 1048576.0);
        return 0;
    }
    nt = b->n / 8;
    if (nt > 32) nt = 32;
    if (cpus > 1 && nt > cpus - 1) nt = cpus - 1;
    if (nt < 1) nt = 1;
    task.b = b; task.pnm = pnm; task.len = pnm_len; task.buf = buf; task.off = off; task.out = nims;
    for (t = 0; t < nt; t++) { task.bad[t] = 0; task.err[t][0] = 0; }
    fa_fan_out(nt, up_share, &task);
    for (t = 0; t < nt; t++) {
        bad += task.bad[t];
        if (task.err[t][0]) fa_set_error("%s", task.err[t]);
    }
    free(off);
    if (bad) {                                 /* nothing was replaced */
        for (i = 0; i < b->n; i++) fa_image_free(nims[i]);
        free(nims);
        return 0;
    }
    if (b->prev_ims) {
        for (i = 0; i < b->n; i++) fa_image_free(b->prev_ims[i]);
        free(b->prev_ims);
    }
    b->prev_ims = b->ims;                      /* alive until the next upload */
    b->ims = nims;
    for (i = 0; i < b->n; i++) b->jobs[i].image = nims[i];
    return fa_core_upload_commit(b->staged);
}

/* include/libfiasco_amd_hip.h: which hot-path backend this library was linked with (the seam fa_core_*()) */
const char *fiasco_amd_core_name(void) { return fa_core_name(); }
