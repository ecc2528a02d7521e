/*
 *  fa_batch_decode.c -- the host outlets of the decoder on a finished batch, and the smoothing-border list.
 *
 *  A staged batch whose last pass succeeded holds one finished automaton per frame.  The entries here hand such an
 *  automaton to the core's decoder (fa_core_decode_frames: the device in the product, the host decoder in the test
 *  oracle) and bring the result to the host: the decoded PSNR, a band as bytes, the planes in 12.4 fixed point, at
 *  the coded size or magnified.  Intra frames only -- a P/B frame needs its reference frames.  The outlets that leave
 *  the frame in device memory are the core's (csrc/hip/output_convert.inc, distortion.inc); they fill their decoder
 *  jobs with fa_dec_job_of() too.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "fa_host.h"
#include "libfiasco_amd_hip.h"
#include "libfiasco_amd_display.h"
#include "libfiasco_amd_420.h"

/* The guard of every outlet `who': the finished intra job of frame i, or NULL + message.  `usable': the caller's own
 * precondition (an output buffer), refused in the same words as a missing automaton.  `why' ends the refusal of a P/B
 * frame; fiasco_amd_batch_decode_plane() passes none and the band it wants, and refuses both in one sentence. */
static const fa_job *finished_intra(const fiasco_amd_batch_t *b, unsigned i, int usable, const char *who, const char *why,
                                    unsigned band)
{
    const fa_job *job;
    unsigned bands;
    if (!b || i >= b->n || !b->jobs[i].status || !b->jobs[i].wfa || !usable) {
        fa_set_error("%s: frame %u has no finished automaton", who, i);
        return NULL;
    }
    job = &b->jobs[i];
    bands = job->image->color ? 3u : 1u;
    if (job->frame_type != FA_I_FRAME || band >= bands) {
        if (why) fa_set_error("%s: intra frames only%s", who, why);
        else fa_set_error("%s: intra frames only, band < %u", who, bands);
        return NULL;
    }
    return job;
}
#define NEEDS_REFERENCES " (a P/B frame needs its reference frames)"

void fa_dec_job_of(const fa_job *job, int magnify, fa_dec_job *d)
{
    memset(d, 0, sizeof *d);
    if (!job->status || !job->wfa || job->frame_type != FA_I_FRAME) { d->skip = 1; return; }
    d->wfa = job->wfa; d->width = job->image->width; d->height = job->image->height; d->color = job->image->color;
    d->frame_type = FA_I_FRAME; d->magnify = magnify;
}

/* the frame of a finished intra job through the core's decoder (the device; the host decoder in the test oracle) */
static fa_image *decode_job(const fa_job *job, int magnify)
{
    fa_dec_job d;
    fa_dec_job_of(job, magnify, &d);
    if (fa_core_decode_frames(1, &d) != 1 || !d.out) {
        fa_set_error("%s", d.errmsg[0] ? d.errmsg : "decoder failed");
        return NULL;
    }
    return d.out;
}

/* ---------------------------------------------------------------- decoded PSNR */

/* Decoded PSNR of frame i of a batch whose last pass succeeded: the finished automaton
 * is decoded like `dfiasco -s 0` does (decode_image, codec/decoder.c:411-536, no smoothing -- the frame the
 * coder itself would use as a reference) and compared with the input the way bin/pnmpsnr.c:36-163 compares
 * two PNM files: both sides as bytes, clip((pixel >> 4) + 128) (lib/image.c gray_write), squared differences
 * summed sequentially in float, 10 log10(255^2 / mean).  psnr_db[band] = +inf when the planes do not
 * differ (pnmpsnr: "don't differ" below 1e-4).  For square gray frames that is pnmpsnr's figure to the
 * last digit (tests/golden/MANIFEST.json "decoded_psnr").  For w x h frames the reference tool divides by
 * w x w -- fiasco_image_get_height() returns the width, lib/image.c:134 -- so its mean is ours x h / w for
 * h <= w (the tests convert); here the mean is over the pixels of the image.  For colour frames the three
 * planes Y, Cb, Cr are compared as they are, without pnmpsnr's detour through RGB. */

/* mean squared error and PSNR of a decoded frame against its original, as bin/pnmpsnr.c:92-101 sums them */
static void psnr_of(const fa_image *orig, const fa_image *dec, double psnr_db[3], double mse[3])
{
    const unsigned nb = orig->color ? 3 : 1;
    unsigned band;
    for (band = 0; band < 3; band++) { if (psnr_db) psnr_db[band] = 0; if (mse) mse[band] = 0; }
    for (band = 0; band < nb; band++) {
        const int16_t *p = orig->pixels[band], *q = dec->pixels[band];
        const size_t n = (size_t) orig->width * orig->height;
        size_t k;
        float norm = 0;                                 /* real_t, summed in file order (bin/pnmpsnr.c:92-101) */
        for (k = 0; k < n; k++) {
            int a = (p[k] >> 4) + 128, c = (q[k] >> 4) + 128;
            a = a < 0 ? 0 : a > 255 ? 255 : a;
            c = c < 0 ? 0 : c > 255 ? 255 : c;
            norm += (float) ((a - c) * (a - c));
        }
        norm /= (float) n;
        if (mse) mse[band] = norm;
        if (psnr_db) psnr_db[band] = norm > 1e-4 ? 10 * log(255.0 * 255.0 / norm) / log(10.0) : INFINITY;
    }
}

int fiasco_amd_batch_decode_psnr(const fiasco_amd_batch_t *b, unsigned i, double psnr_db[3], double mse[3])
{
    const fa_job *job = finished_intra(b, i, 1, "fiasco_amd_batch_decode_psnr", NEEDS_REFERENCES, 0);
    fa_image *dec;
    if (!job) return 0;
    if (!fa_image_host_planes(job->image)) return 0;           /* a frame that lives on the device: fetched now */
    dec = decode_job(job, 0);
    if (!dec) return 0;
    psnr_of(job->image, dec, psnr_db, mse);
    fa_image_free(dec);
    return 1;
}

/* All frames of the batch in ONE call of the core's decoder (the device runs them back to back on a stream, every
 * device of the process its share); psnr_db / mse: [n][3], either may be NULL.  Frames without a finished intra
 * automaton get zeros.  Returns the number of frames decoded. */
typedef struct psnr_task { const fiasco_amd_batch_t *b; fa_dec_job *d; double *psnr_db, *mse; } psnr_task;

static void psnr_share(void *ctx, unsigned t, unsigned nt)
{
    psnr_task *s = (psnr_task *) ctx;
    unsigned i, k;
    for (i = t; i < s->b->n; i += nt) {
        double p[3] = { 0, 0, 0 }, m[3] = { 0, 0, 0 };
        if (s->d[i].out) psnr_of(s->b->jobs[i].image, s->d[i].out, p, m);
        for (k = 0; k < 3; k++) { if (s->psnr_db) s->psnr_db[i * 3 + k] = p[k]; if (s->mse) s->mse[i * 3 + k] = m[k]; }
    }
}

int fiasco_amd_batch_decode_psnr_all(const fiasco_amd_batch_t *b, double *psnr_db, double *mse)
{
    psnr_task task;
    fa_dec_job *d;
    unsigned i, nt = fa_online_cpus();
    int good;
    if (!b || !b->n) { fa_set_error("fiasco_amd_batch_decode_psnr_all: empty batch"); return 0; }
    d = (fa_dec_job *) calloc(b->n, sizeof *d);
    if (!d) { fa_set_error("Out of memory!"); return 0; }
    for (i = 0; i < b->n; i++) {
        fa_dec_job_of(&b->jobs[i], 0, &d[i]);
        if (!d[i].skip && !fa_image_host_planes(b->jobs[i].image)) { free(d); return 0; }   /* as fiasco_amd_batch_decode_psnr: 0 + message */
    }
    good = fa_core_decode_frames(b->n, d);
    if (nt > 16) nt = 16;
    if (nt > b->n) nt = b->n;
    task.b = b; task.d = d; task.psnr_db = psnr_db; task.mse = mse;
    fa_fan_out(nt, psnr_share, &task);
    for (i = 0; i < b->n; i++) {
        if (!d[i].skip && !d[i].out && d[i].errmsg[0]) fa_set_error("%s", d[i].errmsg);
        fa_image_free(d[i].out);
    }
    free(d);
    return good;
}

/* ---------------------------------------------------------------- the decoded frame itself */

/* Frame i at magnification `magnify', copied out: the body of the three entries below.  planes != 0: all bands as the
 * decoder leaves them, back to back; else band `band' as bytes, clip((pixel >> 4) + 128).  The size rule is consulted
 * only for magnify != 0; a core that hands back a frame of another size (the test oracle's host decoder) does not
 * magnify: refused */
static int decode_out(const char *who, const fiasco_amd_batch_t *b, unsigned i, int magnify, const char *why,
                      unsigned band, int planes, void *out)
{
    const fa_job *job = finished_intra(b, i, out != NULL, who, why, band);
    unsigned w, h, k;
    size_t npix, j;
    fa_image *dec;
    if (!job) return 0;
    w = job->image->width; h = job->image->height;
    if (magnify && !fiasco_amd_magnified_size(w, h, magnify, &w, &h)) return 0;
    dec = decode_job(job, magnify);
    if (!dec) return 0;
    if (magnify && (dec->width != w || dec->height != h)) {
        fa_set_error("%s: the decoder of this library (%s) does not magnify: %u x %u pixels "
                     "where magnification %d shows %u x %u", who, fa_core_name(), dec->width, dec->height, magnify, w, h);
        fa_image_free(dec);
        return 0;
    }
    npix = (size_t) w * h;
    for (k = 0; planes && k < (job->image->color ? 3u : 1u); k++) memcpy((int16_t *) out + k * npix, dec->pixels[k], npix * 2);
    for (j = 0; !planes && j < npix; j++) {
        int v = (dec->pixels[band][j] >> 4) + 128;
        ((unsigned char *) out)[j] = (unsigned char) (v < 0 ? 0 : v > 255 ? 255 : v);
    }
    fa_image_free(dec);
    return 1;
}

/* The decoded frame itself: band `band` of frame i as bytes, clip((pixel >> 4) + 128) in raster order
 * (width x height of the input) -- for a gray frame exactly the payload of the PGM that `dfiasco -s 0 -o`
 * writes (lib/image.c gray_write :449-483).  out must hold width * height bytes. */
int fiasco_amd_batch_decode_plane(const fiasco_amd_batch_t *b, unsigned i, unsigned band, unsigned char *out)
{
    return decode_out("fiasco_amd_batch_decode_plane", b, i, 0, NULL, band, 0, out);
}

/* The decoded planes themselves, before any smoothing: 12.4 fixed point, all bands back to back -- the sibling of
 * fiasco_amd_batch_input_planes() on the other side of the coder. */
int fiasco_amd_batch_decode_planes(const fiasco_amd_batch_t *b, unsigned i, int16_t *out)
{
    return decode_out("fiasco_amd_batch_decode_planes", b, i, 0, NEEDS_REFERENCES, 0, 1, out);
}

/* fiasco_amd_batch_decode_planes() at a magnification: the planes have the size of fiasco_amd_magnified_size() */
int fiasco_amd_batch_decode_planes_magnified(const fiasco_amd_batch_t *b, unsigned i, int magnify, int16_t *out)
{
    return decode_out("fiasco_amd_batch_decode_planes_magnified", b, i, magnify, NEEDS_REFERENCES, 0, 1, out);
}

/* ---------------------------------------------------------------- magnification (include/libfiasco_amd_hip.h) */

/* The size `dfiasco -m magnify' shows a frame of width x height at, and whether it decodes it at all: the rules of
 * fiasco_decoder_new (codec/dfiasco.c:104-137) and of get_next_frame (codec/decoder.c:329-342).  Enlarging stops where a
 * step passes 2048 x 2048 pixels; reducing stops where a side falls below 32, and the halved sides are rounded up to
 * even.  A pure function of its arguments.  1 + the size, or 0 + a message that names the limit as the reference's does. */
int fiasco_amd_magnified_size(unsigned width, unsigned height, int magnify, unsigned *out_w, unsigned *out_h)
{
    long n;
    if (!width || !height || width > 8192 || height > 8192) {
        fa_set_error("fiasco_amd_magnified_size: no frame of %u x %u pixels", width, height);
        return 0;
    }
    if (magnify >= 0) {
        const unsigned long long pixels = (unsigned long long) width * height;
        for (n = 1; n <= magnify; n++)
            if (pixels << (n << 1) > 2048ull * 2048ull) {      /* stops at n <= 12: the shift stays small */
                fa_set_error("Magnification factor `%d' is too large for a frame of %u x %u pixels. Maximum value is %ld.",
                             magnify, width, height, n - 1);
                return 0;
            }
        if (out_w) *out_w = width << magnify;
        if (out_h) *out_h = height << magnify;
    } else {
        const long k = -(long) magnify;
        unsigned w, h;
        for (n = 0; n <= k; n++)
            if (width >> n < 32 || height >> n < 32) {         /* stops at n <= 9 */
                fa_set_error("Magnification factor `%d' is too small for a frame of %u x %u pixels. Minimum value is %ld.",
                             magnify, width, height, -(n > 1 ? n - 1 : 0));
                return 0;
            }
        w = width >> k; h = height >> k;
        if (out_w) *out_w = w + (w & 1);
        if (out_h) *out_h = h + (h & 1);
    }
    return 1;
}

/* ---------------------------------------------------------------- smoothing along the partition borders */

/* The borders smooth_image (codec/decoder.c:674-768) blends in a frame of width x height, in an order a parallel
 * machine can follow.  The reference walks the states basis_states .. bound - 1 in index order and changes the Y plane
 * in place; bound is the number of states for a gray frame and tree[root][0] for a colour frame, which leaves the Y
 * band AND the Cb band in (chroma states carry band-relative coordinates, so the luminance plane is smoothed a second
 * time along the Cb partition) and Cr out.  States are numbered children first, and two borders of one band share
 * pixels only when one state lies below the other in the tree; borders of one level and band lie inside disjoint
 * blocks.  So `Y band by ascending level, then Cb band by ascending level' gives the sequential result: one pass per
 * (band, level) that has a border, borders of a pass in state order.
 * A state's border lies between the halves of its block, where its label-1 child begins: odd levels are cut
 * horizontally (rows y - 1 and y, `len' columns from x), even levels vertically (columns x - 1 and x, `len' rows from
 * y); len is the block's side, clipped at the frame.  Returns the number of borders; out may be NULL (count only);
 * more than cap: 0 + message. */
/* The list at magnification `mag_y' (the Cb phase: `mag_cb', the same but for a 4:2:0 frame), against the size shown (width x height are the magnified ones): what smooth_image
 * walks after enlarge_image (codec/decoder.c:776-840) has added 2 mag to the level of every state and shifted its
 * coordinates by mag.  Same phases, same order.  *low: set to 1 + the coded level of the first visible state whose shifted
 * level falls below 1 (the caller refuses the frame); such a state is not listed. */
static unsigned borders_at(const fa_wfa *w, unsigned width, unsigned height, int color, int mag_y, int mag_cb, fiasco_amd_border *out, unsigned cap,
                           unsigned *low, int *low_mag)
{
    unsigned from[2], to[2], phases = 1, phase, n = 0, pass = 0;
    from[0] = w->basis_states; to[0] = w->states;
    if (color) {
        const unsigned join = (unsigned) FA_TREE(w, w->root_state, 0);
        to[0] = (unsigned) FA_TREE(w, join, 0) + 1;
        from[1] = to[0]; to[1] = join;
        phases = 2;
    }
    for (phase = 0; phase < phases; phase++) {
        const int mag = phase ? mag_cb : mag_y;
        int level, maxl = 0;
        unsigned s;
        for (s = from[phase]; s < to[phase]; s++) if ((int) w->level_of_state[s] + 2 * mag > maxl) maxl = (int) w->level_of_state[s] + 2 * mag;
        for (level = 0; level <= maxl; level++) {
            const unsigned side = level & 1 ? 1u << (level >> 1) : 1u << ((level + 1) >> 1);
            unsigned found = 0;
            for (s = from[phase]; s < to[phase]; s++) {
                const int shifted = (int) w->level_of_state[s] + 2 * mag;
                const unsigned x = mag >= 0 ? (unsigned) w->x[s * 2 + 1] << mag : (unsigned) w->x[s * 2 + 1] >> -mag;
                const unsigned y = mag >= 0 ? (unsigned) w->y[s * 2 + 1] << mag : (unsigned) w->y[s * 2 + 1] >> -mag;
                unsigned room;
                if ((shifted < 1 ? 0 : shifted) != level || y >= height || x >= width) continue;
                if (shifted < 1) { if (!*low) { *low = 1u + w->level_of_state[s]; *low_mag = mag; } continue; }
                if (level & 1 ? !y : !x) continue;
                room = level & 1 ? width - x : height - y;
                if (out) {
                    if (n >= cap) { fa_set_error("fiasco_amd_batch_smoothing_borders_magnified: more than %u borders", cap); return 0; }
                    out[n].x = (uint16_t) x; out[n].y = (uint16_t) y; out[n].len = (uint16_t) (side < room ? side : room);
                    out[n].level = (uint8_t) level; out[n].pass = (uint8_t) pass;
                }
                n++; found = 1;
            }
            pass += found;
        }
    }
    return n;
}

/* fa_smoothing_borders() of the frame as `dfiasco -m magnify' shows it: the coded list with x and y shifted by magnify,
 * the level raised by 2 magnify, the length the side of that level clipped at the size of fiasco_amd_magnified_size(), a
 * border that begins outside that size left out.  width x height: the CODED size.  magnify == 0: fa_smoothing_borders()
 * itself.  The pass order stays the reference's sequential result while every listed state keeps a level >= 1: its cut
 * then still lies on a whole pixel of the shown grid.  A state whose level falls below 1 (coded level <= 2 k at reduction
 * k) is clamped to level 0 by enlarge_image with its coordinates floored: the cut lands on the block's own edge, borders
 * share pixels, and at (0, 0) smooth_image reads and writes the word before the plane.  Such a frame is refused: 0 + message
 * `who' begins; so is a magnification the size rule refuses (its message). */
static unsigned borders_magnified(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out,
                                  unsigned cap, const char *who)
{
    unsigned mw = width, mh = height, low = 0, n;
    int low_mag = 0;
    if (!magnify) return fa_smoothing_borders(w, width, height, color, out, cap);
    if (!fiasco_amd_magnified_size(width, height, magnify, &mw, &mh)) return 0;
    if (magnify > 8) { fa_set_error("%s: magnification %d: the borders of the frame do not fit 16-bit coordinates", who, magnify); return 0; }
    n = borders_at(w, mw, mh, color, magnify, magnify, out, cap, &low, &low_mag);
    if (low) {
        fa_set_error("%s: at magnification %d a smoothed state of level %u falls to level %d (below 1), where the "
                     "reference's own result is undefined", who, magnify, low - 1, (int) low - 1 + 2 * magnify);
        return 0;
    }
    return n;
}

unsigned fa_smoothing_borders_magnified(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out,
                                        unsigned cap)
{
    return borders_magnified(w, width, height, color, magnify, out, cap, "smoothing borders");
}

unsigned fa_smoothing_borders(const fa_wfa *w, unsigned width, unsigned height, int color, fiasco_amd_border *out, unsigned cap)
{
    unsigned from[2], to[2], phases = 1, phase, n = 0, pass = 0;
    from[0] = w->basis_states; to[0] = w->states;
    if (color) {
        const unsigned join = (unsigned) FA_TREE(w, w->root_state, 0);        /* Y and Cb meet here: the reference's bound */
        to[0] = (unsigned) FA_TREE(w, join, 0) + 1;                           /* ... the root of Y included */
        from[1] = to[0]; to[1] = join;
        phases = 2;
    }
    for (phase = 0; phase < phases; phase++) {
        unsigned level, maxl = 0, s;
        for (s = from[phase]; s < to[phase]; s++) if (w->level_of_state[s] > maxl) maxl = w->level_of_state[s];
        for (level = 0; level <= maxl; level++) {
            const unsigned side = level & 1 ? 1u << (level >> 1) : 1u << ((level + 1) >> 1);   /* width_of_level : height_of_level */
            unsigned found = 0;
            for (s = from[phase]; s < to[phase]; s++) {
                const unsigned x = w->x[s * 2 + 1], y = w->y[s * 2 + 1];
                unsigned room;
                if (w->level_of_state[s] != level || y >= height || x >= width) continue;
                if (level & 1 ? !y : !x) continue;            /* no pixel before the first: no block is cut there */
                room = level & 1 ? width - x : height - y;
                if (out) {
                    if (n >= cap) { fa_set_error("fiasco_amd_batch_smoothing_borders: more than %u borders", cap); return 0; }
                    out[n].x = (uint16_t) x; out[n].y = (uint16_t) y; out[n].len = (uint16_t) (side < room ? side : room);
                    out[n].level = (uint8_t) level; out[n].pass = (uint8_t) pass;
                }
                n++; found = 1;
            }
            pass += found;
        }
    }
    return n;
}

int fiasco_amd_batch_smoothing_borders(const fiasco_amd_batch_t *b, unsigned i, fiasco_amd_border *out, unsigned cap)
{
    const fa_job *job = finished_intra(b, i, 1, "fiasco_amd_batch_smoothing_borders", "", 0);
    return job ? (int) fa_smoothing_borders(job->wfa, job->image->width, job->image->height, job->image->color, out, cap) : 0;
}

/* include/libfiasco_amd_display.h */
int fiasco_amd_batch_smoothing_borders_magnified(const fiasco_amd_batch_t *b, unsigned i, int magnify, fiasco_amd_border *out, unsigned cap)
{
    const fa_job *job = finished_intra(b, i, 1, "fiasco_amd_batch_smoothing_borders_magnified", "", 0);
    char who[80];
    if (!job) return 0;
    snprintf(who, sizeof who, "fiasco_amd_batch_smoothing_borders_magnified: frame %u", i);
    return (int) borders_magnified(job->wfa, job->image->width, job->image->height, job->image->color, magnify, out, cap, who);
}

/* ---------------------------------------------------------------- 4:2:0 (include/libfiasco_amd_420.h) */

/* What decode_image (codec/decoder.c:411-536) makes of the automaton once enlarge_image (:776-840) has shifted it for
 * FORMAT_4_2_0: see fa_host.h.  The states of a band cover every level from the largest range level up to the band's
 * root, so a band has a state at a level exactly when its root is not below it. */
int fa_420_plan_of(const fa_wfa *w, int color, int magnify, fa_420_plan *plan, char *msg, size_t msg_size)
{
    unsigned r0, r1, root[3], s, lc[2] = { 0, 0 }, have[2] = { 0, 0 }, found[3] = { 0, 0, 0 };
    const int shift[2] = { 2 * magnify, 2 * magnify - 2 };
    int top = -1, band, y_level, c_level;
    if (!color) { snprintf(msg, msg_size, "4:2:0: a gray frame has no chroma bands"); return 0; }
    r0 = (unsigned) FA_TREE(w, w->root_state, 0); r1 = (unsigned) FA_TREE(w, w->root_state, 1);
    root[0] = (unsigned) FA_TREE(w, r0, 0); root[1] = (unsigned) FA_TREE(w, r0, 1); root[2] = (unsigned) FA_TREE(w, r1, 0);
    for (s = w->basis_states; s < w->states; s++) {
        if (s == w->root_state || s == r0 || s == r1) continue;
        if (FA_INTO(w, s, 0, 0) == FA_NO_EDGE && FA_INTO(w, s, 1, 0) == FA_NO_EDGE) continue;
        band = s > root[0];
        have[band] = 1;
        if (w->level_of_state[s] > lc[band]) lc[band] = w->level_of_state[s];
    }
    for (band = 0; band < 2; band++) {
        if (!have[band]) continue;
        if ((int) lc[band] + shift[band] < 0) {
            snprintf(msg, msg_size, "4:2:0: the blocks of the %s are smaller than the reduction (level of the linear combinations %u below "
                     "twice the reduction %d)", band ? "chroma bands" : "Y band", lc[band], -shift[band] / 2);
            return 0;
        }
        if ((int) lc[band] + shift[band] > top) top = (int) lc[band] + shift[band];
    }
    if (top < 0) { snprintf(msg, msg_size, "4:2:0: no state with a linear combination"); return 0; }
    if (top > 24) { snprintf(msg, msg_size, "4:2:0: level of the magnified linear combinations out of range (above 24)"); return 0; }
    y_level = top - shift[0]; c_level = top - shift[1];
    if (y_level < 0 || c_level < 0) { snprintf(msg, msg_size, "4:2:0: the blocks of the frame are smaller than the reduction"); return 0; }
    for (s = w->basis_states; s < w->states; s++) {
        if (s == w->root_state || s == r0 || s == r1) continue;
        band = s <= root[0] ? 0 : s <= root[1] ? 1 : 2;
        if ((int) w->level_of_state[s] == (band ? c_level : y_level)) found[band] = 1;
    }
    if (!found[0]) {
        snprintf(msg, msg_size, "4:2:0: max_level %d at magnification %d takes Y states of level %d, the Y root has level %u: the "
                 "reference's Y plane stays zero there", top, magnify, y_level, (unsigned) w->level_of_state[root[0]]);
        return 0;
    }
    if (!found[1] || !found[2]) {
        snprintf(msg, msg_size, "4:2:0: max_level %d at magnification %d takes chroma states of level %d, the chroma root has level %u: "
                 "the reference's chroma planes stay zero there", top, magnify, c_level, (unsigned) w->level_of_state[root[found[1] ? 2 : 1]]);
        return 0;
    }
    plan->max_level = (unsigned) top; plan->y_level = (unsigned) y_level; plan->c_level = (unsigned) c_level;
    return 1;
}

/* the list smooth_image walks on the automaton enlarge_image has shifted for FORMAT_4_2_0 */
static unsigned borders_420(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap,
                            const char *who, int intra)
{
    unsigned mw = width, mh = height, low = 0, n;
    int low_mag = 0;
    fa_420_plan plan;
    char msg[200];
    if (magnify && !fiasco_amd_magnified_size(width, height, magnify, &mw, &mh)) return 0;
    /* the plan refuses what decode_image leaves zero; a P/B frame whose residual lacks a band is such a frame by right
     * (fa_smoothing_borders_420_residual): its borders are those of its partition all the same */
    if (!color) { fa_set_error("%s: 4:2:0: a gray frame has no chroma bands", who); return 0; }
    if (intra && !fa_420_plan_of(w, color, magnify, &plan, msg, sizeof msg)) { fa_set_error("%s: %s", who, msg); return 0; }
    if (magnify > 8) { fa_set_error("%s: magnification %d: the borders of the frame do not fit 16-bit coordinates", who, magnify); return 0; }
    n = borders_at(w, mw, mh, color, magnify, magnify - 1, out, cap, &low, &low_mag);
    if (low) {
        fa_set_error("%s: in 4:2:0 at magnification %d a smoothed state of level %u falls to level %d (below 1), where the "
                     "reference's own result is undefined", who, magnify, low - 1, (int) low - 1 + 2 * low_mag);
        return 0;
    }
    return n;
}

unsigned fa_smoothing_borders_420(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{
    return borders_420(w, width, height, color, magnify, out, cap, "smoothing borders", 1);
}

unsigned fa_smoothing_borders_420_residual(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{
    return borders_420(w, width, height, color, magnify, out, cap, "smoothing borders", 0);
}

int fiasco_amd_batch_smoothing_borders_420(const fiasco_amd_batch_t *b, unsigned i, int magnify, fiasco_amd_border *out, unsigned cap)
{
    const fa_job *job = finished_intra(b, i, 1, "fiasco_amd_batch_smoothing_borders_420", "", 0);
    char who[80];
    if (!job) return 0;
    snprintf(who, sizeof who, "fiasco_amd_batch_smoothing_borders_420: frame %u", i);
    return (int) borders_420(job->wfa, job->image->width, job->image->height, job->image->color, magnify, out, cap, who, 1);
}

int fiasco_amd_batch_decode_planes_420(const fiasco_amd_batch_t *b, unsigned i, int magnify, int16_t *out)
{
    const char *who = "fiasco_amd_batch_decode_planes_420";
    const fa_job *job = finished_intra(b, i, out != NULL, who, NEEDS_REFERENCES, 0);
    unsigned w, h;
    size_t npix, cpix;
    fa_420_plan plan;
    fa_dec_job d;
    char msg[200];
    if (!job) return 0;
    w = job->image->width; h = job->image->height;
    if (magnify && !fiasco_amd_magnified_size(w, h, magnify, &w, &h)) return 0;
    if (!fa_420_plan_of(job->wfa, job->image->color, magnify, &plan, msg, sizeof msg)) { fa_set_error("%s: frame %u: %s", who, i, msg); return 0; }
    fa_dec_job_of(job, magnify, &d);
    d.format_420 = 1;
    if (fa_core_decode_frames(1, &d) != 1 || !d.out) {
        fa_set_error("%s", d.errmsg[0] ? d.errmsg : "decoder failed");
        return 0;
    }
    if (!d.out_420 || d.out->width != w || d.out->height != h) {
        fa_set_error("%s: the decoder of this library (%s) does not decode 4:2:0: it handed back a 4:4:4 frame of %u x %u pixels",
                     who, fa_core_name(), d.out->width, d.out->height);
        fa_image_free(d.out);
        return 0;
    }
    npix = (size_t) w * h; cpix = (size_t) (w >> 1) * (h >> 1);
    memcpy(out, d.out->pixels[0], npix * 2);
    memcpy(out + npix, d.out->pixels[1], cpix * 2);
    memcpy(out + npix + cpix, d.out->pixels[2], cpix * 2);
    fa_image_free(d.out);
    return 1;
}
