/*
 *  decoder_cursor_check.c -- the cursor under fa_stream_walk (fa_cursor, csrc/host/fa_stream.c) on the host, stand-alone:
 *  built by tests/test_decoder_cursor_host.py with -fsanitize=address,undefined from the product's fa_reader.c, fa_stream.c,
 *  fa_bitio.c, fa_wfa.c, fa_writer.c, fa_rpf.c and fa_error.c.  No frame is decoded: the run callback below hands back
 *  tagged images without planes and keeps the books a decoder on the device could not.
 *
 *    decoder_cursor_check a.fco ...    every stream played display frame by display frame at read-ahead 1, 2, 3 and 32,
 *                                      and closed early once.  Checked, with exit status 1 and a line on stderr otherwise:
 *      - every coded frame is handed to run() exactly once per cursor;
 *      - the references of a P/B job are images run() made, alive at that moment, of jobs that kept their planes
 *        (keep_dev) -- the unsmoothed frame, whatever smoothing the wanted job carried;
 *      - the frames reach run() in the order of fa_stream_walk() over the whole stream, and every flight of the walk ends
 *        where a call of the cursor ends (at a read-ahead of 32, more than any stream here has frames, the calls ARE the
 *        walk's flights);
 *      - a frame run() fails is consumed, the frames predicted from it carry its cause, the others are decoded;
 *      - after the last frame was handed out, and after an early close, no image is alive.
 *    One line per stream on stdout: "<name> <frames> ok=<display frames decoded> failed=<d:cause;...>".
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fa_host.h"
#include "libfiasco_amd_stream.h"

/* ------------------------------------------------------------------ what the product's other files would bring */

void fa_limits(unsigned *max_states, unsigned *max_level) { *max_states = FA_STOCK_STATES; *max_level = FA_STOCK_LEVEL; }
void fa_info_free(fa_info *wi) { free(wi->basis_name); free(wi->title); free(wi->comment); wi->basis_name = wi->title = wi->comment = NULL; }
const char *fa_core_name(void) { return "cursor-check"; }
void fa_core_release_dev(void *dev, int dev_id) { (void) dev; (void) dev_id; }
int fa_core_decode_frames(unsigned n, fa_dec_job *jobs) { (void) n; (void) jobs; return 0; }
unsigned fa_smoothing_borders(const fa_wfa *w, unsigned width, unsigned height, int color, fiasco_amd_border *out, unsigned cap)
{ (void) w; (void) width; (void) height; (void) color; (void) out; (void) cap; return 0; }
unsigned fa_smoothing_borders_magnified(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{ (void) w; (void) width; (void) height; (void) color; (void) magnify; (void) out; (void) cap; return 0; }
unsigned fa_smoothing_borders_420(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{ (void) w; (void) width; (void) height; (void) color; (void) magnify; (void) out; (void) cap; return 0; }
unsigned fa_smoothing_borders_420_residual(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{ (void) w; (void) width; (void) height; (void) color; (void) magnify; (void) out; (void) cap; return 0; }
int fiasco_amd_magnified_size(unsigned width, unsigned height, int magnify, unsigned *out_w, unsigned *out_h)
{ (void) magnify; *out_w = width; *out_h = height; return 1; }

/* images are tagged, counted and listed: dev_id holds the display number, src_dev_id whether the job kept its planes */
#define MAXF 64
static fa_image *g_alive[4 * MAXF];
static unsigned g_nalive;

fa_image *fa_image_alloc(unsigned width, unsigned height, int color)
{
    fa_image *im = (fa_image *) calloc(1, sizeof *im);
    if (!im) return NULL;
    im->width = width; im->height = height; im->color = color;
    g_alive[g_nalive++] = im;
    return im;
}

void fa_image_free(fa_image *im)
{
    unsigned i;
    if (!im) return;
    for (i = 0; i < g_nalive && g_alive[i] != im; i++) ;
    if (i == g_nalive) { fprintf(stderr, "an image is freed that is not alive\n"); exit(1); }
    g_alive[i] = g_alive[--g_nalive];
    free(im);
}

static int alive(const fa_image *im)
{
    unsigned i;
    for (i = 0; i < g_nalive; i++) if (g_alive[i] == im) return 1;
    return 0;
}

/* ------------------------------------------------------------------ the books of one play */

typedef struct Play {
    unsigned calls[MAXF];               /* by display number: times handed to run() */
    unsigned order[4 * MAXF], norder;   /* display numbers as they reached run() */
    unsigned ends[4 * MAXF], nends;     /* norder after each call of run() */
    int bad;
} Play;

#define FAIL(P, ...) do { fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); (P)->bad = 1; } while (0)

/* as the device decoder: a vector needs its frame */
static int lacks_reference(const fa_dec_job *j)
{
    const unsigned root = j->color ? (unsigned) FA_TREE(j->wfa, (unsigned) FA_TREE(j->wfa, j->wfa->root_state, 0), 0) : j->wfa->root_state;
    unsigned s, l;
    int lacks = 0;
    for (s = j->wfa->basis_states; s <= root; s++)
        for (l = 0; l < 2; l++) {
            const int t = j->wfa->mv[s * 2 + l].type;
            lacks = lacks || (t != FA_MV_NONE && ((t != FA_MV_BACKWARD && !j->past) || (t != FA_MV_FORWARD && !j->future)));
        }
    return lacks;
}

static void fake_run(void *ctx, unsigned n, fa_dec_job *jobs, const unsigned *display, const uint8_t *wanted)
{
    Play *P = (Play *) ctx;
    unsigned i;
    int r;
    for (i = 0; i < n; i++) {
        fa_dec_job *j = &jobs[i];
        j->out = NULL; j->errmsg[0] = 0;
        if (display[i] >= MAXF) { FAIL(P, "display number %u", display[i]); continue; }
        P->calls[display[i]]++;
        P->order[P->norder++] = display[i];
        if (!j->from_stream || j->share_key != 1) FAIL(P, "frame %u: not a job of a walked stream", display[i]);
        if (!wanted[i] && j->smoothing) FAIL(P, "frame %u: smoothed and not wanted", display[i]);
        for (r = 0; r < 2 && j->frame_type != FA_I_FRAME; r++) {
            const fa_image *ref = r ? j->future : j->past;
            if (!ref) continue;
            if (!alive(ref)) { FAIL(P, "frame %u: its %s reference is not alive", display[i], r ? "future" : "past"); continue; }
            if (!ref->src_dev_id) FAIL(P, "frame %u: its %s reference (frame %d) did not keep its planes", display[i], r ? "future" : "past", ref->dev_id);
        }
        if (j->frame_type != FA_I_FRAME && lacks_reference(j)) { snprintf(j->errmsg, sizeof j->errmsg, "device decoder: motion vector without its reference frame"); continue; }
        j->out = fa_image_alloc(j->width, j->height, j->color);
        if (!j->out) { snprintf(j->errmsg, sizeof j->errmsg, "Out of memory!"); continue; }
        j->out->dev_id = (int) display[i]; j->out->src_dev_id = j->keep_dev;
    }
    P->ends[P->nends++] = P->norder;
}

static unsigned char *read_file(const char *name, size_t *len)
{
    FILE *f = fopen(name, "rb");
    unsigned char *buf;
    long n;
    if (!f) { fprintf(stderr, "%s: cannot be read\n", name); exit(2); }
    fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
    buf = (unsigned char *) malloc(n > 0 ? (size_t) n : 1);
    if (!buf || fread(buf, 1, (size_t) n, f) != (size_t) n) { fprintf(stderr, "%s: cannot be read\n", name); exit(2); }
    fclose(f);
    *len = (size_t) n;
    return buf;
}

static int check_stream(const char *path)
{
    static const unsigned ahead[] = { 1, 2, 3, 32 };
    size_t len;
    unsigned char *data = read_file(path, &len);
    fiasco_amd_stream_t *s = fiasco_amd_stream_open(data, len);
    const char *base = strrchr(path, '/') ? strrchr(path, '/') + 1 : path;
    Play walk;
    char (*errs)[160];
    unsigned n, a, d, i;
    int bad = 0, good;
    free(data);
    if (!s) { fprintf(stderr, "%s: %s\n", path, fiasco_get_error_message()); return 1; }
    n = fa_stream_info(s)->frames;
    if (n > MAXF) { fprintf(stderr, "%s: %u frames\n", path, n); fiasco_amd_stream_free(s); return 1; }
    /* the yardstick: fa_stream_walk over the whole stream */
    memset(&walk, 0, sizeof walk);
    errs = (char (*)[160]) calloc(n, 160);
    good = fa_stream_walk(s, "check", 0, n, NULL, 0, 35, 0, fake_run, &walk, 0, NULL, errs);
    bad = walk.bad;
    if (g_nalive) { fprintf(stderr, "%s: %u images alive behind the walk\n", base, g_nalive); bad = 1; }
    printf("%.*s %u ok=%d failed=", (int) (strrchr(base, '.') ? strrchr(base, '.') - base : (long) strlen(base)), base, n, good);
    for (d = 0; d < n; d++) if (errs[d][0]) printf("%u:%s;", d, errs[d]);
    printf("\n");

    for (a = 0; a < sizeof ahead / sizeof *ahead; a++) {
        Play P;
        fa_cursor *c = fa_cursor_open(s, "check", 0, n, NULL, 0, 35, 0, 0);
        unsigned w = 0;
        memset(&P, 0, sizeof P);
        if (!c) { fprintf(stderr, "%s: %s\n", base, fiasco_get_error_message()); bad = 1; break; }
        for (d = 0; d < n; d++) {
            const char *cause = "";
            int st;
            fa_cursor_advance(c, d, ahead[a], fake_run, &P);
            st = fa_cursor_status(c, d, &cause);
            if (st < 0) FAIL(&P, "%s, read-ahead %u: frame %u is not decoded behind its advance", base, ahead[a], d);
            if ((st == 0) != (errs[d][0] != 0) || (st == 0 && strcmp(cause, errs[d]))) FAIL(&P, "%s, read-ahead %u: frame %u: `%s', the walk says `%s'", base, ahead[a], d, cause, errs[d]);
        }
        if (fa_cursor_held(c) || g_nalive) FAIL(&P, "%s, read-ahead %u: %u images held, %u alive behind the last frame", base, ahead[a], fa_cursor_held(c), g_nalive);
        fa_cursor_close(c);
        for (d = 0; d < n; d++) {
            /* a frame whose reference failed never reaches run(): the walk agrees */
            if (P.calls[d] != walk.calls[d] || P.calls[d] > 1) FAIL(&P, "%s, read-ahead %u: frame %u reached run() %u times (the walk: %u)", base, ahead[a], d, P.calls[d], walk.calls[d]);
        }
        if (P.norder != walk.norder || memcmp(P.order, walk.order, P.norder * sizeof *P.order)) FAIL(&P, "%s, read-ahead %u: the frames reach run() in another order than in the walk", base, ahead[a]);
        /* every end of a flight of the walk is the end of a call of the cursor */
        for (i = 0; i < walk.nends; i++) {
            while (w < P.nends && P.ends[w] < walk.ends[i]) w++;
            if (w == P.nends || P.ends[w] != walk.ends[i]) { FAIL(&P, "%s, read-ahead %u: a call of the cursor spans two flights of the walk", base, ahead[a]); break; }
        }
        if (ahead[a] >= n && (P.nends != walk.nends || memcmp(P.ends, walk.ends, P.nends * sizeof *P.ends))) FAIL(&P, "%s, read-ahead %u: not the flights of the walk", base, ahead[a]);
        bad = bad || P.bad;
    }
    /* closed early: behind the first frame, with what was decoded ahead still held */
    {
        Play P;
        fa_cursor *c = fa_cursor_open(s, "check", 0, n, NULL, 0, -1, 0, 0);
        memset(&P, 0, sizeof P);
        if (c) fa_cursor_advance(c, 0, 2, fake_run, &P);
        fa_cursor_close(c);
        if (!c || P.bad || g_nalive) { fprintf(stderr, "%s: %u images alive behind an early close\n", base, g_nalive); bad = 1; }
    }
    free(errs);
    fiasco_amd_stream_free(s);
    return bad;
}

int main(int argc, char **argv)
{
    int a, bad = 0;
    for (a = 1; a < argc; a++) bad |= check_stream(argv[a]);
    return bad;
}
