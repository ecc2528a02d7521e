/*
 *  stream_check.c -- the stream reader on the host, stand-alone: built by tests/test_stream_check.py with
 *  -fsanitize=address,undefined from the product's fa_reader.c, fa_stream.c, fa_bitio.c, fa_wfa.c, fa_writer.c, fa_rpf.c,
 *  fa_error.c and the test oracle's host decoder (oracle/oracle_decoder.c).  The decoder of the walk is that host decoder
 *  here (fa_core_decode_frames below), so fiasco_amd_stream_decode_planes() runs on the CPU at magnification 0.
 *
 *    stream_check decode DIR a.fco ...   every frame of every stream as DIR/<name>.<display>.i16 (12.4 planes, unsmoothed),
 *                                        and one line "<name> <frames> <types>" each
 *    stream_check mutate a.fco N         every prefix of the stream (N == 0) or of nothing, and every single-bit flip of
 *                                        its first N bytes (0: all): each must be refused, or give a stream that is
 *                                        written again and decoded without a report of the sanitizers (a prefix that
 *                                        lacks only bits no section reads is a stream)
 *    stream_check offsets a.fco          the byte offset of every frame
 *    stream_check wrap a.fco out.fco     the stream with one block per type and P/B frame moved over the right edge of the
 *                                        frame (for tests/golden/make_decoded_streams.py)
 *    stream_check mc                     dec_mc_scaled / dec_mc420_item (csrc/hip/dec_mc.h) against loops written from
 *                                        the text of enlarge_image and restore_mc
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "fa_host.h"
#include "libfiasco_amd_stream.h"
#include "dec_mc.h"

/* ------------------------------------------------------------------ what the product's other files would bring */

void fa_limits(unsigned *max_states, unsigned *max_level) { *max_states = FA_STOCK_STATES; *max_level = FA_STOCK_LEVEL; }
void fa_info_free(fa_info *wi) { free(wi->basis_name); free(wi->title); free(wi->comment); wi->basis_name = wi->title = wi->comment = NULL; }
const char *fa_core_name(void) { return "host-check"; }
void fa_core_release_dev(void *dev, int dev_id) { (void) dev; (void) dev_id; }

fa_image *fa_image_alloc(unsigned width, unsigned height, int color)
{
    fa_image *im = (fa_image *) calloc(1, sizeof *im);
    int b;
    if (!im) return NULL;
    im->width = width; im->height = height; im->color = color;
    for (b = 0; b < (color ? 3 : 1); b++)
        if (!(im->pixels[b] = (int16_t *) calloc((size_t) width * height, sizeof(int16_t)))) { fa_image_free(im); return NULL; }
    return im;
}

void fa_image_free(fa_image *im)
{
    int b;
    if (!im) return;
    for (b = 0; b < 3; b++) free(im->pixels[b]);
    free(im);
}

unsigned fa_smoothing_borders(const fa_wfa *w, unsigned width, unsigned height, int color, fiasco_amd_border *out, unsigned cap)
{ (void) w; (void) width; (void) height; (void) color; (void) out; (void) cap; fa_set_error("no border lists in this program"); return 0; }
unsigned fa_smoothing_borders_magnified(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{ (void) magnify; return fa_smoothing_borders(w, width, height, color, out, cap); }
unsigned fa_smoothing_borders_420(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{ (void) magnify; return fa_smoothing_borders(w, width, height, color, out, cap); }
unsigned fa_smoothing_borders_420_residual(const fa_wfa *w, unsigned width, unsigned height, int color, int magnify, fiasco_amd_border *out, unsigned cap)
{ (void) magnify; return fa_smoothing_borders(w, width, height, color, out, cap); }
int fiasco_amd_magnified_size(unsigned width, unsigned height, int magnify, unsigned *out_w, unsigned *out_h)
{ (void) width; (void) height; (void) magnify; (void) out_w; (void) out_h; fa_set_error("no magnification in this program"); return 0; }

/* the seam, on the host: decode_image, and restore_mc for a P/B frame -- what the test oracle's core does */
int fa_core_decode_frames(unsigned n, fa_dec_job *jobs)
{
    unsigned i;
    int good = 0;
    for (i = 0; i < n; i++) {
        fa_dec_job *j = &jobs[i];
        j->out = NULL; j->errmsg[0] = 0;
        if (j->skip) continue;
        if (j->magnify || j->format_420 || j->smoothing) { snprintf(j->errmsg, sizeof j->errmsg, "the host decoder decodes 4:4:4 at the coded size"); continue; }
        if (j->frame_type != FA_I_FRAME) {
            /* as the device decoder: a vector needs its frame */
            const unsigned root = j->color ? (unsigned) FA_TREE(j->wfa, (unsigned) FA_TREE(j->wfa, j->wfa->root_state, 0), 0) : j->wfa->root_state;
            unsigned s, l;
            int lacks = 0;
            for (s = j->wfa->basis_states; s <= root; s++)
                for (l = 0; l < 2; l++) {
                    const int t = j->wfa->mv[s * 2 + l].type;
                    lacks = lacks || (t != FA_MV_NONE && ((t != FA_MV_BACKWARD && !j->past) || (t != FA_MV_FORWARD && !j->future)));
                }
            if (lacks) { snprintf(j->errmsg, sizeof j->errmsg, "device decoder: motion vector without its reference frame"); continue; }
        }
        j->out = fa_decode_image(j->width, j->height, j->wfa, j->color);
        if (j->out && j->frame_type != FA_I_FRAME && !fa_restore_mc(j->out, j->past, j->future, j->wfa, j->p_max_level)) {
            fa_image_free(j->out);
            j->out = NULL;
        }
        if (!j->out) snprintf(j->errmsg, sizeof j->errmsg, "%s", fiasco_get_error_message());
        else good++;
    }
    return good;
}

/* ------------------------------------------------------------------ decode */

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

static const char *base_of(const char *path, char *buf, size_t n)
{
    const char *b = strrchr(path, '/');
    char *dot;
    snprintf(buf, n, "%s", b ? b + 1 : path);
    if ((dot = strrchr(buf, '.'))) *dot = 0;
    return buf;
}

static int decode_streams(const char *dir, int argc, char **argv)
{
    int a;
    for (a = 0; a < argc; a++) {
        size_t len;
        unsigned char *data = read_file(argv[a], &len), *again = NULL;
        fiasco_amd_stream_t *s = fiasco_amd_stream_open(data, len);
        fiasco_amd_stream_info info;
        char name[200], path[600];
        unsigned d;
        size_t alen = 0;
        if (!s) { printf("%s REFUSED %s\n", base_of(argv[a], name, sizeof name), fiasco_get_error_message()); free(data); continue; }
        fiasco_amd_stream_get_info(s, &info);
        if (!fiasco_amd_stream_rewrite(s, &again, &alen) || alen != len || memcmp(again, data, len)) {
            fprintf(stderr, "%s: written again, the stream differs\n", argv[a]);
            return 1;
        }
        free(again);
        printf("%s %u", base_of(argv[a], name, sizeof name), info.frames);
        for (d = 0; d < info.frames; d++) {
            const size_t vals = (size_t) info.width * info.height * (info.color ? 3 : 1);
            int16_t *planes = (int16_t *) malloc(vals * 2);
            FILE *f;
            printf(" %d", fiasco_amd_stream_frame_type(s, d));
            if (!fiasco_amd_stream_decode_planes(s, d, 0, planes)) { printf(" FAILED %s\n", fiasco_get_error_message()); free(planes); break; }
            snprintf(path, sizeof path, "%s/%s.%u.i16", dir, name, d);
            f = fopen(path, "wb");
            if (!f || fwrite(planes, 2, vals, f) != vals) { fprintf(stderr, "%s: cannot be written\n", path); return 2; }
            fclose(f);
            free(planes);
        }
        printf("\n");
        fiasco_amd_stream_free(s);
        free(data);
    }
    return 0;
}

/* ------------------------------------------------------------------ mutate */

static unsigned long accepted, refused, decoded;

/* one mutated stream: refused, or written again and decoded frame by frame.  What the decoder refuses (a vector without
 * its frame, a half-pixel stream) is a refusal too; only the sanitizers fail this program */
static void try_stream(const unsigned char *data, size_t len)
{
    fiasco_amd_stream_t *s = fiasco_amd_stream_open(data, len);
    fiasco_amd_stream_info info;
    unsigned char *again = NULL;
    size_t alen = 0;
    unsigned d;
    if (!s) {
        if (!fiasco_get_error_message()[0]) { fprintf(stderr, "a refusal without a message\n"); exit(1); }
        refused++;
        return;
    }
    accepted++;
    fiasco_amd_stream_get_info(s, &info);
    if (fiasco_amd_stream_rewrite(s, &again, &alen)) free(again);
    if ((unsigned long long) info.width * info.height <= 512ull * 512ull)
        for (d = 0; d < info.frames; d++) {
            const size_t vals = (size_t) info.width * info.height * (info.color ? 3 : 1);
            int16_t *planes = (int16_t *) malloc(vals * 2);
            if (planes && fiasco_amd_stream_decode_planes(s, d, 0, planes)) decoded++;
            free(planes);
        }
    fiasco_amd_stream_free(s);
}

static int mutate(const char *file, unsigned long nflip)
{
    size_t len, i;
    unsigned char *data = read_file(file, &len), *copy;
    unsigned bit;
    fiasco_set_verbosity(FIASCO_NO_VERBOSITY);
    if (!nflip) {
        for (i = 0; i < len; i++) {             /* a prefix in a buffer of exactly its size: a read behind it is a report */
            copy = (unsigned char *) malloc(i ? i : 1);
            memcpy(copy, data, i);
            try_stream(copy, i);
            free(copy);
        }
    }
    if (!nflip || nflip > len) nflip = len;
    copy = (unsigned char *) malloc(len);
    for (i = 0; i < nflip; i++)
        for (bit = 0; bit < 8; bit++) {
            memcpy(copy, data, len);
            copy[i] ^= (unsigned char) (1u << bit);
            try_stream(copy, len);
        }
    free(copy);
    try_stream(data, len);
    printf("%s: %lu refused, %lu accepted, %lu frames decoded\n", file, refused, accepted, decoded);
    free(data);
    return accepted ? 0 : 1;                    /* the stream itself is accepted */
}

static int offsets(const char *file)
{
    size_t len;
    unsigned char *data = read_file(file, &len);
    fa_bitr in;
    fa_info wi;
    fa_wfa *basis = fa_wfa_alloc(FA_STOCK_STATES + 8);
    unsigned k;
    fa_br_init(&in, data, len);
    if (!basis || !fa_read_header(&in, file, &wi) || !fa_load_basis(wi.basis_name, basis)) { fprintf(stderr, "%s\n", fiasco_get_error_message()); return 1; }
    for (k = 0; k < wi.frames; k++) {
        unsigned number;
        int flags[3];
        const size_t at = in.pos / 8;
        fa_wfa *w = fa_read_frame(&in, &wi, basis, &number, flags);
        if (!w) { fprintf(stderr, "%s\n", fiasco_get_error_message()); return 1; }
        printf("%lu %u %d\n", (unsigned long) at, number, w->frame_type);
        {   /* its motion blocks: "mv <display> <x> <y> <level> <type> <fx> <fy> <bx> <by>" */
            const unsigned root = wi.color ? (unsigned) FA_TREE(w, (unsigned) FA_TREE(w, w->root_state, 0), 0) : w->root_state;
            unsigned s, l;
            for (s = w->basis_states; s <= root; s++)
                for (l = 0; l < 2; l++) {
                    const fa_mv *mv = &w->mv[s * 2 + l];
                    if (mv->type != FA_MV_NONE)
                        printf("mv %u %u %u %d %d %d %d %d %d\n", number, (unsigned) w->x[s * 2 + l], (unsigned) w->y[s * 2 + l],
                               (int) w->level_of_state[s] - 1, (int) mv->type, (int) mv->fx, (int) mv->fy, (int) mv->bx, (int) mv->by);
                }
        }
        fa_wfa_free(w);
    }
    printf("%lu end\n", (unsigned long) ((in.pos + 7) / 8));
    fa_wfa_free(basis); fa_info_free(&wi); free(data);
    return 0;
}

/* A stream no coder writes, for the fixture: in every P and B frame of `file', per block type, the block that lies
 * furthest to the right (two rows clear of the top and the bottom of the frame) gets a horizontal vector that carries it 3
 * pixels over the right edge of the frame and a vertical one of -1: the decoders address linearly, the block comes back in on
 * the left of the next row and stays inside the plane.  Everything else is written again as it was read */
static int wrap(const char *file, const char *out_name)
{
    size_t len;
    unsigned char *data = read_file(file, &len);
    fa_bitr in;
    fa_bitw out;
    fa_info wi;
    fa_wfa *basis = fa_wfa_alloc(FA_STOCK_STATES + 8);
    unsigned k, changed = 0;
    FILE *f;
    fa_br_init(&in, data, len);
    if (!basis || !fa_read_header(&in, file, &wi) || !fa_load_basis(wi.basis_name, basis)) { fprintf(stderr, "%s\n", fiasco_get_error_message()); return 1; }
    fa_bw_init(&out);
    for (k = 0; k < wi.frames; k++) {
        unsigned number, s, l;
        int flags[3], t;
        fa_wfa *w = fa_read_frame(&in, &wi, basis, &number, flags);
        if (!w) { fprintf(stderr, "%s\n", fiasco_get_error_message()); return 1; }
        for (t = FA_MV_FORWARD; t <= FA_MV_INTERPOLATED && w->frame_type != FA_I_FRAME; t++) {
            const unsigned root = wi.color ? (unsigned) FA_TREE(w, (unsigned) FA_TREE(w, w->root_state, 0), 0) : w->root_state;
            fa_mv *best = NULL;
            unsigned best_right = 0;
            for (s = w->basis_states; s <= root; s++)
                for (l = 0; l < 2; l++) {
                    fa_mv *mv = &w->mv[s * 2 + l];
                    const unsigned lv = (unsigned) w->level_of_state[s] - 1, x = w->x[s * 2 + l], y = w->y[s * 2 + l];
                    const unsigned right = x + fa_width_of_level(lv);
                    if (mv->type != t || y < 2 || y + fa_height_of_level(lv) + 2 > wi.height || right > wi.width) continue;
                    if (wi.width - right + 3 > wi.search_range || right <= best_right) continue;
                    best = mv; best_right = right;
                }
            if (!best) continue;
            if (t == FA_MV_BACKWARD) { best->bx = (int16_t) (wi.width - best_right + 3); best->by = -1; }
            else { best->fx = (int16_t) (wi.width - best_right + 3); best->fy = -1; }
            printf("frame %u: a block of type %d now ends at column %u of %u\n", number, t, wi.width + 3, wi.width);
            changed++;
        }
        if (!fa_write_frame(w, &wi, w->frame_type, number, flags[0], flags[1], flags[2], &out)) { fprintf(stderr, "%s\n", fiasco_get_error_message()); return 1; }
        fa_wfa_free(w);
    }
    f = fopen(out_name, "wb");
    if (!f || fwrite(out.buf, 1, fa_bw_finish(&out), f) != fa_bw_finish(&out)) { fprintf(stderr, "%s: cannot be written\n", out_name); return 2; }
    fclose(f);
    fa_bw_free(&out); fa_wfa_free(basis); fa_info_free(&wi); free(data);
    return changed ? 0 : 1;
}

/* ------------------------------------------------------------------ mc */

typedef struct block { unsigned x, y; int level, type, fx, fy, bx, by; } block;

/* enlarge_image (codec/decoder.c:804-835) on one block, from its text */
static void enlarge_block(block *b, int factor)
{
    int n;
    b->level = b->level + factor * 2;
    if (factor > 0) {
        b->x <<= factor; b->y <<= factor;
        for (n = factor; n; n--) { b->fx = (int16_t) (b->fx * 2); b->fy = (int16_t) (b->fy * 2); b->bx = (int16_t) (b->bx * 2); b->by = (int16_t) (b->by * 2); }
    } else {
        b->x >>= -factor; b->y >>= -factor;
        for (n = -factor; n; n--) { b->fx /= 2; b->fy /= 2; b->bx /= 2; b->by /= 2; }
    }
}

#define FXV(v) (band ? ((v) / 2) : (v))
/* restore_mc (codec/motion.c:65-188) for one block of a 4:2:0 frame, from its text: extract_mc_block copies rows of the
 * reference, the sums go into the image with the row offset of the band */
static void restore_block(const block *b, int16_t *const image[3], int16_t *const past[3], int16_t *const future[3], unsigned W)
{
    int band;
    for (band = 0; band < 3; band++) {
        const int width = FXV((int) fa_width_of_level(b->level)), height = FXV((int) fa_height_of_level(b->level));
        const int ref_width = FXV((int) W), xo = FXV((int) b->x), yo = FXV((int) b->y);
        int16_t *orig = image[band] + xo + yo * ref_width;
        const int16_t *r1 = NULL, *r2 = NULL;
        int x, y;
        if (b->type != FA_MV_BACKWARD) r1 = past[band] + (yo + FXV(b->fy)) * ref_width + (xo + FXV(b->fx));
        if (b->type != FA_MV_FORWARD) r2 = future[band] + (yo + FXV(b->by)) * ref_width + (xo + FXV(b->bx));
        for (y = 0; y < height; y++)
            for (x = 0; x < width; x++) {
                const int a = r1 ? r1[y * ref_width + x] : 0, c = r2 ? r2[y * ref_width + x] : 0;
                const int add = b->type == FA_MV_INTERPOLATED ? (a + c) >> 1 : b->type == FA_MV_FORWARD ? a : c;
                orig[y * ref_width + x] = (int16_t) (uint16_t) ((unsigned) orig[y * ref_width + x] + (unsigned) add);
            }
    }
}

static int mc_check(void)
{
    /* coded blocks of a 16 x 12 frame (every one inside its plane after every scaling tried): vectors of -1, -3 and +3, a
     * block at the last column, levels that come out as 0 and 1 after a reduction by one step */
    static const block coded[] = {
        { 4, 4, 4, FA_MV_FORWARD, -1, -3, 0, 0 }, { 8, 4, 3, FA_MV_BACKWARD, 0, 0, 3, -1 }, { 4, 8, 4, FA_MV_INTERPOLATED, -3, -1, 3, -3 },
        { 12, 0, 4, FA_MV_FORWARD, 3, 3, 0, 0 }, { 14, 8, 2, FA_MV_FORWARD, -3, -3, 0, 0 }, { 8, 8, 3, FA_MV_INTERPOLATED, -1, -3, -3, -1 },
        { 0, 2, 2, FA_MV_BACKWARD, 0, 0, 3, 3 },
    };
    const unsigned nblocks = sizeof coded / sizeof coded[0];
    int mag, bad = 0;
    for (mag = -1; mag <= 1; mag++) {
        const unsigned W = mag > 0 ? 32 : mag < 0 ? 8 : 16, H = mag > 0 ? 24 : mag < 0 ? 6 : 12;
        const size_t npix = (size_t) W * H, cpix = (size_t) (W >> 1) * (H >> 1), vals = npix + 2 * cpix;
        int16_t *a = (int16_t *) calloc(vals, 2), *b = (int16_t *) calloc(vals, 2), *p = (int16_t *) malloc(vals * 2), *f = (int16_t *) malloc(vals * 2);
        int16_t *ia[3] = { a, a + npix, a + npix + cpix }, *ip[3] = { p, p + npix, p + npix + cpix }, *ifu[3] = { f, f + npix, f + npix + cpix };
        unsigned k, band, px, seed = 12345u + (unsigned) (mag + 1);
        size_t v;
        for (v = 0; v < vals; v++) { seed = seed * 1103515245u + 12345u; p[v] = (int16_t) (seed >> 16); seed = seed * 1103515245u + 12345u; f[v] = (int16_t) (seed >> 16); }
        for (k = 0; k < nblocks; k++) {
            block e = coded[k];
            DecMc m;
            const int ok = dec_mc_scaled(&m, coded[k].x, coded[k].y, coded[k].level, coded[k].type, coded[k].fx, coded[k].fy, coded[k].bx, coded[k].by, mag);
            enlarge_block(&e, mag);
            if (mag) { if (!ok != (e.level < 0)) { printf("mc: block %u at %d: refusal\n", k, mag); bad = 1; } }
            if (!ok) continue;
            if (m.x0 != (int) e.x || m.y0 != (int) e.y || m.level != e.level || m.fx != e.fx || m.fy != e.fy || m.bx != e.bx || m.by != e.by) {
                printf("mc: block %u at %d: scaled block differs\n", k, mag);
                bad = 1;
            }
            restore_block(&e, ia, ip, ifu, W);
            for (band = 0; band < 3; band++)
                for (px = 0; px < (1u << m.level); px++) {
                    unsigned long long base;
                    long long np, di, fi, bi;
                    int add;
                    if (!dec_mc420_item(&m, band, px, W, H, &base, &np, &di, &fi, &bi)) continue;
                    if (di < 0 || di >= np || (m.type != FA_MV_BACKWARD && (fi < 0 || fi >= np)) || (m.type != FA_MV_FORWARD && (bi < 0 || bi >= np))) {
                        printf("mc: block %u at %d band %u: leaves its plane\n", k, mag, band);
                        bad = 1;
                        continue;
                    }
                    add = m.type == FA_MV_FORWARD ? p[base + fi] : m.type == FA_MV_BACKWARD ? f[base + bi] : ((int) p[base + fi] + (int) f[base + bi]) >> 1;
                    b[base + di] = (int16_t) (uint16_t) ((unsigned) b[base + di] + (unsigned) add);
                }
        }
        if (memcmp(a, b, vals * 2)) { printf("mc: magnification %d: the planes differ\n", mag); bad = 1; }
        else printf("mc: magnification %d: %u x %u, planes equal\n", mag, W, H);
        free(a); free(b); free(p); free(f);
    }
    return bad;
}

int main(int argc, char **argv)
{
    if (argc >= 4 && !strcmp(argv[1], "decode")) return decode_streams(argv[2], argc - 3, argv + 3);
    if (argc == 4 && !strcmp(argv[1], "mutate")) return mutate(argv[2], strtoul(argv[3], NULL, 10));
    if (argc == 3 && !strcmp(argv[1], "offsets")) return offsets(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "wrap")) return wrap(argv[2], argv[3]);
    if (argc == 2 && !strcmp(argv[1], "mc")) return mc_check();
    fprintf(stderr, "usage: stream_check decode DIR a.fco ... | mutate a.fco N | offsets a.fco | wrap a.fco out.fco | mc\n");
    return 2;
}
