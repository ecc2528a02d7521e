/*
 *  fa_render.c -- the reference's renderer (lib/dither.c) restated: a handle with its parameters, the size of the
 *  surface, and the plain loop from 12.4 planes to the pixels of an XImage (include/libfiasco_amd_render.h has the
 *  arithmetic and the refusals).  Host code without a device; the kernel (hip/render.inc) is the other statement of the
 *  same arithmetic and is compared with this one.
 *
 *  Where the reference indexes tables, this file computes: a table entry is a pure function of its index, and the end
 *  values the reference repeats beyond its defined ranges are clamps.
 */
#include <stdlib.h>
#include <string.h>
#include "fa_host.h"
#include "libfiasco_amd_render.h"
#include "libfiasco_amd_render_420.h"

/* bits set / zero bits below, and whether the mask is one run of at most 8 bits inside `bpp' bits */
static int mask_shape(unsigned long mask, unsigned bpp, unsigned *bits, unsigned *below)
{
    unsigned n = 0, s = 0;
    if (!mask || (bpp < 8 * sizeof mask && (mask >> bpp))) return 0;
    while (!(mask & 1)) { mask >>= 1; s++; }
    while (mask & 1) { mask >>= 1; n++; }
    if (mask || n > 8) return 0;
    *bits = n; *below = s;
    return 1;
}

fiasco_amd_renderer_t *fiasco_amd_renderer_new(unsigned long red_mask, unsigned long green_mask, unsigned long blue_mask, unsigned bpp,
                                               int double_resolution)
{
    unsigned nr, ng, nb, sr, sg, sb;
    fiasco_amd_renderer_t *r;
    if (bpp != 16 && bpp != 24 && bpp != 32) {
        fa_set_error("Rendering depth of XImage must be 16, 24, or 32 bpp.");
        return NULL;
    }
    if (!mask_shape(red_mask, bpp, &nr, &sr) || !mask_shape(green_mask, bpp, &ng, &sg) || !mask_shape(blue_mask, bpp, &nb, &sb)) {
        fa_set_error("fiasco_amd_renderer_new: masks %lx, %lx, %lx: every colour mask must be one run of 1 .. 8 bits inside the %u bits of a pixel.",
                     red_mask, green_mask, blue_mask, bpp);
        return NULL;
    }
    r = calloc(1, sizeof *r);
    if (!r) { fa_set_error("Out of memory."); return NULL; }
    r->bpp = bpp; r->doubled = double_resolution ? 1 : 0; r->rgb = red_mask > green_mask;
    r->r_drop = 8 - nr; r->g_drop = 8 - ng; r->b_drop = 8 - nb;
    r->r_up = sr; r->g_up = sg; r->b_up = sb;
    return r;
}

void fiasco_amd_renderer_delete(fiasco_amd_renderer_t *r) { free(r); }

int fiasco_amd_renderer_surface_size(const fiasco_amd_renderer_t *r, unsigned width, unsigned height, int color, unsigned *out_width,
                                     unsigned *out_height, size_t *row_bytes)
{
    if (!r) { fa_set_error("Parameter `%s' not defined (NULL).", "renderer"); return 0; }
    if (!width || !height || width > FA_RENDER_MAX_SIDE || height > FA_RENDER_MAX_SIDE) {
        fa_set_error("fiasco_amd_renderer: a frame of %u x %u pixels (1 .. %u each way).", width, height, (unsigned) FA_RENDER_MAX_SIDE);
        return 0;
    }
    /* the reference's loops count pixel pairs and quadruples: where they leave the end of the surface unwritten */
    if (r->bpp == 24 && !r->doubled && ((size_t) width * height & 3)) {
        fa_set_error("fiasco_amd_renderer: 24 bpp: %u x %u pixels are not a multiple of 4 (the reference leaves the last ones unwritten).", width, height);
        return 0;
    }
    if (r->bpp == 24 && r->doubled && (width & 1)) {
        fa_set_error("fiasco_amd_renderer: 24 bpp doubled: the width %u is odd (the reference leaves the last pixel of every row unwritten).", width);
        return 0;
    }
    if (r->bpp == 16 && !r->doubled && !color && ((size_t) width * height & 1)) {
        fa_set_error("fiasco_amd_renderer: 16 bpp gray: %u x %u pixels are an odd number (the reference leaves the last one unwritten).", width, height);
        return 0;
    }
    if (out_width) *out_width = width << r->doubled;
    if (out_height) *out_height = height << r->doubled;
    if (row_bytes) *row_bytes = (size_t) (width << r->doubled) * (r->bpp / 8);
    return 1;
}

static unsigned clip255(int v) { return (unsigned) (v < 0 ? 0 : v > 255 ? 255 : v); }
static int clamp_chroma(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }

/* the pixel of yval and two clamped chroma values as its `bytes' bytes in memory */
static void pixel_bytes(const fiasco_amd_renderer_t *r, int color, int yval, int cb, int cr, unsigned char px[4])
{
    int R = yval, G = yval, B = yval;
    if (color) {
        /* lib/dither.c:155-158: double arithmetic, C truncation (this file is built with -ffp-contract=off) */
        R = yval + (int) ( 1.4022 * cr + 0.5);
        G = yval + (int) (-0.7145 * cr + 0.5) + (int) (-0.3456 * cb + 0.5);
        B = yval + (int) ( 1.7710 * cb + 0.5);
    }
    px[0] = px[1] = px[2] = px[3] = 0;
    if (r->bpp == 24) {
        px[0] = (unsigned char) clip255(r->rgb ? R : B); px[1] = (unsigned char) clip255(G); px[2] = (unsigned char) clip255(r->rgb ? B : R);
    } else {
        /* blue is not shifted (lib/dither.c:205-208) */
        const unsigned v = ((clip255(R) >> r->r_drop) << r->r_up) | ((clip255(G) >> r->g_drop) << r->g_up) | (clip255(B) >> r->b_drop);
        px[0] = (unsigned char) v; px[1] = (unsigned char) (v >> 8); px[2] = (unsigned char) (v >> 16); px[3] = (unsigned char) (v >> 24);
    }
}

int fiasco_amd_renderer_render_planes(const fiasco_amd_renderer_t *r, const int16_t *planes, int color, unsigned width, unsigned height,
                                      unsigned char *out)
{
    size_t row = 0;
    if (!planes || !out) { fa_set_error("fiasco_amd_renderer_render_planes: no planes or no surface"); return 0; }
    if (!fiasco_amd_renderer_surface_size(r, width, height, color, NULL, NULL, &row)) return 0;
    const size_t npix = (size_t) width * height;
    const unsigned bytes = r->bpp / 8, dup = r->doubled + 1;
    for (unsigned y = 0; y < height; y++) {
        unsigned char *q = out + (size_t) y * dup * row;
        for (unsigned x = 0; x < width; x++) {
            const size_t at = (size_t) y * width + x;
            const int yval = (planes[at] >> 4) + 128;
            unsigned char px[4];
            pixel_bytes(r, color, yval, color ? clamp_chroma(planes[npix + at] >> 4) : 0, color ? clamp_chroma(planes[2 * npix + at] >> 4) : 0, px);
            for (unsigned k = 0; k < dup; k++) memcpy(q + ((size_t) x * dup + k) * bytes, px, bytes);
        }
        if (dup == 2) memcpy(q + row, q, row);
    }
    return 1;
}

/* ------------------------------------------------------------------ 4:2:0 (include/libfiasco_amd_render_420.h) */

int fiasco_amd_renderer_surface_size_420(const fiasco_amd_renderer_t *r, unsigned width, unsigned height, unsigned *out_width,
                                         unsigned *out_height, size_t *row_bytes)
{
    if (!r) { fa_set_error("Parameter `%s' not defined (NULL).", "renderer"); return 0; }
    if (!width || !height || width > FA_RENDER_MAX_SIDE || height > FA_RENDER_MAX_SIDE) {
        fa_set_error("fiasco_amd_renderer: a frame of %u x %u pixels (1 .. %u each way).", width, height, (unsigned) FA_RENDER_MAX_SIDE);
        return 0;
    }
    /* the reference's 4:2:0 loops count pixel pairs and row pairs */
    if ((width | height) & 1) {
        fa_set_error("fiasco_amd_renderer: 4:2:0: %u x %u pixels: the width or the height is odd (the reference renders pixel pairs of row pairs).", width, height);
        return 0;
    }
    /* ... and at 24 bpp quadruples of a row, by which they walk the chroma pointers as well */
    if (r->bpp == 24 && !r->doubled && (width & 3)) {
        fa_set_error("fiasco_amd_renderer: 4:2:0 at 24 bpp: the width %u is not a multiple of 4 (the reference's rows fall out of step with its chroma planes).", width);
        return 0;
    }
    if (out_width) *out_width = width << r->doubled;
    if (out_height) *out_height = height << r->doubled;
    if (row_bytes) *row_bytes = (size_t) (width << r->doubled) * (r->bpp / 8);
    return 1;
}

int fiasco_amd_renderer_render_planes_420(const fiasco_amd_renderer_t *r, const int16_t *y, const int16_t *cb, const int16_t *cr,
                                          unsigned width, unsigned height, unsigned char *out)
{
    size_t row = 0;
    if (!y || !cb || !cr || !out) { fa_set_error("fiasco_amd_renderer_render_planes_420: no planes or no surface"); return 0; }
    if (!fiasco_amd_renderer_surface_size_420(r, width, height, NULL, NULL, &row)) return 0;
    const unsigned bytes = r->bpp / 8, dup = r->doubled + 1, cw = width >> 1;
    for (unsigned yy = 0; yy < height; yy++) {
        unsigned char *q = out + (size_t) yy * dup * row;
        for (unsigned x = 0; x < width; x++) {
            const size_t c = (size_t) (yy >> 1) * cw + (x >> 1);
            unsigned char px[4];
            pixel_bytes(r, 1, (y[(size_t) yy * width + x] >> 4) + 128, clamp_chroma(cb[c] >> 4), clamp_chroma(cr[c] >> 4), px);
            for (unsigned k = 0; k < dup; k++) memcpy(q + ((size_t) x * dup + k) * bytes, px, bytes);
        }
        if (dup == 2) memcpy(q + row, q, row);
    }
    return 1;
}
