/*
 *  render_step_check.cpp -- the rendering kernel of the device decoder (csrc/hip/render.inc, rd_render_kernel) replayed on
 *  the CPU, for the sanitizers.
 *
 *  A stand-alone program: it includes render.inc with RENDER_HOST_REPLAY defined -- the per-item function rd_item and what
 *  it calls (rd_pixels, rd_word, rd_emit, the store helper px_store_bytes_wide of px_access.inc) and the exchange inside a wave that the doubled build
 *  runs between two barriers (rd_wave_put, rd_wave_store) as plain C++, no HIP, no library, no device -- and is
 *  built by tests/test_render_step_host.py with -fsanitize=address,undefined and linked with csrc/host/fa_render.c, the
 *  plain host loop.
 *    frames     widths 1, 15, 16, 17, 18, 33 and 34, heights 1, 3 and 4, gray and colour, full-range values; the planes are
 *               heap blocks of exactly W x H values per band and an item loads only the values it owns
 *    surfaces   heap blocks of exactly the bytes the rows span, beginning at the block (16-byte aligned), one pixel into it
 *               and, at 24 bpp, one byte into it; packed, and with a pitch of 7 bytes (24 bpp) or a pixel and one more (16,
 *               32 bpp) above the row.  Every byte between two rows must keep its pattern
 *    renderers  all twelve: 565, 555, XRGB8888, the one with blue high, 24 bpp in both byte orders, each doubled and not
 *  The items of a frame run in a scrambled order.  The result must equal a per-pixel loop written here, and
 *  fiasco_amd_renderer_render_planes() wherever that accepts the shape.
 *  Exit status 0 and "render_step_check: ok", or 1 and what went wrong.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "libfiasco_amd_render.h"
#include "fa_host.h"

#define RENDER_HOST_REPLAY 1
#include "render.inc"

extern "C" void fa_set_error(const char *fmt, ...) { (void) fmt; }       /* fa_render.c's messages are not looked at here */

static unsigned bad;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned) ((rng_state >> 11) % n);
}

/* what px_load_values hands the item: `n' values packed in pairs, the rest zero; reads exactly n values */
static void load16(const int16_t *p, unsigned n, unsigned v[8])
{
    for (unsigned k = 0; k < 8; k++) {
        const unsigned lo = 2 * k < n ? (uint16_t) p[2 * k] : 0u, hi = 2 * k + 1 < n ? (uint16_t) p[2 * k + 1] : 0u;
        v[k] = lo | (hi << 16);
    }
}

static int clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
static int chroma(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }

/* one pixel as its bytes in memory */
static void plain_pixel(const fiasco_amd_renderer &r, int color, int y, int cb, int cr, unsigned char px[4])
{
    const int yval = (y >> 4) + 128;
    int R = yval, G = yval, B = yval;
    if (color) {
        cb = chroma(cb >> 4); cr = chroma(cr >> 4);
        R = yval + (int) (1.4022 * cr + 0.5);
        G = yval + (int) (-0.7145 * cr + 0.5) + (int) (-0.3456 * cb + 0.5);
        B = yval + (int) (1.7710 * cb + 0.5);
    }
    R = clip255(R); G = clip255(G); B = clip255(B);
    if (r.bpp == 24) { px[0] = (unsigned char) (r.rgb ? R : B); px[1] = (unsigned char) G; px[2] = (unsigned char) (r.rgb ? B : R); px[3] = 0; return; }
    const unsigned v = (((unsigned) R >> r.r_drop) << r.r_up) | (((unsigned) G >> r.g_drop) << r.g_up) | ((unsigned) B >> r.b_drop);
    for (unsigned k = 0; k < 4; k++) px[k] = (unsigned char) (v >> (8 * k));
}

struct Mask { const char *name; unsigned bpp; unsigned long red, green, blue; };
static const Mask k_masks[6] = {
    { "rgb565", 16, 0xf800, 0x07e0, 0x001f }, { "rgb555", 16, 0x7c00, 0x03e0, 0x001f },
    { "xrgb8888", 32, 0xff0000, 0x00ff00, 0x0000ff }, { "blue high", 32, 0x0000ff, 0x00ff00, 0xff0000 },
    { "rgb24", 24, 0xff0000, 0x00ff00, 0x0000ff }, { "bgr24", 24, 0x0000ff, 0x00ff00, 0xff0000 },
};

static void one(const Mask &m, int doubled, unsigned W, unsigned H, int color, unsigned offset, unsigned extra)
{
    fiasco_amd_renderer_t *r = fiasco_amd_renderer_new(m.red, m.green, m.blue, m.bpp, doubled);
    if (!r) { FAIL("%s: no renderer", m.name); return; }
    const RdParams P = { r->bpp, r->doubled, r->rgb, r->r_drop, r->g_drop, r->b_drop, r->r_up, r->g_up };
    const unsigned bytes = m.bpp / 8, dup = doubled ? 2 : 1, bands = color ? 3 : 1;
    const size_t npix = (size_t) W * H, row = (size_t) W * dup * bytes, pitch = row + extra, sh = (size_t) H * dup;
    const size_t extent = (sh - 1) * pitch + row;
    /* planes of exactly W x H values per band, each band a block of its own would hide an overrun into the next: one block */
    int16_t *planes = (int16_t *) malloc(npix * bands * sizeof(int16_t));
    for (size_t k = 0; k < npix * bands; k++) planes[k] = (int16_t) (rnd(8) ? (int) rnd(8192) - 4096 : (int) rnd(65536) - 32768);
    /* exactly the bytes the rows span, so that the sanitizer sees the first byte behind them; an allocator whose blocks do
     * not begin on 16 bytes gets a rounded block instead, whose tail is checked by hand below */
    size_t block_bytes = offset + extent;
    unsigned char *block = (unsigned char *) malloc(block_bytes);
    if ((size_t) block & 15) { free(block); block_bytes = (block_bytes + 15) / 16 * 16; block = (unsigned char *) aligned_alloc(16, block_bytes); }
    unsigned char *shadow = (unsigned char *) malloc(offset + extent);
    memset(block, 0xa5, block_bytes);
    memset(shadow, 0xa5, offset + extent);
    unsigned char *dst = block + offset, *want = shadow + offset;
    for (unsigned y = 0; y < H; y++)
        for (unsigned x = 0; x < W; x++) {
            unsigned char px[4];
            const size_t at = (size_t) y * W + x;
            plain_pixel(*r, color, planes[at], color ? planes[npix + at] : 0, color ? planes[2 * npix + at] : 0, px);
            for (unsigned dy = 0; dy < dup; dy++)
                for (unsigned dx = 0; dx < dup; dx++) memcpy(want + ((size_t) y * dup + dy) * pitch + ((size_t) x * dup + dx) * bytes, px, bytes);
        }
    /* the items of the frame, scrambled */
    const unsigned cpr = (W + 15) / 16;
    std::vector<unsigned> items(cpr * H);
    for (unsigned k = 0; k < items.size(); k++) items[k] = k;
    for (size_t k = items.size(); k > 1; k--) std::swap(items[k - 1], items[rnd((unsigned) k)]);
    for (unsigned it : items) {
        const unsigned rw = it / cpr, x0 = (it - rw * cpr) * 16, n = W - x0 < 16 ? W - x0 : 16;
        const int16_t *p = planes + (size_t) rw * W + x0;
        unsigned y[8], cbv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, crv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
        load16(p, n, y);
        if (color) { load16(p + npix, n, cbv); load16(p + 2 * npix, n, crv); }
        rd_item(P, color != 0, y, cbv, crv, n, dst, pitch, rw, x0);
    }
    auto compare = [&](const char *path) {
    if (memcmp(block, shadow, offset + extent)) {
        size_t k = 0;
        while (block[k] == shadow[k]) k++;
        FAIL("%s%s %u x %u %s offset %u pitch +%u (%s): byte %lu is %02x, not %02x", m.name, doubled ? " doubled" : "", W, H, color ? "colour" : "gray", offset, extra, path,
             (unsigned long) k, block[k], shadow[k]);
    }
    for (size_t k = offset + extent; k < block_bytes; k++)
        if (block[k] != 0xa5) { FAIL("%s %u x %u: wrote behind the surface", m.name, W, H); break; }
    };
    compare("items");
    if (doubled) {
        /* the exchange inside a wave, as the kernel's doubled build runs it: 64 consecutive items put their pieces into an
         * RdWave of exactly its size, then -- the barrier -- the lanes store, here in a scrambled order; a lane beyond the
         * last item puts n = 0 */
        memset(block, 0xa5, block_bytes);
        RdWave *wave = (RdWave *) aligned_alloc(16, sizeof(RdWave));
        const unsigned total = cpr * H;
        for (unsigned first = 0; first < total; first += RD_LANES) {
            memset(wave, 0xee, sizeof(RdWave));
            for (unsigned lane = 0; lane < RD_LANES; lane++) {
                const unsigned it = first + lane;
                unsigned pw[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, n = 0;
                unsigned char *q0 = nullptr;
                if (it < total) {
                    const unsigned rw = it / cpr, x0 = (it - rw * cpr) * 16;
                    n = W - x0 < 16 ? W - x0 : 16;
                    const int16_t *p = planes + (size_t) rw * W + x0;
                    unsigned y[8], cbv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, crv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
                    load16(p, n, y);
                    if (color) { load16(p + npix, n, cbv); load16(p + 2 * npix, n, crv); }
                    rd_pixels(P, color != 0, y, cbv, crv, pw);
                    q0 = rd_first(P, dst, pitch, rw, x0);
                }
                rd_wave_put_any(P, *wave, lane, pw, n, q0, it < total ? pitch : 0);
            }
            unsigned lanes[RD_LANES];
            for (unsigned k = 0; k < RD_LANES; k++) lanes[k] = k;
            for (unsigned k = RD_LANES; k > 1; k--) std::swap(lanes[k - 1], lanes[rnd(k)]);
            for (unsigned lane : lanes) rd_wave_store_any(P, *wave, lane);
        }
        free(wave);
        compare("exchange");
    }
    /* the host loop, where it accepts the shape: packed rows */
    size_t hrow = 0;
    if (fiasco_amd_renderer_surface_size(r, W, H, color, nullptr, nullptr, &hrow)) {
        unsigned char *host = (unsigned char *) malloc(sh * hrow);
        if (hrow != row || !fiasco_amd_renderer_render_planes(r, planes, color, W, H, host)) FAIL("%s %u x %u: the host loop failed", m.name, W, H);
        else for (size_t yy = 0; yy < sh; yy++)
            if (memcmp(host + yy * hrow, want + yy * pitch, row)) { FAIL("%s%s %u x %u: the host loop differs in row %lu", m.name, doubled ? " doubled" : "", W, H, (unsigned long) yy); break; }
        free(host);
    }
    free(shadow); free(block); free(planes);
    fiasco_amd_renderer_delete(r);
}

int main(void)
{
    static const unsigned widths[] = { 1, 15, 16, 17, 18, 33, 34 }, heights[] = { 1, 3, 4 };
    unsigned runs = 0;
    for (const Mask &m : k_masks)
        for (int doubled = 0; doubled < 2; doubled++)
            for (unsigned W : widths)
                for (unsigned H : heights)
                    for (int color = 0; color < 2; color++) {
                        const unsigned px = m.bpp / 8;
                        const unsigned offsets[3] = { 0, px, 1 }, extras[2] = { 0, m.bpp == 24 ? 7u : 2 * px };
                        for (unsigned o = 0; o < (m.bpp == 24 ? 3u : 2u); o++)
                            for (unsigned e = 0; e < 2; e++) { one(m, doubled, W, H, color, offsets[o], extras[e]); runs++; }
                    }
    if (bad) { printf("render_step_check: %u failures in %u runs\n", bad, runs); return 1; }
    printf("render_step_check: ok (%u runs)\n", runs);
    return 0;
}
