/*
 *  render_420_step_check.cpp -- the 4:2:0 rendering kernel of the device decoder (csrc/hip/render_420.inc,
 *  rd420_render_kernel) replayed on the CPU, for the sanitizers.
 *
 *  A stand-alone program: it includes render_420.inc with RENDER420_HOST_REPLAY defined -- the per-item functions rd4_load
 *  and rd4_item, render.inc's rd_pixels, rd_store and the exchange inside a wave (rd_wave_put, rd_wave_store) that the
 *  doubled build runs once per source row, and the accesses of px_access.inc, all as plain C++: no HIP, no library, no
 *  device -- and is built by tests/test_render_420_step_host.py with -fsanitize=address,undefined and linked with
 *  csrc/host/fa_render.c, the plain host loop.
 *    frames     widths 2, 4, 14, 16, 18, 30, 32, 34, 36 and 66, heights 2, 4 and 6, full-range values; every plane is a heap
 *               block of its own of exactly W x H or (W / 2) x (H / 2) values, and an item loads only the values it owns
 *    surfaces   heap blocks of exactly the bytes the rows span, beginning at the block (16-byte aligned), one pixel into it
 *               and, at 24 bpp, one byte into it; packed, and with a pitch of 7 bytes (24 bpp) or two pixels (16, 32 bpp)
 *               above the row.  Every byte between two rows must keep its pattern
 *    renderers  all twelve; 24 bpp not doubled at the widths that are multiples of 4 (4, 16, 32, 36), as the size rule has it
 *    exchange   waves of 64 lanes, and for every frame also waves that hold 1 and 63 live lanes only
 *  The items of a frame run in a scrambled order.  The result must equal a per-pixel loop written here, and
 *  fiasco_amd_renderer_render_planes_420().
 *  Exit status 0 and "render_420_step_check: ok", or 1 and what went wrong.
 */
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "libfiasco_amd_render_420.h"
#include "fa_host.h"

#define RENDER420_HOST_REPLAY 1
#include "render_420.inc"

extern "C" void fa_set_error(const char *fmt, ...) { (void) fmt; }       /* fa_render.c's messages are not looked at here */

static unsigned bad;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned) ((rng_state >> 11) % n);
}

static int clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
static int chroma(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }

/* one pixel as its bytes in memory */
static void plain_pixel(const fiasco_amd_renderer &r, int y, int cb, int cr, unsigned char px[4])
{
    const int yval = (y >> 4) + 128;
    cb = chroma(cb >> 4); cr = chroma(cr >> 4);
    const int R = clip255(yval + (int) (1.4022 * cr + 0.5));
    const int G = clip255(yval + (int) (-0.7145 * cr + 0.5) + (int) (-0.3456 * cb + 0.5));
    const int B = clip255(yval + (int) (1.7710 * cb + 0.5));
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

static int16_t *random_plane(size_t n)
{
    int16_t *p = (int16_t *) malloc(n * sizeof(int16_t));
    for (size_t k = 0; k < n; k++) p[k] = (int16_t) (rnd(8) ? (int) rnd(8192) - 4096 : (int) rnd(65536) - 32768);
    return p;
}

static void one(const Mask &m, int doubled, unsigned W, unsigned H, unsigned offset, unsigned extra)
{
    fiasco_amd_renderer_t *r = fiasco_amd_renderer_new(m.red, m.green, m.blue, m.bpp, doubled);
    if (!r) { FAIL("%s: no renderer", m.name); return; }
    const RdParams P = { r->bpp, r->doubled, r->rgb, r->r_drop, r->g_drop, r->b_drop, r->r_up, r->g_up };
    const unsigned bytes = m.bpp / 8, dup = doubled ? 2 : 1, cw = W / 2, ch = H / 2;
    const size_t row = (size_t) W * dup * bytes, pitch = row + extra, sh = (size_t) H * dup;
    const size_t extent = (sh - 1) * pitch + row;
    /* three blocks of exactly their values: the sanitizer sees the first value behind each */
    int16_t *py = random_plane((size_t) W * H), *pcb = random_plane((size_t) cw * ch), *pcr = random_plane((size_t) cw * ch);
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
            const size_t c = (size_t) (y / 2) * cw + x / 2;
            plain_pixel(*r, py[(size_t) y * W + x], pcb[c], pcr[c], px);
            for (unsigned dy = 0; dy < dup; dy++)
                for (unsigned dx = 0; dx < dup; dx++) memcpy(want + ((size_t) y * dup + dy) * pitch + ((size_t) x * dup + dx) * bytes, px, bytes);
        }
    Rd4Frame F;
    F.sy = py; F.s0 = pcb; F.s1 = pcr; F.dst = dst; F.pitch = pitch; F.first = 0; F.width = W; F.height = H; F.cpr = (W + 15) / 16;
    const unsigned total = F.cpr * ch;
    /* the items of the frame, scrambled */
    std::vector<unsigned> items(total);
    for (unsigned k = 0; k < total; k++) items[k] = k;
    for (size_t k = items.size(); k > 1; k--) std::swap(items[k - 1], items[rnd((unsigned) k)]);
    for (unsigned it : items) rd4_item(F, it, P);
    auto compare = [&](const char *path) {
        if (memcmp(block, shadow, offset + extent)) {
            size_t k = 0;
            while (block[k] == shadow[k]) k++;
            FAIL("%s%s %u x %u offset %u pitch +%u (%s): byte %lu is %02x, not %02x", m.name, doubled ? " doubled" : "", W, H, offset, extra, path,
                 (unsigned long) k, block[k], shadow[k]);
        }
        for (size_t k = offset + extent; k < block_bytes; k++)
            if (block[k] != 0xa5) { FAIL("%s %u x %u: wrote behind the surface", m.name, W, H); break; }
    };
    compare("items");
    if (doubled) {
        /* the exchange inside a wave, as the kernel's doubled build runs it: `live' consecutive items put the pieces of one
         * source row into an RdWave of exactly its size, the other lanes put n = 0, then -- the barrier -- all 64 lanes
         * store, here in a scrambled order; then the same for the second source row */
        static const unsigned lives[3] = { RD_LANES, 63, 1 };
        RdWave *wave = (RdWave *) aligned_alloc(16, sizeof(RdWave));
        for (unsigned live : lives) {
            memset(block, 0xa5, block_bytes);
            for (unsigned first = 0; first < total; first += live)
                for (unsigned h = 0; h < 2; h++) {
                    memset(wave, 0xee, sizeof(RdWave));
                    for (unsigned lane = 0; lane < RD_LANES; lane++) {
                        const unsigned it = first + lane;
                        unsigned pw[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, n = 0;
                        unsigned char *q0 = nullptr;
                        const bool has = lane < live && it < total;
                        if (has) {
                            unsigned y0[8], y1[8], cbv[8], crv[8], crow, x0;
                            n = rd4_load(F, it, y0, y1, cbv, crv, crow, x0);
                            rd_pixels<1>(P, true, h ? y1 : y0, cbv, crv, pw);
                            q0 = rd_first(P, dst, pitch, 2 * crow + h, x0);
                        }
                        rd_wave_put_any(P, *wave, lane, pw, n, q0, has ? pitch : 0);
                    }
                    unsigned lanes[RD_LANES];
                    for (unsigned k = 0; k < RD_LANES; k++) lanes[k] = k;
                    for (unsigned k = RD_LANES; k > 1; k--) std::swap(lanes[k - 1], lanes[rnd(k)]);
                    for (unsigned lane : lanes) rd_wave_store_any(P, *wave, lane);
                }
            compare(live == RD_LANES ? "exchange, 64 live lanes" : live == 63 ? "exchange, 63 live lanes" : "exchange, 1 live lane");
        }
        free(wave);
    }
    /* the host loop: packed rows */
    size_t hrow = 0;
    if (!fiasco_amd_renderer_surface_size_420(r, W, H, nullptr, nullptr, &hrow) || hrow != row) FAIL("%s %u x %u: the size rule refuses", m.name, W, H);
    else {
        unsigned char *host = (unsigned char *) malloc(sh * hrow);
        if (!fiasco_amd_renderer_render_planes_420(r, py, pcb, pcr, W, H, host)) FAIL("%s %u x %u: the host loop failed", m.name, W, H);
        else for (size_t yy = 0; yy < sh; yy++)
            if (memcmp(host + yy * hrow, want + yy * pitch, row)) { FAIL("%s%s %u x %u: the host loop differs in row %lu", m.name, doubled ? " doubled" : "", W, H, (unsigned long) yy); break; }
        free(host);
    }
    free(shadow); free(block); free(py); free(pcb); free(pcr);
    fiasco_amd_renderer_delete(r);
}

int main(void)
{
    static const unsigned widths[] = { 2, 4, 14, 16, 18, 30, 32, 34, 36, 66 }, heights[] = { 2, 4, 6 };
    unsigned runs = 0, runs24 = 0;
    for (const Mask &m : k_masks)
        for (int doubled = 0; doubled < 2; doubled++)
            for (unsigned W : widths)
                for (unsigned H : heights) {
                    if (m.bpp == 24 && !doubled && (W & 3)) {          /* refused, and by the host loop as well */
                        fiasco_amd_renderer_t *r = fiasco_amd_renderer_new(m.red, m.green, m.blue, m.bpp, doubled);
                        if (fiasco_amd_renderer_surface_size_420(r, W, H, nullptr, nullptr, nullptr)) FAIL("%s %u x %u: the size rule accepts", m.name, W, H);
                        fiasco_amd_renderer_delete(r);
                        continue;
                    }
                    const unsigned px = m.bpp / 8;
                    const unsigned offsets[3] = { 0, px, 1 }, extras[2] = { 0, m.bpp == 24 ? 7u : 2 * px };
                    for (unsigned o = 0; o < (m.bpp == 24 ? 3u : 2u); o++)
                        for (unsigned e = 0; e < 2; e++) { one(m, doubled, W, H, offsets[o], extras[e]); runs++; runs24 += m.bpp == 24 && !doubled; }
                }
    if (!runs24) FAIL("no 24 bpp surface that is not doubled was rendered");
    if (bad) { printf("render_420_step_check: %u failures in %u runs\n", bad, runs); return 1; }
    printf("render_420_step_check: ok (%u runs)\n", runs);
    return 0;
}
