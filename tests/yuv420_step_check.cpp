/*
 *  yuv420_step_check.cpp -- the 4:2:0 conversion kernel of the device decoder (csrc/hip/output_convert_420.inc,
 *  oc420_convert_kernel) replayed on the CPU, for the sanitizers.
 *
 *  A stand-alone program: it includes output_convert_420.inc with Y420_HOST_REPLAY defined -- the per-item function y4_item
 *  and what it calls (px_load_values, px_store_bytes_vec of px_access.inc, y4_byte, y4_bytes) as plain C++, no HIP, no library, no device -- and is built
 *  by tests/test_420_step_host.py with -fsanitize=address,undefined.
 *    planes     widths 2, 30, 34 and 50, heights 2 and 6; Y of exactly W x H values, Cb and Cr of exactly (W / 2) x (H / 2), heap
 *               blocks of their own, so an item that loads a value it does not own is caught; every plane meets the clip
 *               bounds (p >> 4 of -129, -128, 127, 128; the formula of tests/yuv420_ref.py handmade(), restated here)
 *    targets    c_step 1 (two planes) and c_step 2 in both orders (NV12, NV21); packed, and with pitches larger than the row;
 *               beginning at a 16-byte aligned address and one byte off it; every plane a heap block of exactly the bytes its
 *               rows span plus 16 guard bytes on either side, and every byte of the guards and between two rows must keep
 *               its pattern
 *  The items of a frame run in a scrambled order.  The result must equal a per-sample loop written here.
 *  Exit status 0 and "yuv420_step_check: ok", or 1 and what went wrong.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define Y420_HOST_REPLAY 1
#include "output_convert_420.inc"

static unsigned bad;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned) ((rng_state >> 11) % n);
}

static const int SPECIALS[4] = { -129, -128, 127, 128 };

/* plane k of tests/yuv420_ref.py handmade(): n values */
static std::vector<int16_t> handmade(unsigned k, size_t n)
{
    std::vector<int16_t> v(n);
    for (size_t i = 0; i < n; i++)
        v[i] = (int16_t) ((int) ((((uint64_t) i * 7919u + (uint64_t) k * 104729u + 12345u) * 2654435761ull) % 65536u) - 32768);
    for (size_t j = 0; j < 4 && j < n; j++) v[j] = (int16_t) (SPECIALS[j] * 16 + (int) ((j * 5) % 16));
    return v;
}

static unsigned char plain_byte(int16_t p)
{
    const int b = (p >> 4) + 128;
    return (unsigned char) (b < 0 ? 0 : b > 255 ? 255 : b);
}

enum { GUARD = 16, PATTERN = 0xa5 };

/* a plane of `rows' rows of `row' bytes, `pitch' apart, that begins `off' bytes behind a 16-byte aligned address, inside a
 * block of exactly GUARD + the bytes the rows span + GUARD bytes */
struct Surface {
    unsigned char *block = nullptr, *first = nullptr;
    size_t span = 0, pitch = 0, row = 0, rows = 0;
    void make(size_t rows_, size_t row_, size_t pitch_, unsigned off)
    {
        rows = rows_; row = row_; pitch = pitch_; span = (rows - 1) * pitch + row;
        block = (unsigned char *) malloc(GUARD + off + span + GUARD);      /* 16-byte aligned; what lies behind the guard is the sanitizer's */
        first = block + GUARD + off;
        memset(block, PATTERN, GUARD + off + span + GUARD);
    }
    /* every byte that is no sample kept its pattern */
    void check_untouched(const char *what, unsigned w, unsigned h, unsigned variant) const
    {
        for (unsigned char *p = block; p < first; p++) if (*p != PATTERN) { FAIL("%s %u x %u variant %u: byte %ld before the plane written", what, w, h, variant, (long) (first - p)); return; }
        for (size_t k = 0; k < GUARD; k++) if (first[span + k] != PATTERN) { FAIL("%s %u x %u variant %u: byte %lu behind the plane written", what, w, h, variant, (unsigned long) k); return; }
        for (size_t r = 0; r + 1 < rows; r++)
            for (size_t k = row; k < pitch; k++) if (first[r * pitch + k] != PATTERN) { FAIL("%s %u x %u variant %u: row %lu: gap byte %lu written", what, w, h, variant, (unsigned long) r, (unsigned long) k); return; }
    }
    ~Surface() { free(block); }
};

static void run(unsigned w, unsigned h, unsigned variant)
{
    const unsigned c_step = variant & 1 ? 2 : 1, pitched = (variant >> 1) & 1, off = (variant >> 2) & 1, nv21 = (variant >> 3) & 1;
    const unsigned cw = w / 2, ch = h / 2;
    if (nv21 && c_step == 1) return;
    /* the planes: heap blocks of exactly their values (16-byte aligned, as the decoder's are at these sizes or not -- rows of
     * odd width / 8 are not, and the loads narrow) */
    const std::vector<int16_t> hy = handmade(0, (size_t) w * h), hcb = handmade(1, (size_t) cw * ch), hcr = handmade(2, (size_t) cw * ch);
    int16_t *sy = (int16_t *) malloc(hy.size() * 2), *scb = (int16_t *) malloc(hcb.size() * 2), *scr = (int16_t *) malloc(hcr.size() * 2);
    memcpy(sy, hy.data(), hy.size() * 2); memcpy(scb, hcb.data(), hcb.size() * 2); memcpy(scr, hcr.data(), hcr.size() * 2);
    for (unsigned k = 0; k < 3; k++) {
        const std::vector<int16_t> &p = k == 0 ? hy : k == 1 ? hcb : hcr;
        for (unsigned j = 0; j < 4 && j < p.size(); j++) if ((p[j] >> 4) != SPECIALS[j]) FAIL("plane %u does not meet clip bound %d", k, SPECIALS[j]);
    }
    Surface Y, C0, C1;
    Y.make(h, w, pitched ? w + 7 : w, off);
    const size_t crow = (size_t) cw * c_step, cpitch = pitched ? crow + 5 : crow;
    C0.make(ch, crow, cpitch, off);
    if (c_step == 1) C1.make(ch, crow, cpitch, off);
    /* the table entry as y4_describe fills it */
    Y4Frame F;
    memset(&F, 0, sizeof F);
    F.sy = sy; F.s0 = nv21 ? scr : scb; F.s1 = nv21 ? scb : scr;
    F.dy = Y.first; F.d0 = C0.first; F.d1 = c_step == 1 ? C1.first : C0.first + 1;
    F.y_pitch = Y.pitch; F.c_pitch = cpitch; F.first = 0;
    F.width = w; F.height = h; F.c_step = c_step;
    F.cpr = (w + 15) / 16; F.ccpr = (cw + 15) / 16; F.ny = F.cpr * h;
    const unsigned total = F.ny + F.ccpr * ch * (c_step == 1 ? 2 : 1);
    std::vector<unsigned> order(total);
    for (unsigned i = 0; i < total; i++) order[i] = i;
    for (unsigned i = total; i > 1; i--) std::swap(order[i - 1], order[rnd(i)]);
    for (unsigned i : order) y4_item(F, i);
    /* against the per-sample loop */
    for (unsigned y = 0; y < h; y++)
        for (unsigned x = 0; x < w; x++)
            if (Y.first[(size_t) y * Y.pitch + x] != plain_byte(hy[(size_t) y * w + x])) { FAIL("Y %u x %u variant %u: (%u, %u)", w, h, variant, x, y); y = h; break; }
    for (unsigned y = 0; y < ch; y++)
        for (unsigned x = 0; x < cw; x++) {
            const unsigned char cb = plain_byte(hcb[(size_t) y * cw + x]), cr = plain_byte(hcr[(size_t) y * cw + x]);
            unsigned char gb, gr;
            if (c_step == 1) { gb = C0.first[y * cpitch + x]; gr = C1.first[y * cpitch + x]; }
            else { gb = C0.first[y * cpitch + 2 * x + (nv21 ? 1 : 0)]; gr = C0.first[y * cpitch + 2 * x + (nv21 ? 0 : 1)]; }
            if (gb != cb || gr != cr) { FAIL("chroma %u x %u variant %u: (%u, %u): %u %u for %u %u", w, h, variant, x, y, gb, gr, cb, cr); y = ch; break; }
        }
    Y.check_untouched("Y", w, h, variant);
    C0.check_untouched("chroma", w, h, variant);
    if (c_step == 1) C1.check_untouched("Cr", w, h, variant);
    free(sy); free(scb); free(scr);
}

int main(void)
{
    const unsigned widths[4] = { 2, 30, 34, 50 }, heights[2] = { 2, 6 };
    unsigned runs = 0;
    for (unsigned w : widths)
        for (unsigned h : heights)
            for (unsigned variant = 0; variant < 16; variant++) { run(w, h, variant); runs++; }
    if (bad) { printf("yuv420_step_check: %u failures\n", bad); return 1; }
    printf("yuv420_step_check: ok (%u runs)\n", runs);
    return 0;
}
