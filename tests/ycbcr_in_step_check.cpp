/*
 *  ycbcr_in_step_check.cpp -- the conversion kernel of YCbCr frames in device memory (csrc/hip/input_convert_ycbcr.inc,
 *  icy_convert_kernel) replayed on the CPU, for the sanitizers.
 *
 *  A stand-alone program: it includes input_convert_ycbcr.inc with YCBCR_IN_HOST_REPLAY defined -- the per-item function
 *  icy_item and what it calls (px_load_bytes_wide, px_load_bytes8, px_store_values of px_access.inc, icy_value, icy_row)
 *  as plain C++, no HIP, no library, no device -- and is built by tests/test_ycbcr_input_step_host.py with -fsanitize=address,undefined.
 *    frames     widths 32, 34, 38 and 50, heights 32 and 34; 4:2:0 with two chroma planes (c_step 1) and with one plane of
 *               pairs in both orders (c_step 2: NV12, NV21), 4:4:4 with two planes; packed, and with pitches larger than
 *               the row; beginning at a 16-byte aligned address and one byte off it.  Every source plane is a heap block
 *               that ends with the last byte of its last row, so an item that loads a byte it does not own is caught.
 *    planes     [3][H][W] int16 in one heap block, beginning 0, 4 or 8 bytes behind a 16-byte aligned address (rows of a
 *               plane then begin on 16, 8 or 4 bytes, depending on the width), 16 guard bytes on either side that must
 *               keep their pattern; the gaps between the rows of the sources are read-only and checked as well
 *  The items of a frame run in a scrambled order.  The result must equal a per-sample loop written here.
 *  Exit status 0 and "ycbcr_in_step_check: ok", or 1 and what went wrong.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define YCBCR_IN_HOST_REPLAY 1
#include "input_convert_ycbcr.inc"

static unsigned bad;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned) ((rng_state >> 11) % n);
}

enum { GUARD = 16, PATTERN = 0xa5 };

/* sample i of plane k: every byte value occurs */
static unsigned char sample(unsigned k, size_t i) { return (unsigned char) ((i * 37u + k * 101u + (i >> 8) * 3u) & 255u); }

/* a plane of `rows' rows of `row' bytes, `pitch' apart, that begins `off' bytes behind a 16-byte aligned address, inside a
 * block that ends with the last byte of the last row */
struct Source {
    unsigned char *block = nullptr, *first = nullptr;
    size_t span = 0, pitch = 0, row = 0, rows = 0;
    void make(size_t rows_, size_t row_, size_t pitch_, unsigned off)
    {
        rows = rows_; row = row_; pitch = pitch_; span = (rows - 1) * pitch + row;
        block = (unsigned char *) malloc(GUARD + off + span);
        first = block + GUARD + off;
        memset(block, PATTERN, GUARD + off + span);
    }
    void check_unwritten(const char *what, unsigned w, unsigned h, unsigned variant) const
    {
        for (unsigned char *p = block; p < first; p++) if (*p != PATTERN) { FAIL("%s %u x %u variant %u: byte before the plane written", what, w, h, variant); return; }
        for (size_t r = 0; r + 1 < rows; r++)
            for (size_t k = row; k < pitch; k++) if (first[r * pitch + k] != PATTERN) { FAIL("%s %u x %u variant %u: row %lu: gap byte written", what, w, h, variant, (unsigned long) r); return; }
    }
    ~Source() { free(block); }
};

static int16_t plain(unsigned char b) { return (int16_t) (((int) b - 128) * 16); }

static void run(unsigned w, unsigned h, unsigned variant)
{
    /* variant: layout 0 .. 3 (4:2:0 two planes, NV12, NV21, 4:4:4), pitched, off, destination alignment 0 .. 2 */
    const unsigned lay = variant & 3, pitched = (variant >> 2) & 1, off = (variant >> 3) & 1, dal = variant >> 4;
    const unsigned sub = lay == 3 ? 0 : 1, c_step = lay == 1 || lay == 2 ? 2 : 1, nv21 = lay == 2;
    const unsigned cw = w >> sub, ch = h >> sub;
    const size_t npix = (size_t) w * h;
    Source Y, C0, C1;
    Y.make(h, w, pitched ? w + 7 : w, off);
    const size_t crow = (size_t) cw * c_step, cpitch = pitched ? crow + 5 : crow;
    C0.make(ch, crow, cpitch, off);
    if (c_step == 1) C1.make(ch, crow, cpitch, off);
    std::vector<unsigned char> sy(npix), scb((size_t) cw * ch), scr((size_t) cw * ch);
    for (size_t i = 0; i < sy.size(); i++) sy[i] = sample(0, i);
    for (size_t i = 0; i < scb.size(); i++) { scb[i] = sample(1, i); scr[i] = sample(2, i); }
    for (unsigned y = 0; y < h; y++) memcpy(Y.first + (size_t) y * Y.pitch, &sy[(size_t) y * w], w);
    for (unsigned y = 0; y < ch; y++)
        for (unsigned x = 0; x < cw; x++) {
            if (c_step == 1) { C0.first[y * cpitch + x] = scb[(size_t) y * cw + x]; C1.first[y * cpitch + x] = scr[(size_t) y * cw + x]; }
            else { C0.first[y * cpitch + 2 * x + (nv21 ? 1 : 0)] = scb[(size_t) y * cw + x]; C0.first[y * cpitch + 2 * x + (nv21 ? 0 : 1)] = scr[(size_t) y * cw + x]; }
        }
    /* the planes: GUARD, dal * 4 bytes, [3][h][w] int16, GUARD -- the block ends there */
    const size_t dbytes = 3 * npix * 2, lead = GUARD + dal * 4;
    unsigned char *dblock = (unsigned char *) malloc(lead + dbytes + GUARD);
    memset(dblock, PATTERN, lead + dbytes + GUARD);
    int16_t *dst = (int16_t *) (dblock + lead);
    /* the table entry as icy_describe fills it */
    IcyFrame F;
    memset(&F, 0, sizeof F);
    F.y = Y.first; F.c0 = C0.first; F.c1 = c_step == 1 ? C1.first : C0.first + 1;
    F.dst = dst; F.y_pitch = Y.pitch; F.c_pitch = cpitch; F.first = 0;
    F.width = w; F.height = h; F.c_step = c_step; F.sub = sub; F.swap = nv21; F.cpr = (w + 15) / 16;
    const unsigned total = F.cpr * (h >> sub);
    std::vector<unsigned> order(total);
    for (unsigned i = 0; i < total; i++) order[i] = i;
    for (unsigned i = total; i > 1; i--) std::swap(order[i - 1], order[rnd(i)]);
    for (unsigned i : order) icy_item(F, i);
    /* against the per-sample loop */
    for (unsigned y = 0; y < h && bad < 20; y++)
        for (unsigned x = 0; x < w; x++) {
            const size_t c = (size_t) (y >> sub) * cw + (x >> sub);
            const int16_t want[3] = { plain(sy[(size_t) y * w + x]), plain(scb[c]), plain(scr[c]) };
            for (unsigned b = 0; b < 3; b++)
                if (dst[b * npix + (size_t) y * w + x] != want[b]) {
                    FAIL("%u x %u variant %u: band %u (%u, %u): %d for %d", w, h, variant, b, x, y, dst[b * npix + (size_t) y * w + x], want[b]);
                    y = h; x = w; break;
                }
        }
    for (size_t k = 0; k < lead; k++) if (dblock[k] != PATTERN) { FAIL("%u x %u variant %u: byte %lu before the planes written", w, h, variant, (unsigned long) (lead - k)); break; }
    for (size_t k = 0; k < GUARD; k++) if (dblock[lead + dbytes + k] != PATTERN) { FAIL("%u x %u variant %u: byte %lu behind the planes written", w, h, variant, (unsigned long) k); break; }
    Y.check_unwritten("Y", w, h, variant);
    C0.check_unwritten("chroma", w, h, variant);
    if (c_step == 1) C1.check_unwritten("Cr", w, h, variant);
    free(dblock);
}

int main(void)
{
    const unsigned widths[4] = { 32, 34, 38, 50 }, heights[2] = { 32, 34 };
    unsigned runs = 0;
    for (unsigned w : widths)
        for (unsigned h : heights)
            for (unsigned variant = 0; variant < 48; variant++) { run(w, h, variant); runs++; }
    if (bad) { printf("ycbcr_in_step_check: %u failures\n", bad); return 1; }
    printf("ycbcr_in_step_check: ok (%u runs)\n", runs);
    return 0;
}
