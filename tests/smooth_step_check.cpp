/*
 *  smooth_step_check.cpp -- the smoothing step of the device decoder (csrc/hip/smooth.inc) replayed on the CPU, for the
 *  sanitizers.
 *
 *  A stand-alone program: it includes smooth.inc with SMOOTH_HOST_REPLAY defined -- the checks, the packing and the
 *  kernel's per-item function as plain C++, no HIP, no library, no device -- and is built by
 *  tests/test_smooth_step_host.py with -fsanitize=address,undefined.
 *    flights    random bintree partitions of gray and colour frames (colour: the Y partition, then the Cb partition, as
 *               fa_smoothing_borders lists them), 1 to 32 frames of mixed and ragged sizes per flight, one list of
 *               1280 x 720 with at least 25 passes among them.  The tables are carved the way dec_flight_prepare carves
 *               them -- a table of 32 SmDesc, then sm_table_bytes() per frame, 256-byte steps -- in ONE heap block of
 *               exactly that size, and a second time with every frame's tables in a heap block of exactly
 *               sm_table_bytes(); every plane is a heap block of exactly W x H values.  Some frames leave the flight
 *               between the carve and the launches, so the descriptor table is shorter than the flight and indexed by
 *               itself.  Every (pass, frame, item) of the grid a launch would have runs once, the items of a pass in a
 *               scattered order, the frames back to front in every other pass.  The planes must equal the sequential loop
 *               over the list (the reference's order), written here a second time.
 *    refusals   malformed lists -- a border outside the plane on either side, at row or column 0, empty, longer than its
 *               level's side, a gap in the passes, a first pass other than 0, a pass that goes back, two levels in one
 *               pass, a level out of range -- are refused by sm_check, a block of another size by sm_pack.
 *    factors    70 -> 333, 179; 1 -> 509, 3; 100 -> 256, 256; 0 and 101: nothing.
 *  Exit status 0 and "smooth_step_check: ok", or 1 and what went wrong.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "libfiasco_amd.h"

#define SMOOTH_HOST_REPLAY 1
#include "smooth.inc"

static const unsigned FLIGHT = 32;       /* DEC_FLIGHT */

static unsigned bad;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static unsigned rnd(unsigned n)              /* 0 .. n - 1 */
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned) ((rng_state >> 11) % n);
}

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

/* ------------------------------------------------------------------ partitions */

typedef std::vector<std::vector<fiasco_amd_border> > ByLevel;       /* [level] */

/* the block of `level' at (x, y): split or not; a split block has its border where its second half begins */
static void split(ByLevel &out, unsigned level, unsigned x, unsigned y, unsigned W, unsigned H, unsigned leaf, unsigned always)
{
    if (x >= W || y >= H || level == 0) return;
    if (level <= leaf || (level <= always && rnd(10) >= 7)) return;
    const unsigned w = 1u << (level >> 1), h = 1u << ((level + 1) >> 1);
    fiasco_amd_border b;
    memset(&b, 0, sizeof b);
    b.level = (uint8_t) level;
    if (level & 1) {                              /* halves above each other */
        const unsigned yb = y + h / 2;
        if (yb < H) { b.x = (uint16_t) x; b.y = (uint16_t) yb; b.len = (uint16_t) (w < W - x ? w : W - x); out[level].push_back(b); }
        split(out, level - 1, x, y, W, H, leaf, always);
        split(out, level - 1, x, yb, W, H, leaf, always);
    } else {                                      /* side by side */
        const unsigned xb = x + w / 2;
        if (xb < W) { b.x = (uint16_t) xb; b.y = (uint16_t) y; b.len = (uint16_t) (h < H - y ? h : H - y); out[level].push_back(b); }
        split(out, level - 1, x, y, W, H, leaf, always);
        split(out, level - 1, xb, y, W, H, leaf, always);
    }
}

/* the list of a frame: bands (1 gray, 2 colour: Y and Cb) x levels ascending, one pass per (band, level) that has a border */
static std::vector<fiasco_amd_border> partition(unsigned W, unsigned H, bool colour, unsigned *npasses)
{
    unsigned root = 0;
    while ((1u << (root >> 1)) < W || (1u << ((root + 1) >> 1)) < H) root++;
    std::vector<fiasco_amd_border> list;
    unsigned pass = 0;
    for (unsigned band = 0; band < (colour ? 2u : 1u); band++) {
        ByLevel lv(root + 1);
        const unsigned leaf = band ? 4 + rnd(4) : 1 + rnd(5);
        split(lv, root, 0, 0, W, H, leaf, root > 6 ? root - 3 : root);
        for (unsigned l = 0; l <= root; l++) {
            if (lv[l].empty()) continue;
            for (fiasco_amd_border b : lv[l]) { b.pass = (uint8_t) pass; list.push_back(b); }
            pass++;
        }
    }
    *npasses = pass;
    return list;
}

/* the reference's loop, restated: the borders one after the other, each pair of each in place */
static void sequential(std::vector<int16_t> &p, unsigned W, const std::vector<fiasco_amd_border> &list, int is, int inegs)
{
    for (const fiasco_amd_border &b : list)
        for (unsigned k = 0; k < b.len; k++) {
            int16_t *one = b.level & 1 ? &p[(size_t) (b.y - 1) * W + b.x + k] : &p[(size_t) (b.y + k) * W + b.x - 1];
            int16_t *two = b.level & 1 ? one + W : one + 1;
            const int a = *one, c = *two;
            *one = (int16_t) (((is * a) >> 10) * 2 + ((inegs * c) >> 10) * 2);
            *two = (int16_t) (((is * c) >> 10) * 2 + ((inegs * a) >> 10) * 2);
        }
}

/* ------------------------------------------------------------------ flights */

struct Frame {
    unsigned W, H, npasses = 0, checked = 0;
    unsigned long long pairs = 0;
    int is = 0, inegs = 0;
    std::vector<fiasco_amd_border> list;
    std::vector<int16_t> want;           /* the sequential result */
    int16_t *plane = nullptr;            /* malloc of exactly W * H values */
    size_t off = 0, bytes = 0;           /* its tables in the flight's block */
    char *own = nullptr;                 /* ... or in a block of their own */
    bool alive = true;
};

static unsigned gcd(unsigned long long a, unsigned long long b) { while (b) { const unsigned long long t = a % b; a = b; b = t; } return (unsigned) a; }

/* one flight; separate: every frame's tables in a heap block of their own instead of the flight's */
static void flight(std::vector<Frame> &fr, bool separate)
{
    static const int percents[4] = { 1, 35, 70, 100 };
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t at = need; need += align256(bytes); return at; };
    /* dec_smooth_prepare: factors, check, the size of the tables */
    for (Frame &f : fr) {
        char msg[200];
        if (!sm_factors(percents[rnd(4)], &f.is, &f.inegs)) FAIL("no factors");
        if (!sm_check(f.list.data(), (unsigned) f.list.size(), f.W, f.H, &f.checked, &f.pairs, msg, sizeof msg)) { FAIL("a generated list was refused: %s", msg); return; }
        if (f.checked != f.npasses) FAIL("sm_check counts %u passes, the generator %u", f.checked, f.npasses);
        f.bytes = sm_table_bytes((unsigned) f.list.size(), f.npasses);
        f.plane = (int16_t *) malloc((size_t) f.W * f.H * sizeof(int16_t));
        f.want.resize((size_t) f.W * f.H);
        for (size_t k = 0; k < f.want.size(); k++) f.want[k] = f.plane[k] = (int16_t) (rnd(65536) - 32768);
        sequential(f.want, f.W, f.list, f.is, f.inegs);
    }
    /* dec_flight_prepare: the carve, then the packing into a block of exactly that size */
    const size_t desc_off = take(FLIGHT * sizeof(SmDesc));
    const size_t first = need;
    for (Frame &f : fr) if (f.npasses) f.off = take(f.bytes);
    char *arena = (char *) malloc(need);
    memset(arena, 0x5a, need);
    for (Frame &f : fr) {
        if (!f.npasses) continue;
        char *at = arena + f.off;
        if (separate) at = f.own = (char *) malloc(f.bytes);
        if (!sm_pack(f.list.data(), (unsigned) f.list.size(), f.npasses, at, f.bytes)) FAIL("sm_pack refused its own carve");
    }
    (void) first;
    /* frames leave the flight between the carve and the launches */
    if (fr.size() > 1) for (Frame &f : fr) if (rnd(5) == 0) f.alive = false;
    /* dec_flight_smooth: the descriptors of the frames that got here, then pass after pass */
    SmDesc *descs = (SmDesc *) (arena + desc_off);
    std::vector<Frame *> got;
    unsigned passes = 0;
    for (Frame &f : fr) {
        if (!f.alive || !f.npasses) continue;
        sm_describe(descs[got.size()], f.plane, f.W, f.H, separate ? f.own : arena + f.off, (unsigned) f.list.size(), f.npasses, f.is, f.inegs);
        got.push_back(&f);
        if (f.npasses > passes) passes = f.npasses;
    }
    static const unsigned strides[5] = { 1000003, 7919, 104729, 611953, 1 };
    for (unsigned p = 0; p < passes; p++) {
        unsigned long long most = 0;
        for (Frame *f : got) {
            const unsigned long long items = sm_pass_items(separate ? f->own : arena + f->off, (unsigned) f->list.size(), f->npasses, p);
            if (items > most) most = items;
        }
        const unsigned long long total = (most + 255) / 256 * 256;          /* the threads of a frame's row of the grid */
        unsigned stride = 1;
        for (unsigned s : strides) if (gcd(total, s) == 1) { stride = s; break; }
        const unsigned long long start = total ? rnd(1u << 20) % total : 0;
        for (size_t g = 0; g < got.size(); g++) {
            const size_t y = p & 1 ? got.size() - 1 - g : g;                /* blockIdx.y */
            for (unsigned long long j = 0; j < total; j++) sm_item(descs[y], p, (start + j * stride) % total);
        }
    }
    for (Frame &f : fr) {
        const bool smoothed = f.alive && f.npasses;
        if (smoothed && memcmp(f.plane, f.want.data(), f.want.size() * sizeof(int16_t)) != 0)
            FAIL("a frame of %u x %u (%zu borders, %u passes) differs from the sequential loop", f.W, f.H, f.list.size(), f.npasses);
        free(f.plane); free(f.own);
        f.plane = nullptr; f.own = nullptr;
    }
    free(arena);
}

static Frame make_frame(unsigned W, unsigned H, bool colour)
{
    Frame f;
    f.W = W; f.H = H;
    f.list = partition(W, H, colour, &f.npasses);
    return f;
}

static void flights(void)
{
    unsigned most_passes = 0, frames = 0, big_passes = 0;
    for (unsigned round = 0; round < 14; round++) {
        const unsigned n = round == 0 ? 1 : round == 1 ? FLIGHT : 1 + rnd(FLIGHT);
        std::vector<Frame> fr;
        for (unsigned k = 0; k < n; k++) {
            const bool big = round == 2 && k == 1;
            const unsigned W = big ? 1280 : k % 3 == 0 ? 16u << rnd(4) : 9 + rnd(190), H = big ? 720 : k % 5 == 0 ? 16u << rnd(4) : 7 + rnd(150);
            fr.push_back(make_frame(W, H, big || rnd(2)));
            if (big) big_passes = fr.back().npasses;
            if (fr.back().npasses > most_passes) most_passes = fr.back().npasses;
        }
        frames += n;
        flight(fr, (round & 1) != 0);
    }
    /* a frame too small to have a border beside others: no tables, no descriptor */
    {
        std::vector<Frame> fr;
        fr.push_back(make_frame(1, 1, false));
        fr.push_back(make_frame(33, 17, true));
        if (fr[0].npasses) FAIL("a frame of one pixel has a border");
        flight(fr, false);
    }
    if (big_passes < 25) FAIL("the 1280 x 720 list has %u passes, fewer than 25", big_passes);
    printf("flights: %u frames, up to %u passes, 1280 x 720 with %u\n", frames, most_passes, big_passes);
}

/* ------------------------------------------------------------------ refusals, factors */

static fiasco_amd_border border(unsigned x, unsigned y, unsigned len, unsigned level, unsigned pass)
{
    fiasco_amd_border b;
    b.x = (uint16_t) x; b.y = (uint16_t) y; b.len = (uint16_t) len; b.level = (uint8_t) level; b.pass = (uint8_t) pass;
    return b;
}

static bool refused(std::vector<fiasco_amd_border> l, unsigned W, unsigned H, const char *why)
{
    unsigned np = 0;
    unsigned long long pairs = 0;
    char msg[200] = "";
    if (sm_check(l.data(), (unsigned) l.size(), W, H, &np, &pairs, msg, sizeof msg)) { FAIL("not refused: %s", why); return false; }
    if (!strstr(msg, why)) FAIL("refused for another reason than `%s': %s", why, msg);
    return true;
}

static void refusals(void)
{
    const unsigned W = 48, H = 40;
    /* level 5: horizontal, side 4; level 6: vertical, side 8 */
    const fiasco_amd_border h = border(8, 4, 4, 5, 0), v = border(4, 8, 8, 6, 1);
    unsigned np = 0;
    unsigned long long pairs = 0;
    char msg[200];
    std::vector<fiasco_amd_border> good = { h, v };
    if (!sm_check(good.data(), 2, W, H, &np, &pairs, msg, sizeof msg) || np != 2 || pairs != 12) FAIL("a good list was refused: %s", msg);
    if (!sm_check(nullptr, 0, W, H, &np, &pairs, msg, sizeof msg) || np != 0 || pairs != 0) FAIL("the empty list was refused");
    /* the last row and column, a border clipped to one pair: inside */
    good = { border(44, H - 1, 4, 5, 0), border(W - 1, 32, 8, 6, 1), border(1, 0, 1, 6, 1), border(W - 1, H - 1, 1, 6, 1) };
    if (!sm_check(good.data(), 4, W, H, &np, &pairs, msg, sizeof msg)) FAIL("borders at the edges were refused: %s", msg);
    refused({ border(8, H, 4, 5, 0) }, W, H, "outside the plane");
    refused({ border(8, 0, 4, 5, 0) }, W, H, "outside the plane");
    refused({ border(46, 4, 4, 5, 0) }, W, H, "outside the plane");
    refused({ border(0, 8, 8, 6, 0) }, W, H, "outside the plane");
    refused({ border(W, 8, 8, 6, 0) }, W, H, "outside the plane");
    refused({ border(4, 36, 8, 6, 0) }, W, H, "outside the plane");
    refused({ border(65535, 65535, 4, 5, 0) }, W, H, "outside the plane");
    refused({ border(8, 4, 0, 5, 0) }, W, H, "length");
    refused({ border(8, 4, 5, 5, 0) }, W, H, "length");
    refused({ h, border(4, 8, 8, 6, 2) }, W, H, "gaps");
    refused({ border(8, 4, 4, 5, 1) }, W, H, "gaps");
    refused({ h, v, border(16, 4, 4, 5, 0) }, W, H, "gaps");
    refused({ h, border(4, 8, 8, 6, 0) }, W, H, "two levels");
    refused({ border(8, 4, 4, 41, 0) }, W, H, "level out of range");
    good = { h, v };
    std::vector<char> block(sm_table_bytes(2, 2) + 8);
    if (sm_pack(good.data(), 2, 2, block.data(), sm_table_bytes(2, 2) + 4)) FAIL("sm_pack took a block of another size");
    if (sm_pack(good.data(), 2, 1, block.data(), sm_table_bytes(2, 1))) FAIL("sm_pack took another number of passes");
    if (!sm_pack(good.data(), 2, 2, block.data(), sm_table_bytes(2, 2))) FAIL("sm_pack refused a good list");
    if (sm_pass_items(block.data(), 2, 2, 0) != 4 || sm_pass_items(block.data(), 2, 2, 1) != 8 || sm_pass_items(block.data(), 2, 2, 2) != 0) FAIL("sm_pass_items");
}

static void factors(void)
{
    static const int want[3][3] = { { 70, 333, 179 }, { 1, 509, 3 }, { 100, 256, 256 } };
    for (const int *w : want) {
        int is = 0, inegs = 0;
        if (!sm_factors(w[0], &is, &inegs) || is != w[1] || inegs != w[2]) FAIL("factors of %d: %d, %d", w[0], is, inegs);
    }
    int is = 0, inegs = 0;
    if (sm_factors(0, &is, &inegs) || sm_factors(101, &is, &inegs) || sm_factors(-1, &is, &inegs)) FAIL("factors where the reference smooths nothing");
}

int main(void)
{
    factors();
    refusals();
    flights();
    if (bad) { printf("smooth_step_check: %u failures\n", bad); return 1; }
    printf("smooth_step_check: ok\n");
    return 0;
}
