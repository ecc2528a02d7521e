/*
 *  shown_step_check.cpp -- the fused smoothing kernel of the device decoder (csrc/hip/smooth.inc, sm_frame_kernel) replayed
 *  on the CPU on the border lists of magnified frames, for the sanitizers.
 *
 *  A stand-alone program: it includes smooth.inc with SMOOTH_HOST_REPLAY defined -- the checks, the packing, the per-item
 *  function and the kernel's body between two barriers (sm_frame_step) as plain C++, no HIP, no library, no device -- and is
 *  built by tests/test_shown_step_host.py with -fsanitize=address,undefined.
 *    lists      random bintree partitions of the coded sizes of tests/golden/DECODED_SHOWN.json (256 x 256, 256 x 192,
 *               100 x 70, 130 x 66, 74 x 138; gray and colour), taken to every magnification from -3 to 2 the size rule
 *               allows by the rule of fa_smoothing_borders_magnified: x and y shifted, the level raised by twice the
 *               magnification, the length the side of the new level clipped at the size shown -- 50 x 36 and 66 x 34 clip
 *               borders at a size that was rounded up to even.  Leaves are large enough that every level stays >= 1.
 *    flights    the planes of one flight share a table of 32 SmDesc, the per-pass ones first and the fused ones behind them
 *               (dec_flight_smooth), and their packed tables lie behind it in 256-byte steps, all in ONE heap block of
 *               exactly the carved size; every plane is a heap block of exactly W x H values.  A fused plane is replayed
 *               as its workgroup runs it: pass after pass -- the barrier --, within a pass the threads in a scrambled
 *               order, each striding the items of the pass by the number of threads the launch would give the block (64
 *               .. 1024).  A per-pass plane runs item by item.  Both must equal the sequential loop over the list, the
 *               reference's order.
 *    policy     sm_fused() is monotone in the pairs and false without passes.
 *  Exit status 0 and "shown_step_check: ok", or 1 and what went wrong.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "libfiasco_amd.h"

#define SMOOTH_HOST_REPLAY 1
#include "smooth.inc"

static const unsigned FLIGHT = 32;       /* DEC_FLIGHT */

static unsigned bad;
#define FAIL(...) do { if (bad++ < 20) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static uint64_t rng_state = 0x2545f4914f6cdd1dull;
static unsigned rnd(unsigned n)              /* 0 .. n - 1 */
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned) ((rng_state >> 11) % n);
}

static size_t align256(size_t v) { return (v + 255) / 256 * 256; }

/* ------------------------------------------------------------------ coded partitions and their magnified lists */

typedef std::vector<std::vector<fiasco_amd_border> > ByLevel;       /* [level] */

/* the block of `level' at (x, y): split down to `leaf'; a split block has its border where its second half begins */
static void split(ByLevel &out, unsigned level, unsigned x, unsigned y, unsigned W, unsigned H, unsigned leaf, unsigned always)
{
    if (x >= W || y >= H || level <= leaf) return;
    if (level <= always && rnd(10) >= 7) return;
    const unsigned w = 1u << (level >> 1), h = 1u << ((level + 1) >> 1);
    fiasco_amd_border b;
    memset(&b, 0, sizeof b);
    b.level = (uint8_t) level;
    if (level & 1) {
        const unsigned yb = y + h / 2;
        if (yb < H) { b.x = (uint16_t) x; b.y = (uint16_t) yb; b.len = (uint16_t) (w < W - x ? w : W - x); out[level].push_back(b); }
        split(out, level - 1, x, y, W, H, leaf, always);
        split(out, level - 1, x, yb, W, H, leaf, always);
    } else {
        const unsigned xb = x + w / 2;
        if (xb < W) { b.x = (uint16_t) xb; b.y = (uint16_t) y; b.len = (uint16_t) (h < H - y ? h : H - y); out[level].push_back(b); }
        split(out, level - 1, x, y, W, H, leaf, always);
        split(out, level - 1, xb, y, W, H, leaf, always);
    }
}

/* the coded list: bands (1 gray, 2 colour: Y and Cb) x levels ascending; no block below level `leaf' + 1 is cut */
static std::vector<fiasco_amd_border> partition(unsigned W, unsigned H, bool colour, unsigned leaf)
{
    unsigned root = 0;
    while ((1u << (root >> 1)) < W || (1u << ((root + 1) >> 1)) < H) root++;
    std::vector<fiasco_amd_border> list;
    unsigned pass = 0;
    for (unsigned band = 0; band < (colour ? 2u : 1u); band++) {
        ByLevel lv(root + 1);
        split(lv, root, 0, 0, W, H, leaf + band, root > 6 ? root - 3 : root);
        for (unsigned l = 0; l <= root; l++) {
            if (lv[l].empty()) continue;
            for (fiasco_amd_border b : lv[l]) { b.pass = (uint8_t) pass; list.push_back(b); }
            pass++;
        }
    }
    return list;
}

/* fiasco_amd_magnified_size()'s rule, restated; false: refused */
static bool shown_size(unsigned W, unsigned H, int m, unsigned *w, unsigned *h)
{
    if (m >= 0) {
        if (((unsigned long long) W * H) << (2 * m) > 2048ull * 2048ull) return false;
        *w = W << m; *h = H << m;
        return true;
    }
    for (int n = 0; n <= -m; n++) if (W >> n < 32 || H >> n < 32) return false;
    *w = W >> -m; *h = H >> -m;
    *w += *w & 1; *h += *h & 1;
    return true;
}

/* the list at magnification m against the size shown: fa_smoothing_borders_magnified's rule on the coded list */
static std::vector<fiasco_amd_border> magnified(const std::vector<fiasco_amd_border> &coded, int m, unsigned w, unsigned h)
{
    std::vector<fiasco_amd_border> out;
    int last = -1;
    unsigned pass = 0;
    for (fiasco_amd_border b : coded) {
        const unsigned x = m >= 0 ? (unsigned) b.x << m : (unsigned) b.x >> -m, y = m >= 0 ? (unsigned) b.y << m : (unsigned) b.y >> -m;
        const int level = (int) b.level + 2 * m;
        if (x >= w || y >= h) continue;
        if (level < 1) { FAIL("a generated border falls to level %d", level); continue; }
        const unsigned side = 1u << sm_log2_side((unsigned) level), room = level & 1 ? w - x : h - y;
        if (last >= 0 && (int) b.pass != last) pass++;
        last = b.pass;
        b.x = (uint16_t) x; b.y = (uint16_t) y; b.level = (uint8_t) level; b.len = (uint16_t) (side < room ? side : room); b.pass = (uint8_t) pass;
        out.push_back(b);
    }
    return out;
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

struct Plane {
    unsigned W = 0, H = 0, np = 0;
    unsigned long long pairs = 0;
    int is = 0, inegs = 0;
    bool fused = false;
    std::vector<fiasco_amd_border> list;
    std::vector<int16_t> want;
    int16_t *plane = nullptr;            /* malloc of exactly W * H values */
    size_t off = 0, bytes = 0;
    unsigned clipped = 0;
};

static void flight(std::vector<Plane> &pl)
{
    static const int percents[3] = { 35, 70, 100 };
    size_t need = 0;
    auto take = [&](size_t bytes) { const size_t at = need; need += align256(bytes); return at; };
    for (Plane &f : pl) {
        char msg[200];
        if (!sm_factors(percents[rnd(3)], &f.is, &f.inegs)) FAIL("no factors");
        if (!sm_check(f.list.data(), (unsigned) f.list.size(), f.W, f.H, &f.np, &f.pairs, msg, sizeof msg)) { FAIL("a magnified list was refused: %s", msg); return; }
        f.bytes = sm_table_bytes((unsigned) f.list.size(), f.np);
        f.plane = (int16_t *) malloc((size_t) f.W * f.H * sizeof(int16_t));
        f.want.resize((size_t) f.W * f.H);
        for (size_t k = 0; k < f.want.size(); k++) f.want[k] = f.plane[k] = (int16_t) (rnd(65536) - 32768);
        sequential(f.want, f.W, f.list, f.is, f.inegs);
    }
    const size_t desc_off = take(FLIGHT * sizeof(SmDesc));
    for (Plane &f : pl) if (f.np) f.off = take(f.bytes);
    char *arena = (char *) malloc(need);
    memset(arena, 0x5a, need);
    for (Plane &f : pl)
        if (f.np && !sm_pack(f.list.data(), (unsigned) f.list.size(), f.np, arena + f.off, f.bytes)) FAIL("sm_pack refused its own carve");
    /* dec_flight_smooth: the per-pass planes first, the fused ones behind them */
    SmDesc *descs = (SmDesc *) (arena + desc_off);
    unsigned n = 0, nper = 0, passes = 0;
    unsigned long long fused_most = 0;
    for (int fused = 0; fused < 2; fused++)
        for (Plane &f : pl) {
            if (!f.np || f.fused != (fused != 0)) continue;
            sm_describe(descs[n++], f.plane, f.W, f.H, arena + f.off, (unsigned) f.list.size(), f.np, f.is, f.inegs);
            if (!fused) { nper++; passes = std::max(passes, f.np); }
            else for (unsigned p = 0; p < f.np; p++) fused_most = std::max(fused_most, sm_pass_items(arena + f.off, (unsigned) f.list.size(), f.np, p));
        }
    /* sm_pass_kernel: one launch per pass for the first nper descriptors */
    for (unsigned p = 0; p < passes; p++)
        for (unsigned y = 0; y < nper; y++) {
            const unsigned long long items = sm_items(descs[y], p), total = (items + 255) / 256 * 256;
            for (unsigned long long j = total; j-- > 0; ) sm_item(descs[y], p, j);
        }
    /* sm_frame_kernel: one block per fused descriptor; the pass loop with its barrier, the threads of a pass scrambled */
    const unsigned threads = fused_most >= 1024 ? 1024u : (unsigned) ((fused_most + 63) / 64 * 64);
    std::vector<unsigned> order(threads);
    for (unsigned k = 0; k < threads; k++) order[k] = k;
    for (unsigned blk = n; blk-- > nper; ) {
        const SmDesc d = descs[blk];
        for (unsigned pass = 0; pass < d.npasses; pass++) {
            for (unsigned k = threads; k > 1; k--) std::swap(order[k - 1], order[rnd(k)]);
            for (unsigned t : order) sm_frame_step(d, pass, t, threads);
        }
    }
    for (Plane &f : pl) {
        if (f.np && memcmp(f.plane, f.want.data(), f.want.size() * sizeof(int16_t)) != 0)
            FAIL("a %s plane of %u x %u (%zu borders, %u passes) differs from the sequential loop", f.fused ? "fused" : "per-pass", f.W, f.H, f.list.size(), f.np);
        free(f.plane);
        f.plane = nullptr;
    }
    free(arena);
}

static void flights(void)
{
    static const struct { unsigned W, H; bool colour; } shapes[7] = {
        { 256, 256, false }, { 256, 256, true }, { 256, 192, true }, { 100, 70, false }, { 130, 66, false }, { 74, 138, true }, { 100, 70, true } };
    unsigned planes = 0, fused = 0, clipped_50x36 = 0, clipped_66x34 = 0, low = 0;
    for (unsigned round = 0; round < 6; round++) {
        std::vector<Plane> pl;
        for (const auto &s : shapes)
            for (int m = -3; m <= 2; m++) {
                Plane f;
                if (!shown_size(s.W, s.H, m, &f.W, &f.H) || (size_t) f.W * f.H > 600000 || pl.size() >= FLIGHT) continue;
                /* leaves of level >= 1 - 2 m: the smallest border of the coded list has that level + 1 at least */
                const unsigned leaf = m < 0 ? (unsigned) (-2 * m) + rnd(2) : 1 + rnd(5);
                f.list = magnified(partition(s.W, s.H, s.colour, leaf), m, f.W, f.H);
                /* round 0 and 1: every plane one way; then mixed, and once by the policy */
                unsigned np = 0; unsigned long long pairs = 0; char msg[200];
                (void) sm_check(f.list.data(), (unsigned) f.list.size(), f.W, f.H, &np, &pairs, msg, sizeof msg);
                f.fused = round == 0 ? true : round == 1 ? false : round == 2 ? sm_fused(pairs, np) : rnd(2) != 0;
                for (const fiasco_amd_border &b : f.list) {
                    const bool clip = b.len < (1u << sm_log2_side(b.level));
                    if (clip && f.W == 50 && f.H == 36) clipped_50x36++;
                    if (clip && f.W == 66 && f.H == 34) clipped_66x34++;
                    if (b.level == 1) low++;
                }
                fused += f.fused;
                pl.push_back(f);
            }
        planes += (unsigned) pl.size();
        flight(pl);
    }
    if (!clipped_50x36 || !clipped_66x34) FAIL("no clipped border at 50 x 36 (%u) or 66 x 34 (%u)", clipped_50x36, clipped_66x34);
    if (!low) FAIL("no border of level 1");
    if (!fused || fused == planes) FAIL("%u of %u planes fused", fused, planes);
    printf("flights: %u planes, %u fused, %u + %u clipped borders at 50 x 36 and 66 x 34, %u borders of level 1\n", planes, fused, clipped_50x36, clipped_66x34, low);
}

static void policy(void)
{
    for (unsigned np : { 1u, 2u, 15u, 40u, 256u }) {
        bool was = true;
        for (unsigned long long pairs = 0; pairs < 3000000; pairs += pairs < 70000 ? 13 : 9973) {
            const bool now = sm_fused(pairs, np);
            if (now && !was) FAIL("sm_fused(%llu, %u) is true after a false", pairs, np);
            was = now;
        }
        if (sm_fused(1ull << 40, np)) FAIL("sm_fused takes a plane of 2^40 pairs");
    }
    if (sm_fused(100, 0)) FAIL("sm_fused takes a plane without passes");
}

int main(void)
{
    policy();
    flights();
    if (bad) { printf("shown_step_check: %u failures\n", bad); return 1; }
    printf("shown_step_check: ok\n");
    return 0;
}
