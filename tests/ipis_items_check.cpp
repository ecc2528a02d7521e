/* Host-side check of the work items of the level recursion (fiasco_amd/csrc/hip/ipt_layout.h: ipis_lanes*, ipis_item_*;
 * op_ipis_t in fc_tables.inc, FC_IPT builds of the frame kernel).
 *
 * The walk below is the kernel's, lane by lane: for every lc_max - images_level in 1 .. 5, every subtree (level,
 * address) op_ipis_t can be called for, first state 0 and 37, 1 .. 70 states and one count above the workgroup size,
 * workgroups of 256 and 1024 lanes.  Per level of the call:
 *   - the items cover every (state, slot) of the call exactly once, and the kernel's loop (state = from + (tid >> lg),
 *     step B >> lg) is the item formula i = tid + k B;
 *   - the lanes of a state are one aligned group of G lanes of one wave, in the same round;
 *   - every load and store is aligned to its width and lies inside its table; the loads of a state's lanes for one term
 *     are consecutive pieces of the domain's row;
 *   - every result carries a distinct value; the kernel's stores (pairs of equal parity for a group of four, single
 *     floats above) must leave in the level's table exactly what ipt_row + ipt_col define for every (state, address) of
 *     the call, each float written once and no other float touched.
 * Built and run by tests/test_ipis_items_host.py; no GPU. */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ipt_layout.h"

static long bad = 0;
#define CHECK(c, ...) do { if (!(c) && bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static const unsigned WAVE = 64;

struct Lane { bool on; unsigned s, j0; float ev[2], od[2]; };

/* the value of the result of (state, level, address): distinct inside a call */
static float value(unsigned s, int lv, unsigned a) { return (float) (1u + a + 32u * (s + 2048u * (unsigned) (lv & 7))); }

static void check_call(int il, int lc_max, unsigned P, unsigned B, int level, unsigned address, unsigned from, unsigned states)
{
    const unsigned NA = 1u << (lc_max - il), NS = 2u * NA - 1u;
    const unsigned image = (1u << (lc_max - level)) - 1u + address;
    std::vector<float> ipt((size_t) NA * P, 0.0f);
    std::vector<unsigned char> wrote((size_t) NA * P, 0);
    std::vector<unsigned char> slotw((size_t) NS * P, 0);
    for (int lv = il + 1; lv <= level; lv++) {
        const int delta = level - lv;
        const unsigned cnt = 1u << delta, adr0 = address << delta, slot0 = ((image + 1u) << delta) - 1u;
        const unsigned n = ipt_n(lc_max, lv), w = ipt_width(cnt);
        const bool first = lv == il + 1;
        const unsigned lg = ipis_lanes_log2(cnt), G = ipis_lanes(cnt);
        CHECK(G == (cnt >= 8 ? cnt / 4 : 1) && G == 1u << lg, "cnt %u: %u lanes per state", cnt, G);
        CHECK(WAVE % G == 0 && B % G == 0, "cnt %u: %u lanes per state do not divide the wave or the workgroup", cnt, G);
        const unsigned nitems = (states - from) * G, rounds = (nitems + B - 1) / B;
        std::vector<unsigned> seen((size_t) (states - from) * cnt, 0u);
        std::vector<size_t> touched;
        for (unsigned k = 0; k < rounds; k++)
            for (unsigned w0 = 0; w0 < B; w0 += WAVE) {
                Lane L[WAVE];
                for (unsigned q = 0; q < WAVE; q++) {
                    const unsigned tid = w0 + q, i = tid + k * B;
                    Lane &l = L[q];
                    /* the kernel's loop against the item formula */
                    const unsigned s = from + ipis_item_state(tid, lg) + k * (B >> lg), j0 = ipis_item_j0(tid, lg);
                    l.on = s < states;
                    CHECK(l.on == (i < nitems), "item %u of %u: state %u of %u", i, nitems, s, states);
                    if (!l.on) continue;
                    CHECK(s == from + ipis_item_state(i, lg) && j0 == ipis_item_j0(i, lg) && s == from + i / G && j0 == 4 * (i % G),
                          "item %u: state %u group %u, expected state %u group %u", i, s, j0, from + i / G, 4 * (i % G));
                    l.s = s; l.j0 = j0;
                    CHECK(j0 + w <= cnt, "item %u: slots %u + %u of %u", i, j0, w, cnt);
                    /* an aligned group of one wave: the first lane of the state is q - q % G, all of them in this wave */
                    CHECK((q % G) * 4 == j0 && q - q % G + G <= WAVE, "item %u: lane %u is not lane %u of its state's group", i, q, j0 / 4);
                    if (q % G) CHECK(L[q - 1].on && L[q - 1].s == s && L[q - 1].j0 + 4 == j0, "item %u: the lane before it serves another state", i);
                    /* the loads of one term and label: domain d, row of rs floats, label half lb */
                    const unsigned doms[] = { 0, 1, P / 2 + 1, P - 1 };
                    for (unsigned d : doms)
                        for (unsigned lab = 0; lab < 2; lab++) {
                            const unsigned rs = first ? NA : 2 * n;
                            const unsigned lb = first ? lab * (NA >> 1) : ipt_row(P, NA, 2 * n, 0) + ipt_src_col(n, lab, 0);
                            const unsigned o = d * rs + lb + adr0 + j0;
                            CHECK(o % w == 0 && o + w <= NA * P, "item %u lv %d domain %u: load of %u floats at %u", i, lv, d, w, o);
                            if (first)
                                CHECK(o + w <= d * NA + (lab + 1) * (NA >> 1) && o >= d * NA + lab * (NA >> 1), "item %u: load at %u leaves the label's half of the row of dots", i, o);
                            else
                                for (unsigned x = 0; x < w; x++)
                                    CHECK(o + x == ipt_row(P, NA, 2 * n, d) + ipt_col(2 * n, 2 * (adr0 + j0 + x) + lab), "item %u lv %d: float %u of the load is not the source of slot %u", i, lv, x, adr0 + j0 + x);
                            /* contiguous inside the lane group: lane c reads the c-th piece from the group's first on */
                            CHECK(o == d * rs + lb + adr0 + 4 * (q % G), "item %u: its load is not piece %u of the group's", i, q % G);
                        }
                    /* results: slot-major stores, one float each */
                    float res[4] = { 0, 0, 0, 0 };
                    for (unsigned jj = 0; jj < w; jj++) {
                        res[jj] = value(s, lv, adr0 + j0 + jj);
                        seen[(size_t) (s - from) * cnt + j0 + jj]++;
                        const size_t o = (size_t) s + (size_t) (slot0 + j0 + jj) * P;
                        CHECK(o < (size_t) NS * P && s < P, "item %u: slot-major store at %zu", i, o);
                        if (o < (size_t) NS * P) { CHECK(!slotw[o], "item %u: slot-major float %zu written twice", i, o); slotw[o] = 1; }
                    }
                    l.ev[0] = res[0]; l.ev[1] = res[2]; l.od[0] = res[1]; l.od[1] = res[3];
                }
                if (lv >= lc_max) continue;
                /* the stores into the level's table, as the kernel chooses them */
                for (unsigned q = 0; q < WAVE; q++) {
                    const Lane &l = L[q];
                    if (!l.on) continue;
                    const unsigned a0 = adr0 + l.j0, row = ipt_row(P, NA, n, l.s);
                    auto put = [&](unsigned o, unsigned width, const float *v) {
                        CHECK(o % width == 0 && o + width <= NA * P && o >= row && o + width <= row + n, "lv %d state %u: store of %u floats at %u (row %u + %u)", lv, l.s, width, o, row, n);
                        for (unsigned x = 0; x < width && o + x < NA * P; x++) {
                            CHECK(!wrote[o + x], "lv %d state %u: float %u stored twice", lv, l.s, o + x);
                            wrote[o + x] = 1; ipt[o + x] = v[x]; touched.push_back(o + x);
                        }
                    };
                    if (cnt >= 4) {
                        put(row + ipt_col(n, a0), 2, l.ev);
                        put(row + ipt_col(n, a0 + 1), 2, l.od);
                    } else {
                        put(row + ipt_col(n, a0), 1, &l.ev[0]);
                        if (cnt == 2) put(row + ipt_col(n, a0 + 1), 1, &l.od[0]);
                    }
                }
            }
        for (size_t x = 0; x < seen.size(); x++)
            CHECK(seen[x] == 1, "lv %d: slot %zu of state %zu served %u times", lv, x % cnt, from + x / cnt, seen[x]);
        if (lv < lc_max) {
            /* the parent's contents, entry for entry, and nothing else */
            CHECK(touched.size() == (size_t) (states - from) * cnt, "lv %d: %zu floats stored, %zu results", lv, touched.size(), (size_t) (states - from) * cnt);
            for (unsigned s = from; s < states; s++)
                for (unsigned a = adr0; a < adr0 + cnt; a++) {
                    const unsigned o = ipt_row(P, NA, n, s) + ipt_col(n, a);
                    CHECK(wrote[o] && ipt[o] == value(s, lv, a), "lv %d state %u address %u: float %u holds %g, expected %g", lv, s, a, o, ipt[o], value(s, lv, a));
                }
            for (size_t o : touched) { wrote[o] = 0; ipt[o] = 0.0f; }
        }
    }
}

int main()
{
    long calls = 0;
    const unsigned Bs[] = { 256, 1024 }, froms[] = { 0, 37 };
    for (unsigned B : Bs)
        for (int D = 1; D <= 5; D++) {
            const int il = 5, lc_max = il + D;
            const unsigned P = 1200;
            for (int level = il + 1; level <= lc_max; level++)
                for (unsigned address = 0; address < (1u << (lc_max - level)); address++)
                    for (unsigned from : froms) {
                        for (unsigned ns = 1; ns <= 70; ns++) { check_call(il, lc_max, P, B, level, address, from, from + ns); calls++; }
                        check_call(il, lc_max, P, B, level, address, from, from + B + 37); calls++;
                    }
        }
    if (bad) { printf("ipis_items_check: %ld failures\n", bad); return 1; }
    printf("ipis_items_check: ok (%ld calls)\n", calls);
    return 0;
}
