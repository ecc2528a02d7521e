/* Host-side check of the state-major copy of the level recursion's sources (fiasco_amd/csrc/hip/ipt_layout.h,
 * DevFrame.ipt, FC_IPT builds of the frame kernel) and of the room make_layout() (enc_layout.inc) gives it.
 *
 * Layout, for every lc_max - images_level in 1 .. 5 and two capacities: the entries of all (state, level, address)
 * are distinct and inside the NA * P floats of the buffer; the source of slot (lv, a), label l, in domain d is the
 * entry of (d, lv - 1, 2 a + l).
 * Accesses, for every subtree (image, address, level) op_ipis_t can be called for: the walk below is the kernel's --
 * levels images_level + 1 .. level, cnt = 2^(level - lv) slots from address adr0 = address << (level - lv) in groups of
 * four; one load of ipt_width(cnt) floats per term and label, from the level-images_level dots at the first level
 * and from the domain's row of the level below above it; below lc_max the results into the state's row, the even and
 * the odd addresses of a group of four as two pairs -- and every one of them must be aligned to its width, stay inside
 * its row, and hold the entries the kernel takes out of it.
 * make_layout: the slab grows by NA * P * 4 bytes rounded to 256 and by nothing else, and 256 slabs of a 4K frame
 * (triangular Gram tables, tight capacity: what fit_hbm() arrives at) still fit 288 GB of HBM.
 * Built and run by tests/test_ipt_layout_host.py; no GPU. */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "fa_host.h"
#include "frame_coder.h"
#include "ipt_layout.h"

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
#include "enc_layout.inc"

static long bad = 0;
#define CHECK(c, ...) do { if (!(c) && bad++ < 10) { printf(__VA_ARGS__); printf("\n"); } } while (0)

static void check_geometry(int il, int lc_max, unsigned P)
{
    const unsigned NA = 1u << (lc_max - il);
    const int D = lc_max - il;
    /* distinct, inside the buffer: who owns a float (level * P + state + 1) */
    std::vector<unsigned> owner((size_t) NA * P, 0u);
    for (int lv = il + 1; lv < lc_max; lv++) {
        const unsigned n = ipt_n(lc_max, lv);
        for (unsigned s = 0; s < P; s++)
            for (unsigned a = 0; a < n; a++) {
                const unsigned o = ipt_row(P, NA, n, s) + ipt_col(n, a);
                CHECK(ipt_col(n, a) < n && o < NA * P, "D %d level %d state %u address %u: float %u outside the buffer", D, lv, s, a, o);
                if (o >= NA * P) continue;
                CHECK(!owner[o], "D %d level %d state %u address %u: float %u taken", D, lv, s, a, o);
                owner[o] = (unsigned) lv * P + s + 1;
            }
    }
    /* the source of a slot is the domain's entry one level down */
    const unsigned doms[] = { 0, 1, P / 2 + 1, P - 1 };
    for (int lv = il + 2; lv <= lc_max; lv++) {
        const unsigned n = ipt_n(lc_max, lv);
        for (unsigned d : doms)
            for (unsigned a = 0; a < n; a++)
                for (unsigned l = 0; l < 2; l++)
                    CHECK(ipt_row(P, NA, 2 * n, d) + ipt_src_col(n, l, a) == ipt_row(P, NA, 2 * n, d) + ipt_col(2 * n, 2 * a + l),
                          "D %d level %d address %u label %u: source column %u, entry column %u", D, lv, a, l, ipt_src_col(n, l, a), ipt_col(2 * n, 2 * a + l));
    }
    /* the kernel's accesses, subtree by subtree */
    for (int level = il + 1; level <= lc_max; level++)
        for (unsigned address = 0; address < (1u << (lc_max - level)); address++) {
            const unsigned image = (1u << (lc_max - level)) - 1 + address;
            for (int lv = il + 1; lv <= level; lv++) {
                const int delta = level - lv;
                const unsigned cnt = 1u << delta, adr0 = address << delta, slot0 = ((image + 1) << delta) - 1;
                const unsigned n = ipt_n(lc_max, lv), w = ipt_width(cnt);
                CHECK(slot0 == (1u << (lc_max - lv)) - 1 + adr0, "image %u level %d: slot %u is not address %u of level %d", image, level, slot0, adr0, lv);
                CHECK(adr0 % cnt == 0 && adr0 + cnt <= n, "image %u level %d: slots %u + %u of level %d", image, level, adr0, cnt, lv);
                for (unsigned j0 = 0; j0 < cnt; j0 += 4) {
                    const unsigned a0 = adr0 + j0, g = cnt - j0 < 4 ? cnt - j0 : 4;
                    CHECK(g == w, "image %u level %d lv %d: a group of %u slots, loads of %u", image, level, lv, g, w);
                    if (lv == il + 1)          /* the loads from the row of level-images_level dots (D5_AT), NA floats per state */
                        for (unsigned l = 0; l < 2; l++) {
                            const unsigned o = l * (NA >> 1) + a0;
                            CHECK(o % w == 0 && NA % w == 0 && o + w <= (l + 1) * (NA >> 1), "image %u level %d: load of %u dots at %u (row of %u)", image, level, w, o, NA);
                        }
                    else
                        for (unsigned d : doms)
                            for (unsigned l = 0; l < 2; l++) {
                                /* what the kernel computes: domain * floats per state + (table + label half) + address */
                                const unsigned rs = 2 * n, lb = ipt_row(P, NA, 2 * n, 0) + ipt_src_col(n, l, 0), o = d * rs + lb + a0;
                                CHECK(o % w == 0, "image %u level %d lv %d domain %u: load of %u floats at %u", image, level, lv, d, w, o);
                                for (unsigned k = 0; k < w; k++) {
                                    CHECK(o + k < NA * P && owner[o + k] == (unsigned) (lv - 1) * P + d + 1, "image %u level %d lv %d domain %u: float %u is not the domain's, level %d",
                                          image, level, lv, d, o + k, lv - 1);
                                    CHECK(o + k == ipt_row(P, NA, 2 * n, d) + ipt_col(2 * n, 2 * (a0 + k) + l), "image %u level %d lv %d label %u: float %u of the load is not the source of slot %u",
                                          image, level, lv, l, k, a0 + k);
                                }
                            }
                    if (lv < lc_max)
                        for (unsigned s : doms) {
                            const unsigned row = ipt_row(P, NA, n, s);
                            if (cnt >= 4)
                                for (unsigned par = 0; par < 2; par++) {
                                    const unsigned o = row + ipt_col(n, a0 + par);
                                    CHECK(o % 2 == 0, "image %u level %d lv %d state %u: store of 2 floats at %u", image, level, lv, s, o);
                                    CHECK(o + 1 == row + ipt_col(n, a0 + par + 2), "image %u level %d lv %d: address %u is not the neighbour of %u", image, level, lv, a0 + par + 2, a0 + par);
                                }
                            for (unsigned k = 0; k < g; k++) {
                                const unsigned o = row + ipt_col(n, a0 + k);
                                CHECK(o < NA * P && owner[o] == (unsigned) lv * P + s + 1, "image %u level %d lv %d state %u: result of address %u lands at %u", image, level, lv, s, a0 + k, o);
                            }
                        }
                }
            }
        }
}

static void check_slab()
{
    /* default geometry (block levels 6 .. 10), 1080p gray and 4K gray with triangular tables at the tight capacity */
    struct { int P, tri; size_t npix; } f[] = { { 2880, 0, (size_t) 1920 * 1080 }, { 9472, 1, (size_t) 3840 * 2160 }, { 64, 0, 32 * 32 } };
    for (int D = 1; D <= 5; D++)
        for (auto &c : f) {
            const int il = 5, NA = 1 << D, NS = (2 << D) - 1, NL = D + 1, NI = 63;
            const Layout L = make_layout(c.P, c.P, NL, NS, NA, NI, il, 0, c.npix, 0, 0, 1, 0, c.tri != 0, false);
            const size_t ipt_bytes = align_up((size_t) NA * c.P * 4, 256);
            CHECK(L.ipt % 256 == 0 && L.ipt == L.d5 + align_up((size_t) NA * c.P * 4, 256) && L.d4 == L.ipt + ipt_bytes,
                  "D %d P %d: ipt at %zu between d5 at %zu and d4 at %zu", D, c.P, L.ipt, L.d5, L.d4);
            /* what the slab held without it: every array behind ipt moves down by exactly its size */
            size_t sum = 0;
#define PART(field, bytes) sum += align_up((bytes), 256)
            PART(gram, c.tri ? (size_t) NL * ((size_t) c.P * (c.P + 1) / 2 + c.P) * 4 : (size_t) NL * c.P * c.P * 4);
            PART(gcol, c.tri ? (size_t) NL * FC_TRI_HOT * c.P * 4 : 0);
            PART(diag, (size_t) NL * c.P * 4);
            PART(ipis, (size_t) NS * c.P * 4);
            PART(d5, (size_t) NA * c.P * 4);
#undef PART
            CHECK(L.ipt == sum, "D %d P %d: ipt at %zu, the arrays in front of it end at %zu", D, c.P, L.ipt, sum);
            CHECK(L.total > L.pix16 && L.pix16 > L.ipt, "D %d P %d: totals", D, c.P);
            if (D == 5 && c.tri) {
                const double before = 256.0 * (double) (L.total - ipt_bytes), after = 256.0 * (double) L.total;
                printf("4K, 256 slabs: %.2f GB without, %.2f GB with ipt (%.1f MB per frame)\n", before / 1e9, after / 1e9, ipt_bytes / 1e6);
                CHECK(after <= 288e9, "256 slabs of a 4K frame need %.1f GB", after / 1e9);
            }
        }
}

/* the extra bytes of a slab: the same layout with the ipt part taken out again */
static void check_extra()
{
    const int P = 2880, NA = 32;
    const Layout L = make_layout(P, P, 6, 31, NA, 63, 5, 0, (size_t) 1920 * 1080, 0, 0, 1, 0, false, false);
    const Layout Z = make_layout(P, P, 6, 31, 0, 63, 5, 0, (size_t) 1920 * 1080, 0, 0, 1, 0, false, false);   /* NA = 0: no d5, no ipt, empty coop pixels aside */
    const size_t one = align_up((size_t) NA * P * 4, 256);
    CHECK(L.imgT - Z.imgT == 2 * one, "d5 + ipt take %zu bytes, expected 2 x %zu", L.imgT - Z.imgT, one);
    CHECK(L.total - Z.total == 2 * one, "slab grows by %zu bytes over one without d5 and ipt, expected %zu", L.total - Z.total, 2 * one);
}

int main()
{
    for (int D = 1; D <= 5; D++) { check_geometry(5, 5 + D, 64); check_geometry(5, 5 + D, 2880); }
    check_slab();
    check_extra();
    if (bad) { printf("ipt_layout_check: %ld failures\n", bad); return 1; }
    printf("ipt_layout_check: ok\n");
    return 0;
}
