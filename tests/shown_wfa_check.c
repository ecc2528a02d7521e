/*
 *  shown_wfa_check.c -- fa_smoothing_borders_magnified() (csrc/host/fa_batch_decode.c) on automata built by hand.
 *
 *  A stand-alone program, linked by tests/test_shown_api.py against the CPU oracle library, which holds the product's host
 *  code.  A gray automaton of three states in a frame of 64 x 64:
 *    state 1   level 2 (2 x 2), its second half begins at (1, 0): the only state whose level falls below 1 at -1, and the
 *              shift puts it on (0, 0) -- where smooth_image would blend with the word before the plane
 *    state 2   level 8 (16 x 16) at (32, 0): cut at x = 40
 *    state 3   level 9 (16 x 32) at (16, 0): cut at y = 16
 *  At 0 and 1 the list has three borders; at -1 the frame is refused with a message that names the magnification and the
 *  level; with state 1 out of sight (beyond the frame) -1 gives the two others shifted; -2 is the size rule's to refuse.
 *  Exit status 0 and "shown_wfa_check: ok", or 1 and what went wrong.
 */
#include <stdio.h>
#include <string.h>
#include "fa_host.h"

static unsigned bad;
#define FAIL(...) do { bad++; printf(__VA_ARGS__); printf("\n"); } while (0)

static void put(fa_wfa *w, unsigned s, unsigned level, unsigned x1, unsigned y1)
{
    w->level_of_state[s] = (uint8_t) level;
    w->x[s * 2 + 1] = (uint16_t) x1; w->y[s * 2 + 1] = (uint16_t) y1;
}

static int same(const fiasco_amd_border *b, unsigned x, unsigned y, unsigned len, unsigned level, unsigned pass)
{
    return b->x == x && b->y == y && b->len == len && b->level == level && b->pass == pass;
}

int main(void)
{
    fa_wfa *w = fa_wfa_alloc(8);
    fiasco_amd_border out[8];
    unsigned n;
    if (!w) { printf("no automaton\n"); return 1; }
    w->basis_states = 1; w->states = 4; w->root_state = 3;
    put(w, 1, 2, 1, 0);
    put(w, 2, 8, 40, 0);
    put(w, 3, 9, 16, 16);
    n = fa_smoothing_borders_magnified(w, 64, 64, 0, 0, out, 8);
    if (n != 3 || n != fa_smoothing_borders(w, 64, 64, 0, NULL, 0)) FAIL("magnification 0: %u borders", n);
    else if (!same(&out[0], 1, 0, 2, 2, 0) || !same(&out[1], 40, 0, 16, 8, 1) || !same(&out[2], 16, 16, 16, 9, 2)) FAIL("magnification 0: another list");
    n = fa_smoothing_borders_magnified(w, 64, 64, 0, 1, out, 8);
    if (n != 3 || !same(&out[0], 2, 0, 4, 4, 0) || !same(&out[1], 80, 0, 32, 10, 1) || !same(&out[2], 32, 32, 32, 11, 2)) FAIL("magnification 1: %u borders", n);
    /* -1: state 1 falls to level 0 at (0, 0) */
    fa_set_error("%s", "");
    n = fa_smoothing_borders_magnified(w, 64, 64, 0, -1, out, 8);
    if (n != 0) FAIL("magnification -1: %u borders where the frame must be refused", n);
    else {
        const char *msg = fiasco_get_error_message();
        if (!strstr(msg, "magnification -1") || !strstr(msg, "level 2 falls to level 0") || !strstr(msg, "undefined")) FAIL("the refusal says: %s", msg);
    }
    if (fa_smoothing_borders_magnified(w, 64, 64, 0, -1, NULL, 0) != 0) FAIL("counting alone does not refuse");
    /* the same state out of sight: nothing low is listed */
    put(w, 1, 2, 65, 0);
    fa_set_error("%s", "");
    n = fa_smoothing_borders_magnified(w, 64, 64, 0, -1, out, 8);
    if (n != 2 || !same(&out[0], 20, 0, 8, 6, 0) || !same(&out[1], 8, 8, 8, 7, 1)) FAIL("magnification -1, low state out of sight: %u borders (%s)", n, fiasco_get_error_message());
    if (fa_smoothing_borders_magnified(w, 64, 64, 0, -1, out, 1) != 0 || !strstr(fiasco_get_error_message(), "more than 1 borders")) FAIL("no room was not refused");
    /* 64 >> 2 = 16 < 32: the size rule */
    n = fa_smoothing_borders_magnified(w, 64, 64, 0, -2, out, 8);
    if (n != 0 || !strstr(fiasco_get_error_message(), "Minimum value is -1.")) FAIL("magnification -2: %u borders, %s", n, fiasco_get_error_message());
    fa_wfa_free(w);
    if (bad) { printf("shown_wfa_check: %u failures\n", bad); return 1; }
    printf("shown_wfa_check: ok\n");
    return 0;
}
