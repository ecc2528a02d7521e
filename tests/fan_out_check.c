/*
 *  fan_out_check.c -- fa_fan_out() (csrc/host/fa_threads.c) on its own, for the sanitizers.
 *
 *  A stand-alone program: it compiles fa_threads.c itself (no library is loaded) and is built twice by
 *  tests/test_host_api.py, with -fsanitize=thread and with -fsanitize=address,undefined.  For every thread count and
 *  item count below, with every thread starting and with every second thread refusing to start (those shares must
 *  run on the caller), it checks that
 *    - every item is visited exactly once (the visits are plain increments: two shares on one item are a data race
 *      the thread sanitizer reports, and a count other than 1 here);
 *    - the slot of share t is written by one share, slots past the clamped count by none;
 *    - every share sees the same nt, clamped to 1 .. FA_FAN_MAX.
 *  Exit status 0 and "fan_out_check: ok", or 1 and what went wrong.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* pthread_create as fa_threads.c sees it: refuses every second thread while `flaky' is set */
static int flaky;
static unsigned created, refused;
static int flaky_create(pthread_t *th, const pthread_attr_t *attr, void *(*fn)(void *), void *arg)
{
    if (flaky && (created + refused) % 2) { refused++; return 11; }
    created++;
    return pthread_create(th, attr, fn, arg);
}
#define pthread_create flaky_create
#include "fa_threads.c"
#undef pthread_create

enum { SLOTS = FA_FAN_MAX + 2 };
typedef struct { unsigned items, *visits, slot[SLOTS], seen_nt[SLOTS]; } check;

static void visit(void *ctx, unsigned t, unsigned nt)
{
    check *c = (check *) ctx;
    unsigned i;
    if (t < SLOTS) { c->slot[t]++; c->seen_nt[t] = nt; }
    for (i = t; i < c->items; i += nt) c->visits[i]++;
}

int main(void)
{
    static const unsigned counts[] = { 0, 1, 2, 7, 32, 33 }, sizes[] = { 0, 1, 31, 1000 };
    unsigned a, b, i, bad = 0;
    if (fa_online_cpus() < 1) { printf("fa_online_cpus() = 0\n"); bad++; }
    for (flaky = 0; flaky < 2; flaky++)
        for (a = 0; a < sizeof counts / sizeof counts[0]; a++)
            for (b = 0; b < sizeof sizes / sizeof sizes[0]; b++) {
                const unsigned nt = counts[a], want = nt < 1 ? 1 : nt > FA_FAN_MAX ? FA_FAN_MAX : nt;
                check c;
                memset(&c, 0, sizeof c);
                c.items = sizes[b];
                c.visits = (unsigned *) calloc(c.items + 1, sizeof *c.visits);
                if (!c.visits) return 2;
                created = refused = 0;
                fa_fan_out(nt, visit, &c);
                for (i = 0; i < c.items; i++)
                    if (c.visits[i] != 1) { printf("nt %u items %u flaky %d: item %u visited %u times\n", nt, c.items, flaky, i, c.visits[i]); bad++; break; }
                for (i = 0; i < SLOTS; i++)
                    if (c.slot[i] != (i < want) || (i < want && c.seen_nt[i] != want)) {
                        printf("nt %u items %u flaky %d: slot %u written %u times, nt seen %u, wanted %u\n", nt, c.items, flaky, i, c.slot[i], c.seen_nt[i], want);
                        bad++; break;
                    }
                if (created + refused != want - 1 || (flaky && refused != (want - 1) / 2)) {
                    printf("nt %u flaky %d: %u threads started, %u refused\n", nt, flaky, created, refused);
                    bad++;
                }
                free(c.visits);
            }
    if (!bad) printf("fan_out_check: ok\n");
    return bad ? 1 : 0;
}
