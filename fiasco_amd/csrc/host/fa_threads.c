/*
 *  fa_threads.c -- the host's one thread fan-out.
 *
 *  Every threaded step of the host layer has the same shape: items 0 .. n - 1 are independent, share t of nt takes
 *  items t, t + nt, ..., and the caller goes on when all of them are done.  What differs from site to site is how
 *  many shares a step wants (computed there, from fa_online_cpus() and the number of items) and what a share does.
 *  Results of a share that the caller needs (a count, the first error text -- the last-error string is per thread)
 *  go through arrays in ctx indexed by t, which one share writes each.
 */
#include <pthread.h>
#include <unistd.h>
#include "fa_host.h"

unsigned fa_online_cpus(void)
{
    long n = sysconf(_SC_NPROCESSORS_ONLN);
    return n < 1 ? 1u : (unsigned) n;
}

typedef struct fan_arg { void (*share)(void *ctx, unsigned t, unsigned nt); void *ctx; unsigned t, nt; } fan_arg;

static void *fan_thread(void *p)
{
    const fan_arg *a = (const fan_arg *) p;
    a->share(a->ctx, a->t, a->nt);
    return NULL;
}

void fa_fan_out(unsigned nt, void (*share)(void *ctx, unsigned t, unsigned nt), void *ctx)
{
    pthread_t th[FA_FAN_MAX];
    fan_arg arg[FA_FAN_MAX];
    int started[FA_FAN_MAX] = { 0 };
    unsigned t;
    nt = nt < 1 ? 1 : nt > FA_FAN_MAX ? FA_FAN_MAX : nt;
    for (t = 1; t < nt; t++) {
        arg[t].share = share; arg[t].ctx = ctx; arg[t].t = t; arg[t].nt = nt;
        started[t] = pthread_create(&th[t], NULL, fan_thread, &arg[t]) == 0;
    }
    share(ctx, 0, nt);
    for (t = 1; t < nt; t++) {
        if (started[t]) pthread_join(th[t], NULL);
        else share(ctx, t, nt);                  /* no thread: the caller does that share */
    }
}
