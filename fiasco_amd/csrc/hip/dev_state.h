/*
 *  dev_state.h -- what the launcher keeps between calls for ONE device share, and the lock that makes it safe to use
 *  from several host threads at once (included by core_hip.cpp).
 *
 *  Host code only: nothing here needs the HIP runtime, so a program without a device (tests/dev_state_check.cpp, built
 *  under the thread and address sanitizers) includes this file and slab_pool.inc over a fake of the few HIP calls the
 *  pool makes.
 *
 *  Everything the launcher keeps between calls belongs to ONE device: the pool of slabs, the log2 correction table,
 *  the counters.  A process that encodes on one device (the default on a 1-GPU box, a rank of the multi-process
 *  harness after fiasco_amd_set_device()) uses g_state0 from whatever thread calls in: it is the state of share 0,
 *  the first of the list that shares.inc keeps.  The multi-device entries there give every further device a DevState
 *  of its own and run its share of a batch on a host thread whose t_dev points there.
 *
 *  Threading.  Several callers work on one DevState at the same time -- every thread of a process with one device, and
 *  with several shares a caller whose only part lies on share k beside worker k of another caller's batch.  DevState::mu
 *  guards the pool's vector with the allocations and frees behind it (slab_pool.inc), the counters (stats_update,
 *  fiasco_amd_get_stats / _reset_stats) and the state of the log2 table's once-guard (l2_once).  It is held for
 *  host work and memory management only: never across a launch, a stream wait or a download.
 */
#ifndef FA_DEV_STATE_H
#define FA_DEV_STATE_H 1
#include <pthread.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "libfiasco_amd_hip.h"

struct PoolEntry { char *base; size_t bytes; int device; };   /* device: where hipMalloc gave the slab out (checked on every acquire) */
/* the log2 correction table of a share: built for `device'; state and device belong to l2_once() (DevState::mu) */
enum L2State { L2_NONE, L2_BUILDING, L2_OK, L2_FAILED };
struct Log2Patch { unsigned *d_keys = nullptr; double *d_vals = nullptr; unsigned mask = 0; int device = -1;
                   unsigned long long entries = 0; L2State state = L2_NONE; };
struct DevState {
    pthread_mutex_t mu;
    pthread_cond_t  l2_built;           /* a build of the log2 table has ended */
    fiasco_amd_stats stats;
    std::vector<PoolEntry> free;
    Log2Patch l2;
    char l2_err[200];                   /* why the last build of l2 failed: written by the builder, kept while l2 is L2_FAILED */
    DevState()
    {
        pthread_mutex_init(&mu, nullptr); pthread_cond_init(&l2_built, nullptr);
        memset(&stats, 0, sizeof stats); l2_err[0] = 0;
    }
};
static DevState g_state0;
static thread_local DevState *t_dev = &g_state0;
#define g_l2     (t_dev->l2)
#define g_l2_err (t_dev->l2_err)

/* holds the lock of a share for a scope */
struct DevLock {
    DevState *st;
    explicit DevLock(DevState *s) : st(s) { pthread_mutex_lock(&st->mu); }
    ~DevLock() { pthread_mutex_unlock(&st->mu); }
    DevLock(const DevLock &) = delete;
    DevLock &operator=(const DevLock &) = delete;
};

/* every change of the calling thread's share's counters: fn(stats) under the share's lock */
template <typename Fn> static void stats_update(Fn fn)
{
    DevLock lock(t_dev);
    fn(t_dev->stats);
}

/* The log2 table of share `st' for device `dev', built ONCE however many threads ask at the same time: the first
 * caller runs build() -- without the lock: it launches kernels and waits for them --, callers that arrive meanwhile
 * wait and leave with the builder's result and the builder's text in st->l2_err.  A failed build stays failed for that
 * device; another device builds again (build() drops what the table of the old one holds).  build() sets every field
 * of st->l2 but `state' and `device', and st->l2_err when it fails.  err (n bytes): the reason when the answer is
 * false, copied under the lock. */
template <typename Build> static bool l2_once(DevState *st, int dev, Build build, char *err, size_t n)
{
    pthread_mutex_lock(&st->mu);
    while (st->l2.state == L2_BUILDING) pthread_cond_wait(&st->l2_built, &st->mu);
    if (st->l2.state == L2_NONE || st->l2.device != dev) {
        st->l2.state = L2_BUILDING; st->l2.device = dev;
        st->l2_err[0] = 0;
        pthread_mutex_unlock(&st->mu);
        const bool ok = build();
        pthread_mutex_lock(&st->mu);
        st->l2.device = dev;
        st->l2.state = ok ? L2_OK : L2_FAILED;
        pthread_cond_broadcast(&st->l2_built);
    }
    const bool ok = st->l2.state == L2_OK;
    if (err && n) snprintf(err, n, "%s", ok ? "" : st->l2_err);
    pthread_mutex_unlock(&st->mu);
    return ok;
}

#endif
