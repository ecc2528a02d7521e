/*
 *  dev_state_check.cpp -- what several caller threads share on one device share (csrc/hip/dev_state.h, slab_pool.inc)
 *  on its own, for the sanitizers.
 *
 *  A stand-alone program: it includes the two files over tests/fake_hip_pool.h (no library is loaded, no device is
 *  needed) and is built twice by tests/test_host_api.py, with -fsanitize=thread and with -fsanitize=address,undefined.
 *    pool     eight threads, a few thousand acquire / stamp / re-read / release rounds each, sizes of three classes --
 *             two inside the 25 % reuse window of each other, one outside -- under a budget so tight that the "drop the
 *             pool and try once more" branch runs while others stage.  No slab has two holders (a holder writes its id
 *             through the whole slab and finds it intact before release: plain stores, a second holder is a data race
 *             the thread sanitizer reports and a foreign byte here), *got covers the request, no request fails, and
 *             after the pool is emptied every allocation has been freed exactly once.
 *    tags     an entry released while another device is current keeps the tag of the device that allocated it and is
 *             not handed to a thread on another device (the pool says so, once).
 *    once     eight threads ask for the log2 table at a barrier, the build sleeps 50 ms: one build, one answer and one
 *             error text for all; a failed build is not tried again on that device; another device builds once more.
 *    counters concurrent increments through stats_update() sum exactly.
 *  Exit status 0 and "dev_state_check: ok", or 1 and what went wrong.
 */
#include <pthread.h>
#include <sched.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <atomic>
#include <vector>
#include "fake_hip_pool.h"
#include "dev_state.h"

/* what the pool prints (an entry that met another device): kept here, the program's stderr stays empty */
static char said[200];
static unsigned said_n;
static int pool_says(FILE *, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(said, sizeof said, fmt, ap);
    va_end(ap);
    said_n++;
    return 0;
}
#define fprintf pool_says
#include "slab_pool.inc"
#undef fprintf

enum { THREADS = 8, ROUNDS = 3000 };
static const size_t CLASS[3] = { 4096, 4608, 8192 };     /* 4608 <= 4096 + 4096 / 4; 8192 is outside both windows */

static unsigned bad;
static pthread_mutex_t bad_mu = PTHREAD_MUTEX_INITIALIZER;
static void fail(const char *fmt, ...)
{
    va_list ap;
    pthread_mutex_lock(&bad_mu);
    if (bad++ < 20) { va_start(ap, fmt); vprintf(fmt, ap); va_end(ap); printf("\n"); }
    pthread_mutex_unlock(&bad_mu);
}

static pthread_barrier_t gate;

/* ---- pool ---- */

static void *pool_thread(void *arg)
{
    const unsigned me = (unsigned) (size_t) arg;
    unsigned rnd = 12345u + 977u * me;
    pthread_barrier_wait(&gate);
    for (unsigned r = 0; r < ROUNDS; r++) {
        rnd = rnd * 1664525u + 1013904223u;
        const size_t want = CLASS[(rnd >> 16) % 3];
        size_t got = 0;
        int dev = -7;
        char *p = slab_acquire(want, &got, &dev);
        if (!p) { fail("thread %u round %u: no slab of %zu bytes", me, r, want); continue; }
        if (got < want || got > want + want / 4) fail("thread %u round %u: asked for %zu bytes, got %zu", me, r, want, got);
        if (dev != 0) fail("thread %u round %u: slab tagged device %d", me, r, dev);
        memset(p, (int) (me + 1), got);
        if (r % 8 == 0) sched_yield();
        for (size_t i = 0; i < got; i++)
            if ((unsigned char) p[i] != me + 1) { fail("thread %u round %u: byte %zu of its slab belongs to holder %u", me, r, i, (unsigned) (unsigned char) p[i]); break; }
        slab_release(p, got, dev);
    }
    return nullptr;
}

static void check_pool(void)
{
    pthread_t th[THREADS];
    /* every thread can hold a slab of the largest class, and half a slab more: the pool's idle entries of the other
     * classes have to go before the next allocation fits */
    fake_hip::budget = THREADS * CLASS[2] + CLASS[0];
    pthread_barrier_init(&gate, nullptr, THREADS);
    for (size_t t = 0; t < THREADS; t++) pthread_create(&th[t], nullptr, pool_thread, (void *) t);
    for (size_t t = 0; t < THREADS; t++) pthread_join(th[t], nullptr);
    pthread_barrier_destroy(&gate);
    /* nothing but the drop branch frees while callers stage */
    if (fake_hip::frees.load() == 0) fail("pool: the drop-and-retry branch never ran (%llu allocations refused)", fake_hip::refused.load());
    if (pool_bytes() != fake_hip::used.load()) fail("pool: holds %zu bytes, %zu are allocated", pool_bytes(), fake_hip::used.load());
    { DevLock lock(&g_state0); pool_drop_locked(&g_state0); }
    if (fake_hip::mallocs.load() != fake_hip::frees.load() || fake_hip::bad_frees.load() || fake_hip::used.load())
        fail("pool: %llu allocations, %llu frees, %llu of them of a block not live, %zu bytes left", fake_hip::mallocs.load(),
             fake_hip::frees.load(), fake_hip::bad_frees.load(), fake_hip::used.load());
    if (said_n) fail("pool: complained on one device: %s", said);
}

/* ---- device tags ---- */

static void check_tags(void)
{
    size_t got = 0;
    int dev = -7, dev1 = -7, dev0 = -7;
    fake_hip::device = 0;
    char *a = slab_acquire(CLASS[0], &got, &dev);
    if (!a || dev != 0) { fail("tags: a fresh slab on device 0 is tagged %d", dev); return; }
    fake_hip::device = 1;                        /* released while another device is current */
    slab_release(a, got, dev);
    if (g_state0.free.size() != 1 || g_state0.free[0].device != 0) fail("tags: the entry lost the tag of the device that allocated it");
    char *b = slab_acquire(CLASS[0], &got, &dev1);
    if (!b || b == a || dev1 != 1) fail("tags: a thread on device 1 was handed the slab of device 0 (tag %d)", dev1);
    if (said_n != 1 || !strstr(said, "device 0 met device 1")) fail("tags: the pool said \"%s\" (%u times)", said, said_n);
    fake_hip::device = 0;
    char *c = slab_acquire(CLASS[0], &got, &dev0);
    if (c != a || dev0 != 0) fail("tags: device 0 did not get its slab back (tag %d)", dev0);
    slab_release(b, CLASS[0], dev1);
    slab_release(c, CLASS[0], dev0);
    { DevLock lock(&g_state0); pool_drop_locked(&g_state0); }
    if (fake_hip::mallocs.load() != fake_hip::frees.load() || fake_hip::bad_frees.load() || fake_hip::used.load()) fail("tags: allocations and frees differ");
}

/* ---- once-guard ---- */

static DevState once_state;
static std::atomic<unsigned> builds;
struct OnceCall { int dev; bool fail_build; bool ok; char err[200]; unsigned long long entries; };

static void *once_thread(void *arg)
{
    OnceCall *c = (OnceCall *) arg;
    pthread_barrier_wait(&gate);
    c->ok = l2_once(&once_state, c->dev, [c] {
        const unsigned n = ++builds;
        usleep(50000);
        once_state.l2.entries = 1000 + n;
        if (c->fail_build) snprintf(once_state.l2_err, sizeof once_state.l2_err, "build %u failed on device %d", n, c->dev);
        return !c->fail_build;
    }, c->err, sizeof c->err);
    c->entries = once_state.l2.entries;          /* read after the guard, as staging reads the table */
    return nullptr;
}

/* eight callers at once: `more' builds run, everybody leaves with `ok' and the same text */
static void once_round(const char *what, int dev, bool fail_build, unsigned more, bool ok, const char *text)
{
    pthread_t th[THREADS];
    OnceCall call[THREADS];
    const unsigned before = builds.load();
    pthread_barrier_init(&gate, nullptr, THREADS);
    for (size_t t = 0; t < THREADS; t++) {
        call[t] = OnceCall{ dev, fail_build, false, "?", 0 };
        pthread_create(&th[t], nullptr, once_thread, &call[t]);
    }
    for (size_t t = 0; t < THREADS; t++) pthread_join(th[t], nullptr);
    pthread_barrier_destroy(&gate);
    if (builds.load() - before != more) fail("once, %s: %u builds ran, not %u", what, builds.load() - before, more);
    for (size_t t = 0; t < THREADS; t++)
        if (call[t].ok != ok || strcmp(call[t].err, text) != 0 || call[t].entries != call[0].entries)
            fail("once, %s: caller %zu left with %d \"%s\" (table of build %llu), wanted %d \"%s\"", what, t, (int) call[t].ok,
                 call[t].err, call[t].entries - 1000, (int) ok, text);
    if (once_state.l2.device != dev || once_state.l2.state != (ok ? L2_OK : L2_FAILED)) fail("once, %s: state %d on device %d", what, (int) once_state.l2.state, once_state.l2.device);
}

static void check_once(void)
{
    once_round("first use", 0, false, 1, true, "");
    once_round("built before", 0, true, 0, true, "");                    /* nobody builds: the callback's failure is never asked for */
    once_round("another device, failing", 1, true, 1, false, "build 2 failed on device 1");
    once_round("failed before", 1, false, 0, false, "build 2 failed on device 1");      /* not tried again */
    once_round("back on the first device", 0, false, 1, true, "");
}

/* ---- counters ---- */

enum { INCREMENTS = 20000 };
static void *count_thread(void *)
{
    pthread_barrier_wait(&gate);
    for (unsigned i = 0; i < INCREMENTS; i++)
        stats_update([](fiasco_amd_stats &st) { st.frames += 1; st.frames_by_build[st.frames & 1] += 1; st.kernel_ms += 0.5; });
    return nullptr;
}

static void check_counters(void)
{
    pthread_t th[THREADS];
    pthread_barrier_init(&gate, nullptr, THREADS);
    for (size_t t = 0; t < THREADS; t++) pthread_create(&th[t], nullptr, count_thread, nullptr);
    for (size_t t = 0; t < THREADS; t++) pthread_join(th[t], nullptr);
    pthread_barrier_destroy(&gate);
    DevLock lock(&g_state0);
    const fiasco_amd_stats &st = g_state0.stats;
    const unsigned long long n = (unsigned long long) THREADS * INCREMENTS;
    if (st.frames != n || st.frames_by_build[0] != n / 2 || st.frames_by_build[1] != n / 2 || st.kernel_ms != 0.5 * (double) n)
        fail("counters: %llu frames (%llu + %llu), %.1f ms after %llu increments", st.frames, st.frames_by_build[0], st.frames_by_build[1], st.kernel_ms, n);
}

int main(void)
{
    check_pool();
    check_tags();
    check_once();
    check_counters();
    if (!bad) printf("dev_state_check: ok\n");
    return bad ? 1 : 0;
}
