/*
 *  shares.inc -- the device shares of the process (included by core_hip.cpp): the device list and one DevState per
 *  share, the worker threads, the dealing rule for the encoder's and the decoder's jobs, and the seam of fa_host.h,
 *  fa_core_*(), on top of the core1_*() of one share.
 */

/* ------------------------------------------------------------------ several devices in one process
 *
 * Frames (separate fiasco_coder() calls, frames of a gray all-intra stream, the groups of pictures a
 * sequence is coded in) are independent units (SURVEY.md 8e; tiles are not: codec/tiling.c is dead code in
 * this reference).  The seam fa_core_*() therefore spreads the jobs of a batch round robin over the
 * devices of the process -- job i goes to device i mod D -- and runs every share on a host thread of its
 * own with its own stream, slab pool and log2 table (DevState); results come back in job order.  No
 * collective is involved: what crosses between devices is nothing, what comes back per frame is its
 * automaton (kilobytes) over PCIe as before.  (The reference call site this serves: video_coder()'s
 * frame loop, codec/coder.c:490-668.)
 *
 * Which devices: FIASCO_AMD_DEVICES="0,1,4" if set (an id may repeat -- two shares on one GPU: the test of
 * this path on a 1-GPU box); else, once fiasco_amd_set_device(d) has been called -- one process per GPU,
 * the multi-process harness -- just d; else every visible device.  With one device nothing below starts a
 * thread; every share of a call -- also the only one -- runs bound to its device (bind_share) and the caller's
 * current device is restored afterwards (for_each_share).
 *
 * Threading contract.  Calls on DISTINCT batch, sequence and options objects may run at the same time on any mix of
 * entries, from any number of host threads; one batch or sequence object is used by one thread at a time.  What such
 * calls share is the DevState of a share -- slab pool, counters, log2 table --, and that is locked (dev_state.h): every
 * thread of a process with one device works on g_state0, and with several shares a call whose only part lies on
 * share k runs on its calling thread beside worker k serving another caller.  A call with ONE part runs on its
 * calling thread, concurrently with everything else.  The worker threads of the shares k >= 1 belong to the process,
 * not to a batch: calls that spread over several shares are serialised by g_share_lock, one phase (stage / submit /
 * finish / upload) at a time.  The workers are detached and parked on a condition variable; they are never joined (a
 * dlclose of the library with several devices in use is not supported).
 *   Not while other calls run: fiasco_amd_set_devices(), fiasco_amd_set_device(), fiasco_amd_set_limits() and
 * fiasco_amd_release_memory().  They change what the running calls read without a lock -- the device list, and
 * g_dev_state, which bind_share() indexes while grow_dev_states() may move it -- and hand the pools' slabs back. */
static std::vector<int> g_devices;              /* empty = not resolved yet */
static int  g_device_explicit = -1;             /* fiasco_amd_set_device() */
/* [k]: the state of share k.  [0] is the one every thread works on unless bind_share() says otherwise (t_dev's
 * initial value, core_hip.cpp): there from the start, never moved, read without a lock.  The list only grows: the
 * pool of a share outlives a shorter device list. */
static std::vector<DevState *> g_dev_state(1, t_dev);
static pthread_mutex_t g_dev_lock = PTHREAD_MUTEX_INITIALIZER;

/* a state for every share of the device list (g_dev_lock held) */
static void grow_dev_states(void)
{
    while (g_dev_state.size() < g_devices.size()) g_dev_state.push_back(new DevState);
}

static void resolve_devices(void)
{
    pthread_mutex_lock(&g_dev_lock);
    if (g_devices.empty()) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess) { (void) hipGetLastError(); ndev = 0; }
        const char *e = getenv("FIASCO_AMD_DEVICES");
        if (e && *e) {
            for (const char *q = e; *q; ) {
                char *end;
                long v = strtol(q, &end, 10);
                if (end == q) break;
                if (v >= 0 && v < ndev) g_devices.push_back((int) v);
                q = *end ? end + 1 : end;
            }
        } else if (g_device_explicit >= 0) g_devices.push_back(g_device_explicit);
        else for (int d = 0; d < ndev; d++) g_devices.push_back(d);
        if (g_devices.empty()) g_devices.push_back(-1);      /* -1: whatever the current device is (or none) */
        grow_dev_states();
    }
    pthread_mutex_unlock(&g_dev_lock);
}

extern "C" int fiasco_amd_device_count(void)
{
    resolve_devices();
    return (int) g_devices.size();
}

/* the devices of this process, chosen by the caller: n ids (an id may repeat), or n = 0 for the rule above */
extern "C" int fiasco_amd_set_devices(const int *ids, int n)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) { (void) hipGetLastError(); ndev = 0; }
    for (int i = 0; i < n; i++)
        if (ids[i] < 0 || ids[i] >= ndev) { fa_set_error("libfiasco_amd: no HIP device %d", ids[i]); return 0; }
    fiasco_amd_release_memory();
    pthread_mutex_lock(&g_dev_lock);
    g_devices.clear();
    g_device_explicit = -1;
    for (int i = 0; i < n; i++) g_devices.push_back(ids[i]);
    grow_dev_states();
    pthread_mutex_unlock(&g_dev_lock);
    return 1;
}

/* one process per GPU: bind this process's coder to a device of the node */
extern "C" int fiasco_amd_set_device(int device)
{
    int cur = -1;
    /* the slab pools hold memory of the device they were allocated on: never carry them over */
    if (hipGetDevice(&cur) != hipSuccess || cur != device || g_devices.size() != 1) fiasco_amd_release_memory();
    if (hipSetDevice(device) != hipSuccess) {
        fa_set_error("libfiasco_amd: cannot select HIP device %d", device);
        return 0;
    }
    pthread_mutex_lock(&g_dev_lock);
    g_device_explicit = device;
    g_devices.clear();                              /* resolved again by the next call */
    pthread_mutex_unlock(&g_dev_lock);
    return 1;
}

extern "C" void fiasco_amd_release_memory(void)
{
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    for (size_t k = 0; k < g_dev_state.size(); k++) {
        DevState *st = g_dev_state[k];
        DevLock lock(st);
        if (st->free.empty()) continue;
        if (k < g_devices.size() && g_devices[k] >= 0 && g_devices.size() > 1) (void) hipSetDevice(g_devices[k]);
        pool_drop_locked(st);
    }
    if (have_cur && g_devices.size() > 1) (void) hipSetDevice(cur);
}

/* counters: the sum over the shares; kernel time and the largest automaton: the maximum (the shares run
 * side by side, frames / kernel_ms stays the rate of the whole job) */
extern "C" void fiasco_amd_get_stats(fiasco_amd_stats *out)
{
    memset(out, 0, sizeof *out);
    for (size_t k = 0; k < g_dev_state.size(); k++) {
        DevLock lock(g_dev_state[k]);
        const fiasco_amd_stats &b = g_dev_state[k]->stats;
        unsigned long long *o = (unsigned long long *) ((char *) out + sizeof(double));
        const unsigned long long *v = (const unsigned long long *) ((const char *) &b + sizeof(double));
        const size_t nw = (sizeof(fiasco_amd_stats) - sizeof(double)) / sizeof(unsigned long long);
        const size_t imax = (offsetof(fiasco_amd_stats, states_max) - sizeof(double)) / sizeof(unsigned long long);
        /* workgroups per frame of the table passes: a setting, the same on every share -- not a sum */
        const size_t icoop = (offsetof(fiasco_amd_stats, coop_workgroups) - sizeof(double)) / sizeof(unsigned long long);
        for (size_t i = 0; i < nw; i++) o[i] = i == imax || i == icoop ? (o[i] > v[i] ? o[i] : v[i]) : o[i] + v[i];
        if (b.kernel_ms > out->kernel_ms) out->kernel_ms = b.kernel_ms;
    }
}
extern "C" void fiasco_amd_reset_stats(void)
{
    for (size_t k = 0; k < g_dev_state.size(); k++) {
        DevLock lock(g_dev_state[k]);
        memset(&g_dev_state[k]->stats, 0, sizeof(fiasco_amd_stats));
    }
}

/* A batch over the shares.  Every part is the batch of ONE share (a Staged, enc_stage.inc) and knows the jobs it
 * works on: a DEALT part has copies `sub' of the caller's jobs idx[] -- the phases copy inputs in and results out
 * around the share's work (each_dealt_job) --, the IN-PLACE part, the only one of its batch, works on the caller's
 * jobs[] themselves and nothing is copied. */
struct MultiStaged {
    fa_job  *jobs = nullptr;          /* the caller's */
    struct Part {
        std::vector<unsigned> idx;      /* dealt: the caller's jobs of this part, in its order; in place: empty */
        std::vector<fa_job>   sub;      /* dealt: the part's copies of them */
        std::vector<char>     frames;   /* dealt: the part's frames in device memory (frames_of) */
        fa_job  *jobs = nullptr;        /* what the part's Staged works on: sub, or the caller's jobs[] */
        unsigned n = 0;
        void    *staged = nullptr;
        int      good = 0;              /* what the share's last phase returned (run_parts) */
        size_t   share = 0;             /* the device share (g_devices / g_dev_state index) this part runs on */
        /* the caller's job behind the part's job j */
        unsigned job_index(unsigned j) const { return idx.empty() ? j : idx[j]; }
        /* the part's frames out of one per job of the caller, in the part's order */
        IcInput frames_of(const IcInput &all)
        {
            if (idx.empty()) return all;
            frames.clear();
            for (size_t j = 0; j < idx.size(); j++)
                frames.insert(frames.end(), (const char *) all.at(idx[j]), (const char *) all.at(idx[j]) + all.kind->frame_bytes);
            return IcInput{ all.kind, frames.data() };
        }
    };
    std::vector<Part> parts;
    char  *up_host = nullptr;       /* several shares: the pinned buffer of fa_core_upload_buffer (the shares borrow it) */
    size_t up_host_bytes = 0;
};

/* One persistent host thread per share k >= 1 (created at its first use, parked on a condition variable between
 * calls): a phase of a batch -- stage, submit, finish, upload -- posts its share of the work there instead of
 * creating and joining a thread each time.  A worker binds itself to the device of its share, g_devices[k], at
 * the start of every task (the list may have changed since) and works on the share's DevState. */
struct ShareWorker {
    pthread_t th;
    pthread_mutex_t mu = PTHREAD_MUTEX_INITIALIZER;
    pthread_cond_t cv = PTHREAD_COND_INITIALIZER;
    void (*call)(void *, size_t) = nullptr;
    void *ctx = nullptr;
    size_t k = 0;
    int state = 0;                  /* 0 idle, 1 task posted, 2 task done */
};
static std::vector<ShareWorker *> g_workers;       /* [k], k >= 1; [0] unused */
static pthread_mutex_t g_share_lock = PTHREAD_MUTEX_INITIALIZER;    /* one multi-share phase at a time (see above) */

static void bind_share(size_t k)
{
    t_dev = g_dev_state[k];
    if (k < g_devices.size() && g_devices[k] >= 0) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess || cur != g_devices[k]) { (void) hipGetLastError(); (void) hipSetDevice(g_devices[k]); }
    }
}

static void *share_worker_main(void *p)
{
    ShareWorker *w = (ShareWorker *) p;
    for (;;) {
        pthread_mutex_lock(&w->mu);
        while (w->state != 1) pthread_cond_wait(&w->cv, &w->mu);
        pthread_mutex_unlock(&w->mu);
        bind_share(w->k);
        w->call(w->ctx, w->k);                 /* ctx names the part of the batch (for_shares) */
        pthread_mutex_lock(&w->mu);
        w->state = 2;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
    }
    return nullptr;
}

static ShareWorker *share_worker(size_t k)
{
    pthread_mutex_lock(&g_dev_lock);
    while (g_workers.size() <= k) g_workers.push_back(nullptr);
    ShareWorker *w = g_workers[k];
    if (!w) {
        w = new ShareWorker;
        w->k = k;
        if (pthread_create(&w->th, nullptr, share_worker_main, w) != 0) { delete w; w = nullptr; }
        else { (void) pthread_detach(w->th); g_workers[k] = w; }
    }
    pthread_mutex_unlock(&g_dev_lock);
    return w;
}

/* run fn(share) for every share: share 0 on the calling thread, the others on their workers; EVERY share --
 * also the only one of a call -- runs bound to its device g_devices[k] with the DevState of that share (the slab
 * pool of a share never sees another device), and the caller's current device is what it was afterwards */
template <typename Fn> static void for_shares(const std::vector<size_t> &share, Fn fn)
{
    const size_t D = share.size();
    int cur = -1;
    const bool have_cur = hipGetDevice(&cur) == hipSuccess;
    if (!have_cur) (void) hipGetLastError();
    /* the workers' call / ctx / state slots are per process: two host threads driving two multi-share batches
     * would overwrite each other's task (a lost task, or a wait for `state == 2' that never ends) */
    if (D > 1) pthread_mutex_lock(&g_share_lock);
    struct Task { Fn *fn; size_t part; };
    std::vector<Task> task(D);
    auto tramp = [](void *p, size_t) { Task *t = (Task *) p; (*t->fn)(t->part); };
    std::vector<ShareWorker *> posted(D, nullptr);
    for (size_t k = 1; k < D; k++) {
        /* part k on the worker of ITS share; two parts of one share (never dealt that way) would run one after the other */
        bool dup = false;
        for (size_t j = 0; j < k; j++) dup = dup || share[j] == share[k];
        ShareWorker *w = dup ? nullptr : share_worker(share[k]);
        if (!w) continue;
        task[k].fn = &fn; task[k].part = k;
        pthread_mutex_lock(&w->mu);
        w->call = tramp; w->ctx = &task[k]; w->state = 1;
        pthread_cond_broadcast(&w->cv);
        pthread_mutex_unlock(&w->mu);
        posted[k] = w;
    }
    if (D) { bind_share(share[0]); fn(0); }
    for (size_t k = 1; k < D; k++) {
        if (posted[k]) {
            ShareWorker *w = posted[k];
            pthread_mutex_lock(&w->mu);
            while (w->state != 2) pthread_cond_wait(&w->cv, &w->mu);
            w->state = 0;
            pthread_mutex_unlock(&w->mu);
        } else { bind_share(share[k]); fn(k); }      /* no thread: one after the other */
    }
    if (D > 1) pthread_mutex_unlock(&g_share_lock);
    t_dev = g_dev_state[0];
    if (have_cur) {
        int now = -1;
        if (hipGetDevice(&now) != hipSuccess || now != cur) { (void) hipGetLastError(); (void) hipSetDevice(cur); }
    }
}

/* fn(part) for every part of a staged batch, each on the share it was dealt to */
template <typename Fn> static void for_each_share(MultiStaged *M, Fn fn)
{
    std::vector<size_t> share(M->parts.size());
    for (size_t k = 0; k < share.size(); k++) share[k] = M->parts[k].share;
    for_shares(share, fn);
}

/* The dealing rule: how many shares the n jobs of a call are dealt over -- fa_share_of() (fa_host.h) then says which
 * share takes job i.  Jobs without a key go round robin by their index (SURVEY 8e) and spread over no more shares than
 * there are jobs.  Jobs with a key (the GOP of a video): the share is a function of the key and of the number of
 * devices ALONE, not of how many jobs this call happens to hold; a share without a job gets nothing to do.  The search
 * (fa_job) and the decoder (fa_dec_job) both deal by this, so a frame is decoded where it is searched. */
template <typename Job> static size_t share_count(unsigned n, const Job *jobs)
{
    resolve_devices();
    const size_t D = g_devices.size();
    bool keyed = false;
    for (unsigned i = 0; i < n; i++) keyed = keyed || jobs[i].share_key != 0;
    return !keyed && D > n ? (n ? n : 1) : D;
}

/* fn(the part's copy, the caller's job) for every job of every dealt part: how a phase brings the copies up to date
 * before the shares work and the caller's jobs afterwards.  The in-place part has no copies: nothing happens. */
template <typename Fn> static void each_dealt_job(MultiStaged *M, Fn fn)
{
    for (size_t k = 0; k < M->parts.size(); k++)
        for (size_t j = 0; j < M->parts[k].sub.size(); j++) fn(M->parts[k].sub[j], M->jobs[M->parts[k].idx[j]]);
}

/* one phase of a batch: fn(the share's batch) for every part on its share.  Returns the sum of what the parts returned:
 * good frames (core1_finish2), or -- of the phases that answer 0 or 1 -- how many parts succeeded. */
template <typename Fn> static int run_parts(MultiStaged *M, Fn fn)
{
    int sum = 0;
    for_each_share(M, [&](size_t k) { M->parts[k].good = fn(M->parts[k].staged); });
    for (size_t k = 0; k < M->parts.size(); k++) sum += M->parts[k].good;
    return sum;
}

static void *stage_shares(unsigned n, fa_job *jobs, const IcInput *frames, hipEvent_t ready)
{
    MultiStaged *M = new MultiStaged;
    M->jobs = jobs;
    const size_t D = share_count(n, jobs);
    M->parts.resize(D);
    for (size_t k = 0; k < D; k++) M->parts[k].share = k;
    for (unsigned i = 0; i < n; i++) M->parts[fa_share_of(jobs[i].share_key, i, (unsigned) D)].idx.push_back(i);
    M->parts.erase(std::remove_if(M->parts.begin(), M->parts.end(), [](const MultiStaged::Part &P) { return P.idx.empty(); }),
                   M->parts.end());                  /* a share without a job gets no part */
    if (M->parts.size() <= 1) {
        /* every job on one share (one device; the last GOPs of a video) or no job at all (share 0): in place */
        M->parts.resize(1);
        M->parts[0].idx.clear();
        M->parts[0].jobs = jobs; M->parts[0].n = n;
    } else
        for (MultiStaged::Part &P : M->parts) {
            for (size_t j = 0; j < P.idx.size(); j++) P.sub.push_back(jobs[P.idx[j]]);
            P.jobs = P.sub.data(); P.n = (unsigned) P.sub.size();
        }
    for_each_share(M, [&](size_t k) {
        MultiStaged::Part &P = M->parts[k];
        const IcInput mine = frames ? P.frames_of(*frames) : IcInput{ nullptr, nullptr };
        P.staged = core1_stage(P.n, P.jobs, frames ? &mine : nullptr, ready);      /* every share converts its own frames */
    });
    each_dealt_job(M, [](const fa_job &mine, fa_job &callers) { callers = mine; });   /* what staging said about a job */
    return M;
}

extern "C" void *fa_core_stage(unsigned n, fa_job *jobs) { return stage_shares(n, jobs, nullptr, nullptr); }

extern "C" void fa_core_unstage(void *h)
{
    MultiStaged *M = (MultiStaged *) h;
    if (!M) return;
    for_each_share(M, [&](size_t k) { core1_unstage(M->parts[k].staged); });
    if (M->up_host) (void) hipHostFree(M->up_host);
    delete M;
}

extern "C" int fa_core_submit(void *h)
{
    MultiStaged *M = (MultiStaged *) h;
    if (!M) return 0;
    each_dealt_job(M, [](fa_job &dst, const fa_job &src) {                      /* inputs as the caller has them now */
        dst.image = src.image; dst.frame_type = src.frame_type; dst.past = src.past; dst.future = src.future;
        dst.cp = src.cp; dst.wfa = src.wfa; dst.ycol_carry = src.ycol_carry;
    });
    return run_parts(M, core1_submit) == (int) M->parts.size();                 /* every share started its pass */
}

/* the number of good frames of all shares */
extern "C" int fa_core_finish2(void *h, int resubmit)
{
    MultiStaged *M = (MultiStaged *) h;
    if (!M) return 0;
    const int good = run_parts(M, [&](void *staged) { return core1_finish2(staged, resubmit); });
    each_dealt_job(M, [](const fa_job &mine, fa_job &callers) { callers = mine; });
    return good;
}

extern "C" int fa_core_finish(void *h) { return fa_core_finish2(h, 0); }

extern "C" int fa_core_run(void *h)
{
    if (!fa_core_submit(h)) return 0;
    return fa_core_finish(h);
}

/* replacement inputs for a staged batch (a stream of batches over PCIe).  The caller fills ONE pinned buffer with
 * the planes of all frames; every share then copies the planes of ITS frames to its device (core1_upload_commit).
 * With several shares the buffer belongs to the batch (portable pinned memory: every device reads it). */
extern "C" int16_t *fa_core_upload_buffer(void *h, size_t bytes)
{
    MultiStaged *M = (MultiStaged *) h;
    if (!M) return nullptr;
    if (M->parts.size() == 1) {
        int16_t *r = nullptr;
        for_each_share(M, [&](size_t) { r = core1_upload_buffer(M->parts[0].staged, bytes); });
        return r;
    }
    /* the previous uploads have left the buffer long ago (a whole pass lies in between); make sure */
    for_each_share(M, [&](size_t k) { Staged *S = (Staged *) M->parts[k].staged; if (S && S->ustream) (void) hipStreamSynchronize(S->ustream); });
    if (bytes > M->up_host_bytes) {
        if (M->up_host) (void) hipHostFree(M->up_host);
        M->up_host = nullptr; M->up_host_bytes = 0;
        if (hipHostMalloc((void **) &M->up_host, bytes, hipHostMallocPortable) != hipSuccess) {
            M->up_host = nullptr; (void) hipGetLastError();
            /* the shares still point into the buffer that was just freed: a later commit must not bounds-check
             * against it or copy from it */
            for (size_t k = 0; k < M->parts.size(); k++) {
                Staged *S = (Staged *) M->parts[k].staged;
                if (S && S->up_host_shared) { S->up_host = nullptr; S->up_host_bytes = 0; S->up_host_shared = false; }
            }
            return nullptr;
        }
        M->up_host_bytes = bytes;
    }
    for (size_t k = 0; k < M->parts.size(); k++) {
        Staged *S = (Staged *) M->parts[k].staged;
        if (!S || !S->ok) return nullptr;
        if (S->up_host && !S->up_host_shared) (void) hipHostFree(S->up_host);
        S->up_host = M->up_host; S->up_host_bytes = M->up_host_bytes; S->up_host_shared = true;
    }
    return (int16_t *) M->up_host;
}

extern "C" int fa_core_upload_commit(void *h)
{
    MultiStaged *M = (MultiStaged *) h;
    if (!M) return 0;
    each_dealt_job(M, [](fa_job &mine, const fa_job &callers) { mine.image = callers.image; });   /* the new images of the caller's jobs */
    return run_parts(M, core1_upload_commit) == (int) M->parts.size();
}

extern "C" int fa_core_encode_frames(unsigned n, fa_job *jobs)
{
    void *h = fa_core_stage(n, jobs);
    int good = fa_core_run(h);
    fa_core_unstage(h);
    return good;
}

/* The decoder's side of the dealing rule (share_count).  A job is decoded on the device share the SEARCH deals it to, so
 * that the reference frame of a GOP is decoded where the next frame of that GOP is searched and stays in that device's
 * HBM (fa_image.dev).  decode_frames() deals by dec_shares and dec_share_of; the batch entry points ask them where a
 * frame will be decoded before they accept a target or an original that lives on a device. */
static size_t dec_shares(unsigned n, const fa_dec_job *jobs) { return share_count(n, jobs); }

static size_t dec_share_of(const fa_dec_job *jobs, unsigned i, size_t shares) { return fa_share_of(jobs[i].share_key, i, (unsigned) shares); }

/* cur: the calling thread's device, which a share without a device of its own (g_devices: -1) decodes on */
static int dec_device_of(const fa_dec_job *jobs, unsigned i, size_t shares, int cur)
{
    const int dev = g_devices[dec_share_of(jobs, i, shares)];
    return dev >= 0 ? dev : cur;
}

/* the dealing function of the device shares (fa_host.h), for the tests: job -> share is a function of the key alone */
extern "C" unsigned fiasco_amd_share_of(unsigned share_key, unsigned index, unsigned shares) { return fa_share_of(share_key, index, shares); }
extern "C" const char *fa_core_name(void) { return "hip-gfx950"; }
