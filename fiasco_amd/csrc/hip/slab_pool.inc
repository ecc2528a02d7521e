/*
 *  slab_pool.inc -- the pool of HBM slabs of a device share (included by core_hip.cpp): DevState::free behind
 *  slab_acquire / slab_release.  A frame's slab goes back here when its batch is unstaged and is handed to the next
 *  frame of about its size; fiasco_amd_release_memory() (shares.inc, pool_drop) empties the pools.
 *
 *  Several host threads stage and unstage on one share at the same time (dev_state.h): everything below works on the
 *  pool under the share's lock, the allocations and frees included -- a slab is in the pool or with ONE holder.  Host
 *  code over hipGetDevice, hipMalloc, hipFree, hipMemGetInfo and hipGetLastError only: tests/dev_state_check.cpp
 *  includes this file over a fake of the five.
 */

/* ------------------------------------------------------------------ slab pool */

/* the current device of the calling thread (the share's, bind_share); -1 when HIP cannot tell */
static int pool_device(void)
{
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) { (void) hipGetLastError(); d = -1; }
    return d;
}

/* the pool's slabs back to the device, all of them (the share's lock held; the current device is the share's) */
static void pool_drop_locked(DevState *st)
{
    for (size_t i = 0; i < st->free.size(); i++) (void) hipFree(st->free[i].base);
    st->free.clear();
}

/* a slab of at least `bytes': *got is its size, *device where hipMalloc gave it out (-1: unknown) -- both go back
 * with it (slab_release) */
static char *slab_acquire(size_t bytes, size_t *got, int *device)
{
    /* A slab never meets another device: the pool belongs to a share (t_dev), a share to a device.  An entry whose
     * tag says otherwise (a device list changed under a pool, a share bound to the wrong device) is a bug of the
     * launcher -- such an entry is not handed out, the call allocates afresh and says so. */
    const int here = pool_device();
    DevLock lock(t_dev);
    std::vector<PoolEntry> &pool = t_dev->free;
    size_t best = pool.size();
    for (size_t i = 0; i < pool.size(); i++)
        if (pool[i].device != here && pool[i].device >= 0 && here >= 0) {
            static std::atomic<bool> told(false);
            if (!told.exchange(true)) fprintf(stderr, "libfiasco_amd: slab pool entry of device %d met device %d (not used)\n", pool[i].device, here);
        }
    for (size_t i = 0; i < pool.size(); i++)
        if ((pool[i].device == here || pool[i].device < 0 || here < 0)
            && pool[i].bytes >= bytes && pool[i].bytes <= bytes + bytes / 4
            && (best == pool.size() || pool[i].bytes < pool[best].bytes))
            best = i;
    if (best != pool.size()) {
        char *p = pool[best].base;
        *got = pool[best].bytes;
        *device = pool[best].device;
        pool.erase(pool.begin() + (long) best);
        return p;
    }
    char *p = nullptr;
    size_t free_b = 0, total_b = 0;
    /* leave a reserve for the launch's own buffers (descriptors, packed automata, uploads) */
    const size_t reserve = (size_t) 768 << 20;
    bool fits = hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b >= bytes + reserve;
    if (!fits || hipMalloc((void **) &p, bytes) != hipSuccess) {
        /* pool may be holding slabs of other sizes: drop them and try once more */
        (void) hipGetLastError();
        if (pool.empty()) return nullptr;
        pool_drop_locked(t_dev);
        fits = hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b >= bytes + reserve;
        if (!fits || hipMalloc((void **) &p, bytes) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
    }
    *got = bytes;
    *device = here;
    return p;
}

/* back into the pool, under the tag of the device that allocated it -- not of whichever device is current now */
static void slab_release(char *p, size_t bytes, int device)
{
    if (!p) return;
    DevLock lock(t_dev);
    t_dev->free.push_back(PoolEntry{p, bytes, device});
}

/* bytes the pool of the calling thread's share holds */
static size_t pool_bytes(void)
{
    DevLock lock(t_dev);
    size_t sum = 0;
    for (size_t i = 0; i < t_dev->free.size(); i++) sum += t_dev->free[i].bytes;
    return sum;
}
