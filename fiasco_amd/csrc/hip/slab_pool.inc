/*
 *  slab_pool.inc -- the pool of HBM slabs of a device share (included by core_hip.cpp): DevState::free behind
 *  slab_acquire / slab_release.  A frame's slab goes back here when its batch is unstaged and is handed to the next
 *  frame of about its size; fiasco_amd_release_memory() (shares.inc) empties the pools.
 */

/* ------------------------------------------------------------------ slab pool */

/* the current device of the calling thread (the share's, bind_share); -1 when HIP cannot tell */
static int pool_device(void)
{
    int d = -1;
    if (hipGetDevice(&d) != hipSuccess) { (void) hipGetLastError(); d = -1; }
    return d;
}

static char *slab_acquire(size_t bytes, size_t *got)
{
    /* A slab never meets another device: the pool belongs to a share (t_dev), a share to a device.  An entry whose
     * tag says otherwise (a device list changed under a pool, a share bound to the wrong device) is a bug of the
     * launcher -- such an entry is not handed out, the call allocates afresh and says so. */
    const int here = pool_device();
    size_t best = g_free.size();
    for (size_t i = 0; i < g_free.size(); i++)
        if (g_free[i].device != here && g_free[i].device >= 0 && here >= 0) {
            static bool told = false;
            if (!told) { told = true; fprintf(stderr, "libfiasco_amd: slab pool entry of device %d met device %d (not used)\n", g_free[i].device, here); }
        }
    for (size_t i = 0; i < g_free.size(); i++)
        if ((g_free[i].device == here || g_free[i].device < 0 || here < 0)
            && g_free[i].bytes >= bytes && g_free[i].bytes <= bytes + bytes / 4
            && (best == g_free.size() || g_free[i].bytes < g_free[best].bytes))
            best = i;
    if (best != g_free.size()) {
        char *p = g_free[best].base;
        *got = g_free[best].bytes;
        g_free.erase(g_free.begin() + (long) best);
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
        if (g_free.empty()) return nullptr;
        for (size_t i = 0; i < g_free.size(); i++) (void) hipFree(g_free[i].base);
        g_free.clear();
        fits = hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b >= bytes + reserve;
        if (!fits || hipMalloc((void **) &p, bytes) != hipSuccess) { (void) hipGetLastError(); return nullptr; }
    }
    *got = bytes;
    return p;
}

static void slab_release(char *p, size_t bytes)
{
    if (p) g_free.push_back(PoolEntry{p, bytes, pool_device()});
}
