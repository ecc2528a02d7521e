/*
 *  frame_table.inc -- how the pixel kernels walk the frames of a launch (included by core_hip.cpp ahead of them).
 *
 *  Shape: a launch serves all frames of a share's upload or of a decoder flight.  The host fills a table with one
 *  descriptor per frame (IcFrame, IcyFrame, OcFrame, Y4Frame, Rd4Frame); the work items of all frames form ONE sequence, and a
 *  descriptor's member `first' says how many items the frames before it have -- the only member this file reads.  The grid
 *  is sized from the CU count (ft_grid), not from the work: every workgroup of FT_TILE threads takes one contiguous stretch
 *  of the sequence, tile after tile, neighbouring lanes neighbouring items.  So the frame of an item costs one binary
 *  search per workgroup, for the first item of its stretch, and a step forward now and then (ft_stretch, ft_find,
 *  ft_step).  ft_walk is that loop around a per-item function (ic_item, icy_item, oc_item, y4_item); a kernel whose threads
 *  must all stay in the loop (rd_render_kernel, rd420_render_kernel: the barriers of their doubled builds) keeps its own loop
 *  around the same three.
 */

enum { FT_TILE = 256 };         /* threads of a workgroup = items of a tile */

/* the tiles [t0, t1) of this workgroup's stretch; false: it has none */
static __device__ __forceinline__ bool ft_stretch(unsigned long long total, unsigned long long &t0, unsigned long long &t1)
{
    const unsigned long long tiles = (total + FT_TILE - 1) / FT_TILE;
    t0 = tiles * blockIdx.x / gridDim.x; t1 = tiles * (blockIdx.x + 1) / gridDim.x;
    return t0 < t1;
}

/* the frame of item `it': the last one that starts at or before it */
template <typename Frame> static __device__ __forceinline__ unsigned ft_find(const Frame *frames, unsigned nframes, unsigned long long it)
{
    unsigned lo = 0, hi = nframes;
    while (hi - lo > 1) {
        const unsigned mid = (lo + hi) / 2;
        if (frames[mid].first <= it) lo = mid; else hi = mid;
    }
    return lo;
}

/* the same for an item that is not before one of frame f: a step forward now and then */
template <typename Frame> static __device__ __forceinline__ unsigned ft_step(const Frame *frames, unsigned nframes, unsigned f, unsigned long long it)
{
    while (f + 1 < nframes && frames[f + 1].first <= it) f++;
    return f;
}

/* ITEM(F, local, extra...) for every item of this workgroup's stretch: item `local' of frame F.  ITEM is a per-item
 * function, named at compile time so that it is inlined where a kernel's own loop body would stand */
template <auto ITEM, typename Frame, typename... Extra>
static __device__ __forceinline__ void ft_walk(const Frame *__restrict__ frames, unsigned nframes, unsigned long long total, const Extra &... extra)
{
    unsigned long long t0, t1;
    if (!ft_stretch(total, t0, t1)) return;
    unsigned f = ft_find(frames, nframes, t0 * FT_TILE);
    for (unsigned long long t = t0; t < t1; t++) {
        const unsigned long long it = t * FT_TILE + threadIdx.x;
        if (it >= total) break;
        f = ft_step(frames, nframes, f, it);
        const Frame F = frames[f];
        ITEM(F, (unsigned) (it - F.first), extra...);
    }
}

/* ------------------------------------------------------------------ launching */

/* the CUs of the current device; 256 where the runtime does not say */
static int ft_cus(void)
{
    int dev = 0, ncu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu <= 0) {
        (void) hipGetLastError();
        ncu = 256;
    }
    return ncu;
}

/* the workgroups that fill a device of ncu CUs: eight of four waves per CU */
static unsigned long long ft_groups(int ncu) { return (unsigned long long) (ncu > 0 ? ncu : 256) * 8; }

/* ... fewer when the work is less */
static unsigned ft_grid(unsigned long long total, int ncu)
{
    const unsigned long long grid = ft_groups(ncu), tiles = (total + FT_TILE - 1) / FT_TILE;
    return (unsigned) (grid > tiles ? tiles : grid);
}

/* ONE launch of `kernel' for the n frames of the table at d_tab (device memory) on `stream' */
template <typename Frame, typename... Extra>
static bool ft_launch(void (*kernel)(const Frame *, unsigned, unsigned long long, Extra...), const Frame *d_tab, unsigned n, unsigned long long total,
                      int ncu, hipStream_t stream, Extra... extra)
{
    const unsigned grid = ft_grid(total, ncu);
    if (!grid || !n) return true;
    kernel<<<dim3(grid), dim3(FT_TILE), 0, stream>>>(d_tab, n, total, extra...);
    return hipGetLastError() == hipSuccess;
}

/* The tail of the entries that convert ONE frame outside a batch (fiasco_amd_planes_to_pixels_device and its siblings):
 * on `device', the filled table entry into a table of its own with a blocking copy, launch(d_tab, ncu) on the caller's
 * stream itself -- behind what it holds, before what follows --, and the table freed once the kernel has read it: the
 * call waits on the host.  1, or 0 and the message */
template <typename Launch>
static int ft_run_alone(const void *entry, size_t entry_bytes, Launch launch, int device, hipStream_t stream)
{
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    if (cur != device && hipSetDevice(device) != hipSuccess) { fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError())); return 0; }
    void *d_tab = nullptr;
    const bool ok = hipMalloc(&d_tab, entry_bytes) == hipSuccess
                    && hipMemcpy(d_tab, entry, entry_bytes, hipMemcpyHostToDevice) == hipSuccess
                    && launch(d_tab, ft_cus())
                    && hipStreamSynchronize(stream) == hipSuccess;
    if (!ok) fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
    if (d_tab) (void) hipFree(d_tab);
    if (cur >= 0 && cur != device) (void) hipSetDevice(cur);
    return ok ? 1 : 0;
}
