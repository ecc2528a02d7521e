/*
 *  smooth.inc -- decoded frames smoothed along the borders of their partition, in device memory (included by
 *  core_hip.cpp between distortion.inc, whose batch path its second entry point uses, and frame_decoder.inc, whose
 *  flights launch it between the decoder's kernels and their consumers).
 *
 *  `dfiasco' shows no frame the way `-s 0' decodes it: it blends the luminance plane along every border between the two
 *  halves of a block of the partition (smooth_image, reference codec/decoder.c:674-768), with the percentage of the
 *  stream header or of `-s N'.  fa_smoothing_borders() (host/fa_batch_decode.c) lists those borders in passes -- Y by
 *  ascending level, then Cb by ascending level -- such that the borders of one pass share no pixel; pass after pass
 *  that is the reference's sequential result.  Here ONE launch of sm_pass_kernel per pass index blends that pass in
 *  every frame of a decoder flight (blockIdx.y = frame; a frame with fewer passes returns); stream order separates the
 *  passes.  A plane small enough that those launches, not its bytes, are its cost (sm_fused) takes sm_frame_kernel
 *  instead: ONE launch in which one workgroup runs all passes of the plane, a barrier between two passes.  Magnified
 *  frames and thumbnails are smoothed along fa_smoothing_borders_magnified()'s list against their own size.
 *
 *  Arithmetic (tests/smooth_ref.py restates it in numpy): a pixel pair (a, b) across a border becomes
 *    a' = (((is * a) >> 10) << 1) + (((inegs * b) >> 10) << 1),  b' = the mirror image
 *  in int with arithmetic shifts, stored as int16 with wrap-around.  |is * a| < 2^25; the doubling is written `* 2':
 *  the same value, and defined for a negative operand where `<< 1' is not before C++20.  is and inegs come from the
 *  percentage N with the reference's types: s = 1 - N / 200 as a float, the products in float, + .5 in double,
 *  truncated; N = 70 gives 333 and 179.  s < 0.5 or s >= 1 (N = 0, N > 100): the reference smooths nothing and no
 *  kernel is launched.  Only the Y plane is touched.
 *
 *  Geometry: a border of an odd level is horizontal -- rows y - 1 and y, `len' columns from x --, one of an even level
 *  vertical -- columns x - 1 and x, `len' rows from y.  All borders of a pass have one level, so their unclipped length
 *  `side' is one power of two: item i of a pass is border i >> log2(side), pair i & (side - 1), idle when that is
 *  >= len (a border clipped at the frame).  No prefix sums.
 *
 *  What a wave reads and writes (one 16-bit load and one 16-bit store per pixel, global address space):
 *    horizontal, side >= 64   64 neighbouring pairs of one border: 128 contiguous bytes of row y - 1 and 128 of row y,
 *                             read and written back: two cache lines per instruction where the row is aligned
 *    horizontal, side < 64    64 / side borders, from each side * 2 contiguous bytes of its two rows
 *    vertical                 lane k touches the two neighbouring pixels (x - 1, x) of row y + k: 4 bytes in each of 64
 *                             rows, width * 2 bytes apart -- one cache line per lane.  Accepted: the kernel is bound by
 *                             its launches (about a dozen microseconds per pass of a flight), not by these bytes
 *
 *  Tables, per frame: its borders (8 bytes each, fiasco_amd_border) and npasses + 1 offsets into them, back to back in
 *  sm_table_bytes() bytes; a descriptor SmDesc per frame that is still alive when the step runs holds the Y plane, its
 *  size, the two tables and the factors.  All of it lies in the flight's arena, carved by dec_flight_prepare from the
 *  counts that sm_check() returned and sm_pack() packs -- sm_pack() refuses a block of another size.
 *
 *  sm_factors(), sm_check(), sm_table_bytes(), sm_pack(), sm_pass_items(), sm_describe(), sm_fused(), the per-item function
 *  sm_item() and the fused kernel's body between two barriers, sm_frame_step(), are plain C++: with SMOOTH_HOST_REPLAY
 *  defined this file compiles without HIP and holds nothing else (tests/smooth_step_check.cpp and
 *  tests/shown_step_check.cpp replay flights on the CPU under the sanitizers).
 */

#ifdef SMOOTH_HOST_REPLAY
#define PX_HOST_REPLAY 1
#define SM_BOTH static inline
#else
#define SM_BOTH static __host__ __device__ __forceinline__
#endif
#include "px_access.inc"

enum { SM_MAX_LEVEL = 32 };          /* side 2^16: beyond what the 16-bit coordinates of a border can reach */

/* one frame of a launch: blockIdx.y */
struct SmDesc {
    int16_t                 *plane;      /* Y [H][W] */
    const fiasco_amd_border *borders;    /* [first[npasses]] in pass order */
    const unsigned          *first;      /* [npasses + 1]: the borders of pass p are first[p] .. first[p + 1] - 1 */
    unsigned                 W, H, npasses;
    int                      is, inegs;
};

/* log2 of the unclipped length of a border of `level': width_of_level for a horizontal one, height_of_level else */
SM_BOTH unsigned sm_log2_side(unsigned level) { return level & 1 ? level >> 1 : (level + 1) >> 1; }

/* item i of pass `pass' of the frame d: one pixel pair, or nothing */
PX_DEV void sm_item(const SmDesc &d, unsigned pass, unsigned long long i)
{
    if (pass >= d.npasses) return;
    const PX_GLOBAL unsigned *first = (const PX_GLOBAL unsigned *) d.first;
    const PX_GLOBAL fiasco_amd_border *bd = (const PX_GLOBAL fiasco_amd_border *) d.borders;
    const unsigned b0 = first[pass], nb = first[pass + 1] - b0;
    if (!nb) return;
    const unsigned level = bd[b0].level, lg = sm_log2_side(level);
    if (i >= ((unsigned long long) nb << lg)) return;
    const unsigned k = b0 + (unsigned) (i >> lg), pair = (unsigned) (i & ((1ull << lg) - 1));
    if (pair >= bd[k].len) return;                              /* clipped at the frame */
    const size_t W = d.W, x = bd[k].x, y = bd[k].y;
    size_t ia, ib;
    if (level & 1) { ia = (y - 1) * W + x + pair; ib = ia + W; }
    else           { ia = (y + pair) * W + x - 1; ib = ia + 1; }
    PX_GLOBAL int16_t *p = (PX_GLOBAL int16_t *) d.plane;
    const int a = p[ia], b = p[ib], is = d.is, inegs = d.inegs;
    p[ia] = (int16_t) (((is * a) >> 10) * 2 + ((inegs * b) >> 10) * 2);
    p[ib] = (int16_t) (((is * b) >> 10) * 2 + ((inegs * a) >> 10) * 2);
}

/* the items of pass `pass' of the frame d, read where the kernel reads them: borders << log2(side); 0 beyond the last pass */
PX_DEV unsigned long long sm_items(const SmDesc &d, unsigned pass)
{
    if (pass >= d.npasses) return 0;
    const PX_GLOBAL unsigned *first = (const PX_GLOBAL unsigned *) d.first;
    const PX_GLOBAL fiasco_amd_border *bd = (const PX_GLOBAL fiasco_amd_border *) d.borders;
    const unsigned b0 = first[pass], nb = first[pass + 1] - b0;
    return nb ? (unsigned long long) nb << sm_log2_side(bd[b0].level) : 0ull;
}

/* The body of sm_frame_kernel between two barriers: what thread t of nt does in pass `pass' of the plane its workgroup
 * owns -- the items t, t + nt, ... of that pass, each through sm_item().  The items of a pass touch disjoint pixels, so
 * their order within the pass is free; the barrier between two passes is the caller's (the kernel: __syncthreads(); a
 * replay on the CPU: finishing every t of a pass before the next pass begins). */
PX_DEV void sm_frame_step(const SmDesc &d, unsigned pass, unsigned t, unsigned nt)
{
    const unsigned long long n = sm_items(d, pass);
    for (unsigned long long i = t; i < n; i += nt) sm_item(d, pass, i);
}

/* Which smoothed planes take the fused kernel (sm_frame_kernel: ONE launch, one workgroup per plane, all passes) and
 * which the per-pass launches that the planes of a flight share: a pure function of the counts sm_check() returns.
 * One workgroup blends at most 1024 pairs at a time where the per-pass launches spread a pass over the chip, so the
 * fused kernel wins where launches dominate: small planes.  SM_FUSED_MAX_PAIRS is the largest measured size at which a
 * fused flight of 32 planes was faster by more than the spread of the measurement: 240 x 136, a 1080p frame at -3, by
 * 12 us of 981; at 25 368 pairs (512 x 384) it lost by 5 us (profiles/shown_device.json, DESIGN.md 3).
 * A plane without passes has no launch of either kind. */
static const unsigned long long SM_FUSED_MAX_PAIRS = 17270ull;
static inline bool sm_fused(unsigned long long pairs, unsigned npasses) { return npasses >= 1 && pairs <= SM_FUSED_MAX_PAIRS; }

/* the factors of a smoothing percentage; false: the reference smooths nothing (s < 0.5 || s >= 1) */
static bool sm_factors(int percent, int *is, int *inegs)
{
    const float s = (float) (1.0 - percent / 200.0);
    if (s < 0.5f || s >= 1) return false;
    *is = (int) ((double) (s * 512) + .5);
    *inegs = (int) ((double) ((1 - s) * 512) + .5);
    return true;
}

/* A border list against a plane of W x H, before anything is packed or uploaded: every border inside the plane (odd
 * level: 1 <= y < H, x + len <= W; even level: 1 <= x < W, y + len <= H), len >= 1 and no longer than the level's side,
 * passes ascending from 0 without gaps, one level per pass.  *npasses; *pairs: the pixel pairs of all borders.
 * false + msg: the list is refused */
static bool sm_check(const fiasco_amd_border *borders, unsigned n, unsigned W, unsigned H, unsigned *npasses, unsigned long long *pairs,
                     char *msg, size_t msg_n)
{
    unsigned np = 0, level = 0;
    unsigned long long sum = 0;
    for (unsigned k = 0; k < n; k++) {
        const fiasco_amd_border &b = borders[k];
        const char *bad = nullptr;
        if (b.pass == np) { np++; level = b.level; }            /* the first border of the next pass (pass is 8 bits: np <= 256) */
        else if (!np || b.pass != np - 1) bad = "the passes do not ascend from 0 without gaps";
        if (!bad && b.level != level) bad = "two levels in one pass";
        if (!bad && b.level > SM_MAX_LEVEL) bad = "level out of range";
        if (!bad && (b.len < 1 || b.len > (1u << sm_log2_side(b.level)))) bad = "length out of range for its level";
        if (!bad && (b.level & 1 ? !(b.y >= 1 && b.y < H && (unsigned) b.x + b.len <= W)
                                 : !(b.x >= 1 && b.x < W && (unsigned) b.y + b.len <= H))) bad = "outside the plane";
        if (bad) {
            snprintf(msg, msg_n, "smoothing border %u (x %u, y %u, len %u, level %u, pass %u) of a plane of %u x %u: %s", k,
                     (unsigned) b.x, (unsigned) b.y, (unsigned) b.len, (unsigned) b.level, (unsigned) b.pass, W, H, bad);
            return false;
        }
        sum += b.len;
    }
    *npasses = np; *pairs = sum;
    return true;
}

/* the tables of a frame with n borders in npasses passes: the borders, then npasses + 1 offsets */
static size_t sm_table_bytes(unsigned n, unsigned npasses) { return (size_t) n * sizeof(fiasco_amd_border) + ((size_t) npasses + 1) * sizeof(unsigned); }

/* a checked list into `block' of block_bytes bytes; false: the block was sized from other counts */
static bool sm_pack(const fiasco_amd_border *borders, unsigned n, unsigned npasses, char *block, size_t block_bytes)
{
    if (block_bytes != sm_table_bytes(n, npasses)) return false;
    if (n) memcpy(block, borders, (size_t) n * sizeof(fiasco_amd_border));
    unsigned *first = (unsigned *) (block + (size_t) n * sizeof(fiasco_amd_border));
    unsigned p = 0;
    for (unsigned k = 0; k < n; k++)
        while (p <= borders[k].pass) {
            if (p >= npasses) return false;
            first[p++] = k;
        }
    if (p != npasses) return false;
    first[npasses] = n;
    return true;
}

/* the items of pass `pass' of a packed block (host memory): borders << log2(side); 0 beyond the last pass */
static unsigned long long sm_pass_items(const char *block, unsigned n, unsigned npasses, unsigned pass)
{
    if (pass >= npasses) return 0;
    const fiasco_amd_border *bd = (const fiasco_amd_border *) block;
    const unsigned *first = (const unsigned *) (block + (size_t) n * sizeof(fiasco_amd_border));
    return (unsigned long long) (first[pass + 1] - first[pass]) << sm_log2_side(bd[first[pass]].level);
}

/* the descriptor of a frame whose packed block lies at `tables' (where the kernel reads it) */
static void sm_describe(SmDesc &d, int16_t *plane, unsigned W, unsigned H, const char *tables, unsigned n, unsigned npasses, int is, int inegs)
{
    d.plane = plane; d.borders = (const fiasco_amd_border *) tables;
    d.first = (const unsigned *) (tables + (size_t) n * sizeof(fiasco_amd_border));
    d.W = W; d.H = H; d.npasses = npasses; d.is = is; d.inegs = inegs;
}

#ifndef SMOOTH_HOST_REPLAY

__global__ void __launch_bounds__(256) sm_pass_kernel(const SmDesc *__restrict__ descs, unsigned pass)
{
    const SmDesc d = descs[blockIdx.y];
    sm_item(d, pass, (unsigned long long) blockIdx.x * 256 + threadIdx.x);
}

/* pass `pass' of the nframes frames of the table at d_descs (device memory); most: the items of the frame that has most */
static bool sm_launch(const SmDesc *d_descs, unsigned nframes, unsigned pass, unsigned long long most, hipStream_t stream)
{
    if (!most || !nframes) return true;
    sm_pass_kernel<<<dim3((unsigned) ((most + 255) / 256), nframes), dim3(256), 0, stream>>>(d_descs, pass);
    return hipGetLastError() == hipSuccess;
}

/* All passes of a plane in ONE launch: blockIdx.x selects a descriptor, and the one workgroup that gets it owns that
 * plane for the whole launch.  Pass after pass its threads stride the items of the pass (sm_frame_step -> sm_item, the
 * per-item function of sm_pass_kernel) and meet at a barrier: what a pass reads was written by the kernels before this
 * one on the stream or by waves of THIS workgroup before the barrier -- same CU, same L1; nothing another CU wrote during
 * the launch is read, so there is no hand-off between workgroups.  Plain 16-bit loads and stores.  npasses is one
 * value per block (the descriptor is read by every thread from the same address): every thread reaches every barrier.
 * hipcc, gfx950: 16 VGPRs, 38 SGPRs, no LDS, no scratch (-Rpass-analysis=kernel-resource-usage). */
__global__ void __launch_bounds__(1024) sm_frame_kernel(const SmDesc *__restrict__ descs)
{
    const SmDesc d = descs[blockIdx.x];
    for (unsigned pass = 0; pass < d.npasses; pass++) {
        sm_frame_step(d, pass, threadIdx.x, blockDim.x);
        __syncthreads();
    }
}

/* the nplanes planes of the table at d_descs (device memory), each by a workgroup of its own; most: the items of the
 * largest pass among them, which sizes the workgroups (64 .. 1024 threads, whole waves) */
static bool sm_launch_fused(const SmDesc *d_descs, unsigned nplanes, unsigned long long most, hipStream_t stream)
{
    if (!most || !nplanes) return true;
    const unsigned threads = most >= 1024 ? 1024u : (unsigned) ((most + 63) / 64 * 64);
    sm_frame_kernel<<<dim3(nplanes), dim3(threads), 0, stream>>>(d_descs);
    return hipGetLastError() == hipSuccess;
}

/* sm_fused(), or what the developer switch FIASCO_AMD_SMOOTH_FUSED says in its place (1: every smoothed plane through
 * the fused kernel, 0: none; honoured with FIASCO_AMD_DEBUG only): the tests run both paths on the same frames */
static bool sm_takes_fused(unsigned long long pairs, unsigned npasses)
{
    const long long forced = knob_int("FIASCO_AMD_SMOOTH_FUSED", -1);
    return forced == 0 ? false : forced == 1 ? npasses >= 1 : sm_fused(pairs, npasses);
}

extern "C" int fiasco_amd_smooth_fused(unsigned long long pairs, unsigned npasses) { return sm_fused(pairs, npasses) ? 1 : 0; }

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_smooth.h) */

static const char *sm_refuse(int smoothing)
{
    return smoothing < -1 || smoothing > 100 ? "smoothing out of range (-1: the value of the frame's header, 0: none, 1 .. 100 per cent)" : nullptr;
}

/* the jobs of a checked batch call at `smoothing'; -1: every frame at the value its own stream header carries (what
 * `dfiasco' does when no -s is given); a header value above 100 smooths nothing, as in the reference */
static void sm_batch_jobs(const fiasco_amd_batch_t *b, OcBatch &B, int smoothing)
{
    for (unsigned i = 0; i < b->n; i++) {
        if (B.jobs[i].skip) continue;
        const unsigned header = b->infos[i].smoothing;
        B.jobs[i].smoothing = smoothing >= 0 ? smoothing : header > 100 ? 0 : (int) header;
    }
}

extern "C" int fiasco_amd_batch_decode_device_smoothed(const fiasco_amd_batch_t *b, int smoothing, const fiasco_amd_device_target *targets, void *stream)
{
    OcBatch B;
    const char *who = "fiasco_amd_batch_decode_device_smoothed";
    if (!oc_batch_jobs(who, targets ? sm_refuse(smoothing) : "no targets", b, targets, B)) return 0;
    sm_batch_jobs(b, B, smoothing);
    return oc_decode_batch(who, b, B, 0, stream);
}

extern "C" int fiasco_amd_batch_decode_distortion_device_smoothed(const fiasco_amd_batch_t *b, int smoothing, unsigned long long *sse, unsigned *maxdiff,
                                                                  const fiasco_amd_device_target *targets, void *stream)
{
    OcBatch B;
    const char *who = "fiasco_amd_batch_decode_distortion_device_smoothed";
    if (!oc_batch_jobs(who, sse || maxdiff || targets ? sm_refuse(smoothing) : "no result arrays and no targets", b, targets, B)) return 0;
    sm_batch_jobs(b, B, smoothing);
    return ds_decode_batch(who, b, B, sse, maxdiff, targets, stream);
}

/* include/libfiasco_amd_display.h: the magnified entry and the thumbnail entry with the jobs' smoothing set -- the
 * decoder's flights do the rest (dec_smooth_prepare, frame_decoder.inc) */
extern "C" int fiasco_amd_batch_decode_device_shown(const fiasco_amd_batch_t *b, int magnify, int smoothing, const fiasco_amd_device_target *targets, void *stream)
{
    OcBatch B;
    const char *who = "fiasco_amd_batch_decode_device_shown";
    if (!oc_batch_jobs(who, targets ? sm_refuse(smoothing) : "no targets", b, targets, B, magnify)) return 0;
    sm_batch_jobs(b, B, smoothing);
    return oc_decode_batch(who, b, B, 0, stream);
}

extern "C" int fiasco_amd_batch_decode_device_thumbnails_shown(const fiasco_amd_batch_t *b, int smoothing, const fiasco_amd_device_target *targets, unsigned reduce,
                                                               const fiasco_amd_device_target *thumbs, void *stream)
{
    OcBatch B;
    const char *who = "fiasco_amd_batch_decode_device_thumbnails_shown";
    const char *refuse = !thumbs ? "no thumbnails" : !reduce ? "a reduction of at least 1 (half the side length) is needed" : reduce > 15 ? "reduction out of range"
                         : sm_refuse(smoothing);
    if (!oc_batch_jobs(who, refuse, b, targets, B, 0, thumbs, reduce)) return 0;
    sm_batch_jobs(b, B, smoothing);
    return oc_decode_batch(who, b, B, reduce, stream);
}

/* the step alone (fiasco_amd_smooth_planes_device, fiasco_amd_smooth_planes_device_fused): one launch per pass, or the
 * fused kernel */
static int sm_planes_device(const char *who, bool fused, int16_t *y_plane, unsigned width, unsigned height, const fiasco_amd_border *borders, unsigned n,
                            int smoothing, void *stream)
{
    if (!y_plane || (n && !borders)) { fa_set_error("%s: no plane or no borders", who); return 0; }
    if (smoothing < 0 || smoothing > 100) { fa_set_error("%s: smoothing %d (0 .. 100 per cent; there is no header here).", who, smoothing); return 0; }
    if (width < 1 || width > 8192 || height < 1 || height > 8192) {
        fa_set_error("%s: a plane of %u x %u pixels (1 .. 8192 each).", who, width, height);
        return 0;
    }
    if (!ic_have_device()) return 0;
    /* the plane is WRITTEN: an allocation that cannot be told is refused */
    int dev = -1;
    if (!ic_check_memory(who, "plane is", "plane", y_plane, (size_t) width * height * 2, "plane", &dev, true)) return 0;
    unsigned npasses = 0;
    unsigned long long pairs = 0;
    char msg[200];
    if (!sm_check(borders, n, width, height, &npasses, &pairs, msg, sizeof msg)) { fa_set_error("%s: %s", who, msg); return 0; }
    int is = 0, inegs = 0;
    if (!sm_factors(smoothing, &is, &inegs) || !npasses) return 1;             /* nothing to blend */
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    if (cur != dev && hipSetDevice(dev) != hipSuccess) { fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError())); return 0; }
    /* on the caller's stream itself: behind what it holds, before what follows.  Descriptor and tables share one small
     * allocation, filled with ONE blocking copy from a host block that lives to the end of this function, and freed once
     * the last pass has run: this call waits on the host. */
    const size_t desc_b = align_up(sizeof(SmDesc), 256), tab_b = sm_table_bytes(n, npasses);
    std::vector<char> host(desc_b + tab_b, 0);
    char *buf = nullptr;
    bool ok = sm_pack(borders, n, npasses, host.data() + desc_b, tab_b) && hipMalloc((void **) &buf, host.size()) == hipSuccess;
    if (ok) {
        SmDesc d;
        sm_describe(d, y_plane, width, height, buf + desc_b, n, npasses, is, inegs);
        memcpy(host.data(), &d, sizeof d);
        ok = hipMemcpy(buf, host.data(), host.size(), hipMemcpyHostToDevice) == hipSuccess;
    }
    unsigned long long most = 0;
    for (unsigned p = 0; p < npasses; p++) most = std::max(most, sm_pass_items(host.data() + desc_b, n, npasses, p));
    if (ok && fused) ok = sm_launch_fused((const SmDesc *) buf, 1, most, (hipStream_t) stream);
    for (unsigned p = 0; ok && !fused && p < npasses; p++)
        ok = sm_launch((const SmDesc *) buf, 1, p, sm_pass_items(host.data() + desc_b, n, npasses, p), (hipStream_t) stream);
    if (buf && hipStreamSynchronize((hipStream_t) stream) != hipSuccess) ok = false;
    if (!ok) fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
    if (buf) (void) hipFree(buf);
    if (cur >= 0 && cur != dev) (void) hipSetDevice(cur);
    return ok ? 1 : 0;
}

extern "C" int fiasco_amd_smooth_planes_device(int16_t *y_plane, unsigned width, unsigned height, const fiasco_amd_border *borders, unsigned n,
                                               int smoothing, void *stream)
{
    return sm_planes_device("fiasco_amd_smooth_planes_device", false, y_plane, width, height, borders, n, smoothing, stream);
}

/* include/libfiasco_amd_display.h */
extern "C" int fiasco_amd_smooth_planes_device_fused(int16_t *y_plane, unsigned width, unsigned height, const fiasco_amd_border *borders, unsigned n,
                                                     int smoothing, void *stream)
{
    return sm_planes_device("fiasco_amd_smooth_planes_device_fused", true, y_plane, width, height, borders, n, smoothing, stream);
}

#endif /* !SMOOTH_HOST_REPLAY */
