/*
 *  output_convert_420.inc -- decoded 4:2:0 frames as NV12 / NV21 / I420 bytes in device memory (included by core_hip.cpp
 *  behind output_convert.inc, whose kernel this one is shaped after, and smooth.inc; before frame_decoder.inc, whose
 *  flights launch it).  include/libfiasco_amd_420.h has the format and the reference's rules.
 *
 *  The device decoder leaves a 4:2:0 frame as packed 12.4 planes: Y [H][W], Cb and Cr [H >> 1][W >> 1].  ONE launch of
 *  oc420_convert_kernel per decoder flight turns the planes of all frames of the flight into bytes,
 *  clip255((p >> 4) + 128) for every plane, inside buffers the caller owns: a Y plane, and either two chroma planes
 *  (c_step 1) or one plane of interleaved pairs (c_step 2, either order).
 *
 *  Shape: frame_table.inc's -- one table entry per frame (Y4Frame), one sequence of work items.  A frame's items are of two
 *  kinds:
 *    Y        16 neighbouring pixels of one Y row: two 16-byte loads where the row allows it, one 16-byte store
 *    chroma   a row segment of its own kind, behind the frame's Y items: c_step 1: 16 samples of one row of one chroma
 *             plane, loaded and stored as a Y item's; c_step 2: 16 samples of one row of BOTH planes -- four 16-byte
 *             loads --, the pairs packed into two 16-byte stores
 *  Ragged row ends and unaligned targets take byte stores, rows that do not begin on 16 bytes narrower loads.  Global
 *  accesses, everything in registers.  The kernel moves 3 bytes per sample and is bound by that.
 *
 *  Y420_HOST_REPLAY: the per-item function alone as plain C++ (tests/yuv420_step_check.cpp, for the sanitizers).
 */
#ifdef Y420_HOST_REPLAY
#define PX_HOST_REPLAY 1
#endif
#include "px_access.inc"

struct Y4Frame {
    const int16_t      *sy, *s0, *s1;    /* the planes: Y; the chroma plane of d0 (c_step 2: of the even bytes); the other one */
    unsigned char      *dy, *d0, *d1;    /* first bytes; c_step 2: d0 is the interleaved plane, d1 unused */
    unsigned long long  y_pitch, c_pitch;
    unsigned long long  first;           /* work items of the frames before this one */
    unsigned            width, height, c_step;
    unsigned            cpr, ccpr, ny;   /* items per Y row and per chroma row; Y items: the chroma items follow them */
};

/* value k of 16 packed ones as its byte: clip255((p >> 4) + 128), arithmetic shift */
PX_DEV unsigned y4_byte(const unsigned *v, unsigned k)
{
    const int b = ((int) (int16_t) (v[k >> 1] >> (16 * (k & 1))) >> 4) + 128;
    return (unsigned) (b < 0 ? 0 : b > 255 ? 255 : b);
}

/* 16 packed values as 16 bytes in four words */
PX_DEV void y4_bytes(const unsigned v[8], unsigned w[4])
{
    w[0] = w[1] = w[2] = w[3] = 0;
#pragma unroll
    for (unsigned k = 0; k < 16; k++) w[k >> 2] |= y4_byte(v, k) << (8 * (k & 3));
}

/* work item `local' of frame F (Y4Frame::ny Y items, then the chroma items) */
PX_DEV void y4_item(const Y4Frame &F, unsigned local)
{
    unsigned v[8], w[4];
    if (local < F.ny) {
        const unsigned row = local / F.cpr, x0 = (local - row * F.cpr) * 16;
        const unsigned n = F.width - x0 < 16 ? F.width - x0 : 16;
        px_load_values(F.sy + (size_t) row * F.width + x0, n, v);
        y4_bytes(v, w);
        px_store_bytes_vec(F.dy + (size_t) row * F.y_pitch + x0, n, w);
        return;
    }
    const unsigned cw = F.width >> 1, ch = F.height >> 1;
    unsigned c = local - F.ny;
    if (F.c_step == 1) {
        const unsigned per = F.ccpr * ch, second = c >= per;
        if (second) c -= per;
        const unsigned row = c / F.ccpr, x0 = (c - row * F.ccpr) * 16;
        const unsigned n = cw - x0 < 16 ? cw - x0 : 16;
        px_load_values((second ? F.s1 : F.s0) + (size_t) row * cw + x0, n, v);
        y4_bytes(v, w);
        px_store_bytes_vec((second ? F.d1 : F.d0) + (size_t) row * F.c_pitch + x0, n, w);
        return;
    }
    const unsigned row = c / F.ccpr, x0 = (c - row * F.ccpr) * 16;
    const unsigned n = cw - x0 < 16 ? cw - x0 : 16;
    unsigned u[8], p[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
    px_load_values(F.s0 + (size_t) row * cw + x0, n, v);
    px_load_values(F.s1 + (size_t) row * cw + x0, n, u);
#pragma unroll
    for (unsigned k = 0; k < 16; k++) p[k >> 1] |= (y4_byte(v, k) | (y4_byte(u, k) << 8)) << (16 * (k & 1));
    unsigned char *q = F.d0 + (size_t) row * F.c_pitch + (size_t) x0 * 2;
    const unsigned nb = 2 * n;
    px_store_bytes_vec(q, nb >= 16 ? 16 : nb, p);
    px_store_bytes_vec(q + 16, nb > 16 ? nb - 16 : 0, p + 4);
}

#ifndef Y420_HOST_REPLAY

__global__ void __launch_bounds__(256) oc420_convert_kernel(const Y4Frame *__restrict__ frames, unsigned nframes, unsigned long long total)
{
    ft_walk<y4_item>(frames, nframes, total);
}

/* ------------------------------------------------------------------ launching */

/* a checked target (pitches filled in) and the three planes of its frame as an entry of the table.  c_step 2: the plane of
 * the even bytes is the one whose pointer is the lower */
static void y4_describe(Y4Frame &d, const int16_t *sy, const int16_t *scb, const int16_t *scr, const fiasco_amd_device_target_420 &t,
                        unsigned long long &total)
{
    const bool swap = t.c_step == 2 && (const unsigned char *) t.cr < (const unsigned char *) t.cb;      /* NV21 */
    d.sy = sy; d.s0 = swap ? scr : scb; d.s1 = swap ? scb : scr;
    d.dy = (unsigned char *) t.y; d.d0 = (unsigned char *) (swap ? t.cr : t.cb); d.d1 = (unsigned char *) (swap ? t.cb : t.cr);
    d.y_pitch = t.y_pitch; d.c_pitch = t.c_pitch; d.first = total;
    d.width = t.width; d.height = t.height; d.c_step = t.c_step;
    d.cpr = (t.width + 15) / 16; d.ccpr = ((t.width >> 1) + 15) / 16; d.ny = d.cpr * t.height;
    total += (unsigned long long) d.ny + (unsigned long long) d.ccpr * (t.height >> 1) * (t.c_step == 1 ? 2 : 1);
}

/* the packed planes of a decoded 4:2:0 frame */
static void y4_describe_packed(Y4Frame &d, const int16_t *planes, const fiasco_amd_device_target_420 &t, unsigned long long &total)
{
    const size_t npix = (size_t) t.width * t.height, cpix = (size_t) (t.width >> 1) * (t.height >> 1);
    y4_describe(d, planes, planes + npix, planes + npix + cpix, t, total);
}

static bool y4_launch(const Y4Frame *d_tab, unsigned n, unsigned long long total, int ncu, hipStream_t stream)
{
    return ft_launch(oc420_convert_kernel, d_tab, n, total, ncu, stream);
}

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_420.h) */

/* what can be said about a target without a device: c_step, the pair of a c_step 2 target, the pitches, the size, ranges
 * that overlap.  *out: the target with its pitches filled in */
static bool y4_check_geometry(unsigned i, const fiasco_amd_device_target_420 *in, unsigned width, unsigned height, fiasco_amd_device_target_420 *out,
                              unsigned coded_w = 0, unsigned coded_h = 0, int magnify = 0)
{
    *out = *in;
    if (in->c_step != 1 && in->c_step != 2) {
        fa_set_error("<4:2:0 target %u>: c_step %u (1: two chroma planes, 2: one plane of interleaved pairs).", i, in->c_step);
        return false;
    }
    if (!in->cb || !in->cr) { fa_set_error("<4:2:0 target %u>: no chroma pointers.", i); return false; }
    const unsigned char *y = (const unsigned char *) in->y, *cb = (const unsigned char *) in->cb, *cr = (const unsigned char *) in->cr;
    if (in->c_step == 2 && cr != cb + 1 && cb != cr + 1) {
        fa_set_error("<4:2:0 target %u>: c_step 2 with chroma pointers that are not one byte apart (cr == cb + 1: NV12, cb == cr + 1: NV21).", i);
        return false;
    }
    if (in->width != width || in->height != height) {
        if (magnify) fa_set_error("<4:2:0 target %u>: %u x %u pixels for a frame of %u x %u at magnification %d: %u x %u.", i, in->width, in->height,
                                  coded_w, coded_h, magnify, width, height);
        else fa_set_error("<4:2:0 target %u>: %u x %u pixels for a frame of %u x %u.", i, in->width, in->height, width, height);
        return false;
    }
    const size_t cw = width >> 1, ch = height >> 1, crow = cw * in->c_step;
    if (!out->y_pitch) out->y_pitch = width;
    if (!out->c_pitch) out->c_pitch = crow;
    if (out->y_pitch < width) {
        fa_set_error("<4:2:0 target %u>: Y pitch of %lu bytes is smaller than a row of %u bytes.", i, (unsigned long) out->y_pitch, width);
        return false;
    }
    if (out->c_pitch < crow) {
        fa_set_error("<4:2:0 target %u>: chroma pitch of %lu bytes is smaller than a row of %lu bytes.", i, (unsigned long) out->c_pitch, (unsigned long) crow);
        return false;
    }
    const size_t y_ext = (size_t) (height - 1) * out->y_pitch + width, c_ext = (ch - 1) * out->c_pitch + crow;
    const unsigned char *c0 = cb < cr ? cb : cr, *c1 = cb < cr ? cr : cb;
    const unsigned char *cfirst[2] = { c0, c1 };
    for (unsigned k = 0; k < in->c_step % 2 + 1; k++)         /* c_step 2: the one interleaved plane begins at c0 */
        if (y < cfirst[k] + c_ext && cfirst[k] < y + y_ext) {
            fa_set_error("<4:2:0 target %u>: the Y rows and the chroma rows overlap.", i);
            return false;
        }
    if (in->c_step == 1) {
        /* two planes of one pitch: side by side in one surface is fine, sharing a byte is not */
        const size_t d = (size_t) (c1 - c0), r = d % out->c_pitch;
        if (d < c_ext && (r < cw || out->c_pitch - r < cw)) {
            fa_set_error("<4:2:0 target %u>: the Cb rows and the Cr rows overlap.", i);
            return false;
        }
    }
    return true;
}

/* the rest: every range written is device memory inside one allocation, all on one device (*device) */
static bool y4_check_memory(unsigned i, const fiasco_amd_device_target_420 &t, int *device)
{
    const size_t cw = t.width >> 1, ch = t.height >> 1;
    const unsigned char *cb = (const unsigned char *) t.cb, *cr = (const unsigned char *) t.cr;
    const void *first[3] = { t.y, t.c_step == 2 ? (cb < cr ? t.cb : t.cr) : t.cb, t.cr };
    const size_t ext[3] = { (size_t) (t.height - 1) * t.y_pitch + t.width, (ch - 1) * t.c_pitch + cw * t.c_step, (ch - 1) * t.c_pitch + cw };
    const char *name[3] = { "Y", t.c_step == 2 ? "chroma" : "Cb", "Cr" };
    char who[32];
    snprintf(who, sizeof who, "<4:2:0 target %u>", i);
    *device = -1;
    for (unsigned k = 0; k < (t.c_step == 2 ? 2u : 3u); k++) {
        char is[24], rows[24], plane[24];
        int dev = -1;
        snprintf(is, sizeof is, "%s plane is", name[k]);
        snprintf(rows, sizeof rows, "%s rows", name[k]);
        snprintf(plane, sizeof plane, "%s plane", name[k]);
        if (!ic_check_memory(who, is, rows, first[k], ext[k], plane, &dev)) return false;
        if (*device >= 0 && dev != *device) {
            fa_set_error("<4:2:0 target %u>: its planes live on devices %d and %d.", i, *device, dev);
            return false;
        }
        *device = dev;
    }
    return true;
}

extern "C" int fiasco_amd_batch_decode_device_420(const fiasco_amd_batch_t *b, int magnify, int smoothing,
                                                  const fiasco_amd_device_target_420 *targets, void *stream)
{
    const char *who = "fiasco_amd_batch_decode_device_420";
    if (!b || !b->n) { fa_set_error("%s: empty batch", who); return 0; }
    const char *refuse = targets ? sm_refuse(smoothing) : "no targets";
    if (refuse) { fa_set_error("%s: %s", who, refuse); return 0; }
    const unsigned n = b->n;
    std::vector<fiasco_amd_device_target_420> checked(n, fiasco_amd_device_target_420());
    for (unsigned i = 0; i < n; i++) {
        if (!targets[i].y) continue;
        const fa_image *im = b->jobs[i].image;
        unsigned w = im->width, h = im->height;
        if (magnify && !fiasco_amd_magnified_size(im->width, im->height, magnify, &w, &h)) return 0;
        if (!y4_check_geometry(i, &targets[i], w, h, &checked[i], im->width, im->height, magnify)) return 0;
    }
    /* from here on as the other batch entries: a device, a finished pass, the jobs; OcBatch::target says which frames are
     * wanted (data: the Y plane) */
    OcBatch B;
    if (!oc_batch_jobs(who, nullptr, b, nullptr, B, magnify)) return 0;
    for (unsigned i = 0; i < n; i++) {
        if (B.jobs[i].skip || !targets[i].y) continue;
        int tdev = -1;
        if (!y4_check_memory(i, checked[i], &tdev)) return 0;
        if (tdev != B.device[i]) {
            fa_set_error("<4:2:0 target %u>: the target lives on device %d, the frame is decoded on device %d (no peer copy on this path).", i, tdev, B.device[i]);
            return 0;
        }
        B.jobs[i].format_420 = 1;
        B.target[i].data = checked[i].y; B.target[i].width = checked[i].width; B.target[i].height = checked[i].height;
    }
    sm_batch_jobs(b, B, smoothing);
    return oc_decode_batch(who, b, B, 0, stream, nullptr, checked.data());
}

extern "C" int fiasco_amd_planes_to_420_device(const int16_t *planes_y, const int16_t *planes_cb, const int16_t *planes_cr,
                                               unsigned width, unsigned height, const fiasco_amd_device_target_420 *target, void *stream)
{
    const char *who = "fiasco_amd_planes_to_420_device";
    if (!planes_y || !planes_cb || !planes_cr || !target || !target->y) { fa_set_error("%s: no planes or no target", who); return 0; }
    if (width < 2 || width > 8192 || height < 2 || height > 8192 || ((width | height) & 1)) {
        fa_set_error("%s: planes of %u x %u pixels (even, 2 .. 8192 each).", who, width, height);
        return 0;
    }
    fiasco_amd_device_target_420 t;
    if (!y4_check_geometry(0, target, width, height, &t)) return 0;
    if (!ic_have_device()) return 0;
    int tdev = -1;
    if (!y4_check_memory(0, t, &tdev)) return 0;
    const int16_t *src[3] = { planes_y, planes_cb, planes_cr };
    const size_t bytes[3] = { (size_t) width * height * 2, (size_t) (width >> 1) * (height >> 1) * 2, (size_t) (width >> 1) * (height >> 1) * 2 };
    for (unsigned k = 0; k < 3; k++) {
        int pdev = -1;
        if (!ic_check_memory(who, "planes are", "planes", src[k], bytes[k], nullptr, &pdev)) return 0;
        if (pdev != tdev) {
            fa_set_error("<4:2:0 target 0>: the target lives on device %d, the planes on device %d (no peer copy on this path).", tdev, pdev);
            return 0;
        }
    }
    Y4Frame h;
    unsigned long long total = 0;
    y4_describe(h, planes_y, planes_cb, planes_cr, t, total);
    return ft_run_alone(&h, sizeof h, [&](const void *d_tab, int ncu) { return y4_launch((const Y4Frame *) d_tab, 1, total, ncu, (hipStream_t) stream); },
                        tdev, (hipStream_t) stream);
}

#endif      /* Y420_HOST_REPLAY */
