/*
 *  input_convert_ycbcr.inc -- frames that are YCbCr already, as they lie in device memory: NV12, NV21, I420 / YV12 and
 *  planar 4:4:4 bytes into the coder's planes (included by core_hip.cpp behind input_convert.inc, whose plumbing --
 *  ic_convert(), ic_stage_batch(), ic_upload_batch(), ic_seq_open() -- serves this kind of frame too: IcKind).
 *  include/libfiasco_amd_ycbcr.h has the definition: every plane (byte - 128) * 16, a 4:2:0 chroma sample replicated over
 *  its 2 x 2 pixels.  Integer arithmetic, nothing is rounded; host/fa_image.c fa_image_from_ycbcr() is the same in C.
 *
 *  Shape: frame_table.inc's -- one table entry per frame (IcyFrame), one sequence of work items.  Neighbouring lanes take
 *  neighbouring items of a row, so a wave reads 1 KiB of Y per load instruction and writes 2 KiB per band and row
 *  contiguously.
 *    4:2:0   an item is 16 neighbouring pixels of a ROW PAIR: two 16-byte Y loads, and one 16-byte load of 8 interleaved
 *            pairs (c_step 2) or two 8-byte loads (c_step 1) -- every chroma byte is read exactly once --, six stores of
 *            32 bytes of int16 (2 rows x 3 bands); a replicated chroma pair is one word, (v & 0xffff) * 0x10001
 *    4:4:4   an item is 16 pixels of one row: three 16-byte loads, three 32-byte stores
 *  Loads are 16-, 8- or 4-byte vectors where the address allows it (a plane whose rows start on 4 or 8 bytes only) and
 *  byte loads otherwise (a ragged row end that is no multiple of 4, a source at an odd address: px_load_bytes_wide); stores
 *  are 16-, 8- or 4-byte, a row of a plane always begins on 4 bytes (even width).  Global accesses, everything in registers.
 *  The kernel moves 1.5 + 6 bytes per pixel (4:2:0; 3 + 6 for 4:4:4).  Measured (tests/gpu_ycbcr_input_probe.py under a
 *  rocprofv3 kernel trace, profiles/ycbcr_input.json; 32 frames of 1080p, median of 22 launches): NV12 133 us, I420 130 us,
 *  4:4:4 151 us, ic_convert_kernel on interleaved RGB 156 us -- 3.7 .. 4.0 TB/s of the bytes each has to move.
 *
 *  Build (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): icy_convert_kernel 39 VGPRs, 44 SGPRs,
 *  no scratch, no LDS, 8 waves per SIMD; global_ accesses only, no flat_ one (ic_convert_kernel beside it: 132 VGPRs, 56
 *  SGPRs, no scratch, 3 waves per SIMD).
 *
 *  YCBCR_IN_HOST_REPLAY: the per-item function alone as plain C++ (tests/ycbcr_in_step_check.cpp, for the sanitizers).
 */
#ifdef YCBCR_IN_HOST_REPLAY
#define PX_HOST_REPLAY 1
#endif
#include "px_access.inc"

struct IcyFrame {
    const unsigned char *y, *c0, *c1;    /* first bytes: Y; Cb (c_step 2: the plane of pairs, the lower pointer); Cr (c_step 2: unused) */
    int16_t            *dst;             /* planes [3][height][width] */
    unsigned long long  y_pitch, c_pitch;
    unsigned long long  first;           /* work items of the frames before this one */
    unsigned            width, height, c_step, sub;
    unsigned            swap;            /* c_step 2: the even bytes are Cr (NV21) */
    unsigned            cpr;             /* items per row (4:4:4) or row pair (4:2:0) */
};

/* byte k of packed bytes as its 12.4 value, (b - 128) * 16, in the low half of a word */
PX_DEV unsigned icy_value(const unsigned *w, unsigned k)
{
    return (unsigned) (((int) ((w[k >> 2] >> (8 * (k & 3))) & 255u) - 128) * 16) & 0xffffu;
}

/* 16 bytes, one per pixel, as 16 values in packed pairs */
PX_DEV void icy_row(const unsigned w[4], unsigned out[8])
{
#pragma unroll
    for (unsigned k = 0; k < 8; k++) out[k] = icy_value(w, 2 * k) | (icy_value(w, 2 * k + 1) << 16);
}

/* work item `local' of frame F.  All loads of an item are issued before its first store: the compiler cannot know that
 * the planes and the sources do not overlap and keeps a load behind every store that precedes it in the text. */
PX_DEV void icy_item(const IcyFrame &F, unsigned local)
{
    const unsigned row = local / F.cpr, x0 = (local - row * F.cpr) * 16;
    const unsigned n = F.width - x0 < 16 ? F.width - x0 : 16;             /* even: the width is */
    const size_t npix = (size_t) F.width * F.height;
    unsigned out[8];
    if (!F.sub) {
        /* 4:4:4: 16 pixels of row `row' of the three planes */
        unsigned wy[4], wb[4], wr[4];
        int16_t *q = F.dst + (size_t) row * F.width + x0;
        px_load_bytes_wide(F.y + (size_t) row * F.y_pitch + x0, n, wy);
        px_load_bytes_wide(F.c0 + (size_t) row * F.c_pitch + x0, n, wb);
        px_load_bytes_wide(F.c1 + (size_t) row * F.c_pitch + x0, n, wr);
        icy_row(wy, out);
        px_store_values(q, n, out);
        icy_row(wb, out);
        px_store_values(q + npix, n, out);
        icy_row(wr, out);
        px_store_values(q + 2 * npix, n, out);
        return;
    }
    /* 4:2:0: 16 pixels of the rows 2 row and 2 row + 1, n / 2 samples of chroma row `row' */
    unsigned w0[4], w1[4], wc[4] = { 0, 0, 0, 0 }, u[2] = { 0, 0 }, v[2] = { 0, 0 };
    int16_t *q = F.dst + (size_t) (2 * row) * F.width + x0;
    px_load_bytes_wide(F.y + (size_t) (2 * row) * F.y_pitch + x0, n, w0);
    px_load_bytes_wide(F.y + (size_t) (2 * row + 1) * F.y_pitch + x0, n, w1);
    if (F.c_step == 2) px_load_bytes_wide(F.c0 + (size_t) row * F.c_pitch + x0, n, wc);          /* pair k at byte 2 (x0 / 2 + k) */
    else {
        px_load_bytes8(F.c0 + (size_t) row * F.c_pitch + (x0 >> 1), n >> 1, u);
        px_load_bytes8(F.c1 + (size_t) row * F.c_pitch + (x0 >> 1), n >> 1, v);
    }
    icy_row(w0, out);
    px_store_values(q, n, out);
    icy_row(w1, out);
    px_store_values(q + F.width, n, out);
    unsigned cb[8], cr[8];               /* a sample, replicated over its two pixels of a row: one word each */
    if (F.c_step == 2) {
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            const unsigned even = icy_value(wc, 2 * k) * 0x10001u, odd = icy_value(wc, 2 * k + 1) * 0x10001u;
            cb[k] = F.swap ? odd : even; cr[k] = F.swap ? even : odd;
        }
    } else {
#pragma unroll
        for (unsigned k = 0; k < 8; k++) { cb[k] = icy_value(u, k) * 0x10001u; cr[k] = icy_value(v, k) * 0x10001u; }
    }
    px_store_values(q + npix, n, cb);
    px_store_values(q + npix + F.width, n, cb);
    px_store_values(q + 2 * npix, n, cr);
    px_store_values(q + 2 * npix + F.width, n, cr);
}

#ifndef YCBCR_IN_HOST_REPLAY

__global__ void __launch_bounds__(256) icy_convert_kernel(const IcyFrame *__restrict__ frames, unsigned nframes, unsigned long long total)
{
    ft_walk<icy_item>(frames, nframes, total);
}

/* ------------------------------------------------------------------ the kind (core_hip.cpp IcKind) */

/* the plane of pairs of a c_step 2 frame begins at the lower of its two pointers */
static const unsigned char *icy_pairs(const fiasco_amd_ycbcr_frame &f)
{
    const unsigned char *cb = (const unsigned char *) f.cb, *cr = (const unsigned char *) f.cr;
    return cb < cr ? cb : cr;
}

/* the entry of the descriptor table for the checked frame f, written to dst; total: the work items of the frames before
 * it, moved on */
static void icy_describe(IcyFrame &d, const fiasco_amd_ycbcr_frame &f, int16_t *dst, unsigned long long &total)
{
    d.y = (const unsigned char *) f.y; d.dst = dst;
    d.c0 = f.c_step == 2 ? icy_pairs(f) : (const unsigned char *) f.cb;
    d.c1 = (const unsigned char *) f.cr;
    d.swap = f.c_step == 2 && (const unsigned char *) f.cr < (const unsigned char *) f.cb;
    d.y_pitch = f.y_pitch; d.c_pitch = f.c_pitch; d.first = total;
    d.width = f.width; d.height = f.height; d.c_step = f.c_step; d.sub = f.subsampling;
    d.cpr = (f.width + 15) / 16;
    total += (unsigned long long) d.cpr * (f.height >> f.subsampling);
}

static bool icy_launch(const IcyFrame *d_tab, unsigned n, unsigned long long total, int ncu, hipStream_t stream)
{
    return ft_launch(icy_convert_kernel, d_tab, n, total, ncu, stream);
}

static_assert(sizeof(IcyFrame) <= IC_ENTRY_MAX, "IC_ENTRY_MAX (core_hip.cpp) is the room of a table entry");

static const IcKind IC_YCBCR = {
    "YCbCr frame", sizeof(fiasco_amd_ycbcr_frame), sizeof(IcyFrame),
    [](const void *f, unsigned *w, unsigned *h, int *color) {
        const fiasco_amd_ycbcr_frame &F = *(const fiasco_amd_ycbcr_frame *) f;
        *w = F.width; *h = F.height; *color = 1;
    },
    [](const void *f) { return ic_device_of_pointer(((const fiasco_amd_ycbcr_frame *) f)->y); },      /* its planes lie on one device: icy_check_frame */
    [](const void *, const void **) { return (size_t) 0; },                                             /* no peer copy on this path */
    [](void *entry, const void *f, const void *, int16_t *dst, unsigned long long &total) {
        icy_describe(*(IcyFrame *) entry, *(const fiasco_amd_ycbcr_frame *) f, dst, total);
    },
    [](const void *d_tab, unsigned n, unsigned long long total, int ncu, hipStream_t stream) { return icy_launch((const IcyFrame *) d_tab, n, total, ncu, stream); },
};

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_ycbcr.h) */

/* one caller's frame: what the host entries refuse (fa_ycbcr_check), and per plane that its rows lie in device memory, in
 * their allocation and on the device of the Y plane.  *out = the frame with its pitches filled in. */
static bool icy_check_frame(unsigned i, const fiasco_amd_ycbcr_frame *in, fiasco_amd_ycbcr_frame *out)
{
    char name[32];
    if (!fa_ycbcr_check(i, in, out)) return false;
    snprintf(name, sizeof name, "<YCbCr frame %u>", i);
    const fiasco_amd_ycbcr_frame &f = *out;
    const size_t cw = f.width >> f.subsampling, ch = f.height >> f.subsampling;
    const size_t y_ext = (size_t) (f.height - 1) * f.y_pitch + f.width, c_ext = (ch - 1) * f.c_pitch + cw * f.c_step;
    if (!ic_check_memory(name, "Y plane is", "Y rows", f.y, y_ext)) return false;
    if (f.c_step == 2) { if (!ic_check_memory(name, "chroma plane is", "chroma rows", icy_pairs(f), c_ext)) return false; }
    else if (!ic_check_memory(name, "Cb plane is", "Cb rows", f.cb, c_ext) || !ic_check_memory(name, "Cr plane is", "Cr rows", f.cr, c_ext)) return false;
    const int dy = ic_device_of_pointer(f.y), db = ic_device_of_pointer(f.cb), dr = ic_device_of_pointer(f.cr);
    if (db != dy || dr != dy) {
        fa_set_error("%s: its planes live on devices %d and %d.", name, dy, db != dy ? db : dr);
        return false;
    }
    return true;
}

extern "C" fiasco_amd_batch_t *fiasco_amd_batch_stage_device_ycbcr(unsigned n, const fiasco_amd_ycbcr_frame *frames, void *stream,
                                                                   float quality, const fiasco_c_options_t *options)
{
    std::vector<fiasco_amd_ycbcr_frame> fr(n);
    if (!n || !frames) { fa_set_error("No frames to stage."); return nullptr; }
    if (quality <= 0) { fa_set_error("Compression quality has to be positive."); return nullptr; }
    if (!ic_have_device()) return nullptr;
    for (unsigned i = 0; i < n; i++) if (!icy_check_frame(i, &frames[i], &fr[i])) return nullptr;
    return ic_stage_batch(n, IcInput{ &IC_YCBCR, fr.data() }, stream, quality, options);
}

extern "C" int fiasco_amd_batch_upload_device_ycbcr(fiasco_amd_batch_t *b, const fiasco_amd_ycbcr_frame *frames, void *stream)
{
    if (!ic_upload_ready(b, frames)) return 0;
    std::vector<fiasco_amd_ycbcr_frame> fr(b->n);
    for (unsigned i = 0; i < b->n; i++) if (!icy_check_frame(i, &frames[i], &fr[i])) return 0;
    return ic_upload_batch(b, IcInput{ &IC_YCBCR, fr.data() }, stream);
}

extern "C" fiasco_amd_seq_t *fiasco_amd_seq_open_device_ycbcr(unsigned n, const fiasco_amd_ycbcr_frame *frames, void *stream, float quality,
                                                              const fiasco_c_options_t *options, unsigned rank, unsigned world)
{
    if (!ic_seq_open_ready(n, frames, quality, rank, world)) return nullptr;
    std::vector<fiasco_amd_ycbcr_frame> fr(n);
    for (unsigned i = 0; i < n; i++) if (!icy_check_frame(i, &frames[i], &fr[i])) return nullptr;
    return ic_seq_open(n, IcInput{ &IC_YCBCR, fr.data() }, stream, quality, options, rank, world);
}

#endif      /* YCBCR_IN_HOST_REPLAY */
