/*
 *  render.inc -- decoded frames as the pixels of a display surface in device memory (included by core_hip.cpp behind
 *  output_convert.inc, whose kernel this one is shaped after, and smooth.inc, whose batch entry its batch entry follows;
 *  before frame_decoder.inc, whose flights launch it).
 *
 *  include/libfiasco_amd_render.h has the arithmetic -- the reference's renderer, lib/dither.c -- and host/fa_render.c the
 *  plain loop.  Here ONE launch of rd_render_kernel per decoder flight turns the 12.4 planes of all frames of the flight
 *  into 16, 24 or 32 bits per pixel inside surfaces the caller owns, every pixel doubled in both directions if the
 *  renderer says so.  The four chroma table entries of a pixel are evaluated in double as oc_convert_kernel evaluates
 *  them (nothing contracted into a fused multiply-add); the pixel word is packed arithmetically from the renderer's
 *  shift counts, which travel as a kernel argument: no lookup table.  Blue is not shifted, as in the reference.
 *
 *  Shape: frame_table.inc's, over the flight's table of OcFrame (dst, pitch: the surface's; width, height: the frame's;
 *  layout: GRAY8 for a gray frame, anything else Y, Cb, Cr).  A work item is 16 neighbouring pixels of one source row,
 *  loaded as oc_convert_kernel loads them.  An item owns 16 * bpp / 8 contiguous bytes of its row, twice that and in two
 *  rows when doubled -- 32 .. 128 bytes per row -- and writes them in pieces of 16 bytes: one vector store each where the
 *  address allows it, 4-, 2- or 1-byte stores at a ragged row end or on a surface that is not aligned to 16 bytes
 *  (px_store_bytes_wide).  The doubled row is written in the same pass, not by a second one.  Doubled, the lanes of a wave
 *  would store 64 .. 128 bytes apart and every store instruction would touch 64 lines; there the wave exchanges its pieces through LDS first (RdWave: every lane puts the bytes of its row, then takes the 16 bytes
 *  that follow its left neighbour's), so that neighbouring lanes store neighbouring bytes wherever their items are
 *  neighbours in a row.  Same bytes, same owners of every byte's value; only which lane issues the store changes.
 *
 *  RENDER_HOST_REPLAY: the per-item functions alone as plain C++ (tests/render_step_check.cpp, for the sanitizers).
 */
#ifdef RENDER_HOST_REPLAY
#define PX_HOST_REPLAY 1
#endif
#include "px_access.inc"

/* the renderer as the kernel takes it (fiasco_amd_renderer without the shift it does not apply) */
struct RdParams { unsigned bpp, doubled, rgb, r_drop, g_drop, b_drop, r_up, g_up; };

/* the 16 pixels of an item as they lie in memory: the pixel word at 16 and 32 bpp, three bytes at 24 bpp.  y, cbv, crv:
 * 16 packed values each (cbv, crv unused for gray).  CSH 1: pixel k takes chroma value k >> 1 -- the 8 samples a row of
 * 16 pixels has in 4:2:0 (render_420.inc); 0 leaves this function as it was */
template <unsigned CSH = 0> PX_DEV void rd_pixels(const RdParams &P, bool color, const unsigned y[8], const unsigned cbv[8], const unsigned crv[8], unsigned pw[16])
{
#ifndef RENDER_HOST_REPLAY
#pragma clang fp contract(off)
#endif
#pragma unroll
    for (unsigned k = 0; k < 16; k++) {
        const int yval = px_int(y, k) + 128;
        unsigned r, g, bl;
        if (color) {
            int cb = px_int(cbv, k >> CSH), cr = px_int(crv, k >> CSH);
            cb = cb < -128 ? -128 : cb > 127 ? 127 : cb;
            cr = cr < -128 ? -128 : cr > 127 ? 127 : cr;
            /* lib/dither.c:155-158, character for character: double arithmetic, C truncation */
            const int rr = (int) ( 1.4022 * cr + 0.5);
            const int rg = (int) (-0.7145 * cr + 0.5);
            const int bg = (int) (-0.3456 * cb + 0.5);
            const int bb = (int) ( 1.7710 * cb + 0.5);
            r = px_clip255(yval + rr); g = px_clip255(yval + rg + bg); bl = px_clip255(yval + bb);
        } else r = g = bl = px_clip255(yval);
        if (P.bpp == 24) pw[k] = P.rgb ? r | (g << 8) | (bl << 16) : bl | (g << 8) | (r << 16);
        else pw[k] = ((r >> P.r_drop) << P.r_up) | ((g >> P.g_drop) << P.g_up) | (bl >> P.b_drop);      /* blue: not shifted (lib/dither.c:205-208) */
    }
}

/* word m of the bytes an item writes into one row: B bytes per pixel, every pixel DUP times */
template <unsigned B, unsigned DUP> PX_DEV unsigned rd_word(const unsigned pw[16], unsigned m)
{
    if (B == 4) return pw[m / DUP];
    if (B == 2) return (pw[(2 * m) / DUP] & 0xffffu) | (pw[(2 * m + 1) / DUP] << 16);
    unsigned w = 0;
#pragma unroll
    for (unsigned j = 0; j < 4; j++) {
        const unsigned i = 4 * m + j;
        w |= ((pw[(i / 3) / DUP] >> (8 * (i % 3))) & 0xffu) << (8 * j);
    }
    return w;
}

/* the `n' pixels of an item into q0 (and q1, the row below, when DUP == 2): 16 * B * DUP bytes at most, in pieces of 16 */
template <unsigned B, unsigned DUP> PX_DEV void rd_emit(const unsigned pw[16], unsigned n, unsigned char *q0, unsigned char *q1)
{
    const unsigned nb = n * B * DUP;
#pragma unroll
    for (unsigned c = 0; c < B * DUP; c++) {
        if (16 * c < nb) {
            const unsigned w[4] = { rd_word<B, DUP>(pw, 4 * c), rd_word<B, DUP>(pw, 4 * c + 1), rd_word<B, DUP>(pw, 4 * c + 2), rd_word<B, DUP>(pw, 4 * c + 3) };
            const unsigned k = nb - 16 * c < 16 ? nb - 16 * c : 16;
            px_store_bytes_wide(q0 + 16 * c, k, w);
            if (DUP == 2) px_store_bytes_wide(q1 + 16 * c, k, w);
        }
    }
}

/* the first byte an item owns: column x0 of source row `row' in the surface at dst */
PX_DEV unsigned char *rd_first(const RdParams &P, unsigned char *dst, unsigned long long pitch, unsigned row, unsigned x0)
{
    const unsigned dup = P.doubled ? 2 : 1;
    return dst + (size_t) row * dup * pitch + (size_t) x0 * dup * (P.bpp / 8);
}

/* the `n' pixels pw of an item that begins at column x0 of source row `row', into the surface at dst */
PX_DEV void rd_store(const RdParams &P, const unsigned pw[16], unsigned n, unsigned char *dst, unsigned long long pitch, unsigned row, unsigned x0)
{
    unsigned char *q0 = rd_first(P, dst, pitch, row, x0), *q1 = P.doubled ? q0 + pitch : q0;
    if (P.bpp == 16) { if (P.doubled) rd_emit<2, 2>(pw, n, q0, q1); else rd_emit<2, 1>(pw, n, q0, q1); }
    else if (P.bpp == 24) { if (P.doubled) rd_emit<3, 2>(pw, n, q0, q1); else rd_emit<3, 1>(pw, n, q0, q1); }
    else { if (P.doubled) rd_emit<4, 2>(pw, n, q0, q1); else rd_emit<4, 1>(pw, n, q0, q1); }
}

/* one work item: `n' (1 .. 16) pixels that begin at column x0 of source row `row', into the surface at dst */
PX_DEV void rd_item(const RdParams &P, bool color, const unsigned y[8], const unsigned cbv[8], const unsigned crv[8], unsigned n,
                    unsigned char *dst, unsigned long long pitch, unsigned row, unsigned x0)
{
    unsigned pw[16];
    rd_pixels(P, color, y, cbv, crv, pw);
    rd_store(P, pw, n, dst, pitch, row, x0);
}

/* ------------------------------------------------------------------ doubled surfaces: the exchange inside a wave
 * What the 64 lanes of a wave hand each other between two barriers.  A lane's item owns ROWB = 32 B bytes of a row (B
 * bytes per pixel, 16 pixels, each twice): rd_wave_put lays them at lane * ROWB, its 16-byte pieces rotated by the lane
 * number (so that the lanes of a write and of a read spread over the banks), beside the address of the item's first
 * byte, the pitch of its surface and the bytes it owns (0: the lane has no item).  rd_wave_store then lets lane L take
 * piece c * 64 + L of the wave's ROWB * 64 bytes for c = 0 .. ROWB / 16 - 1 -- the piece of lane j = that / (ROWB / 16) --
 * and store it where lane j would have: into j's row and the row below. */
enum { RD_LANES = 64 };
struct alignas(16) RdWave {
    unsigned           piece[RD_LANES * 32];
    unsigned long long q0[RD_LANES], pitch[RD_LANES];
    unsigned           nb[RD_LANES];
};

template <unsigned B> PX_DEV void rd_wave_put(RdWave &W, unsigned lane, const unsigned pw[16], unsigned n, unsigned char *q0, unsigned long long pitch)
{
    const unsigned CH = 2 * B;
    W.q0[lane] = (unsigned long long) (size_t) q0; W.pitch[lane] = pitch; W.nb[lane] = n * B * 2;
#pragma unroll
    for (unsigned c = 0; c < CH; c++)
        *(px_u4 *) (W.piece + 4 * (lane * CH + (c + lane) % CH)) = px_u4{ rd_word<B, 2>(pw, 4 * c), rd_word<B, 2>(pw, 4 * c + 1), rd_word<B, 2>(pw, 4 * c + 2),
                                                                        rd_word<B, 2>(pw, 4 * c + 3) };
}

template <unsigned B> PX_DEV void rd_wave_store(const RdWave &W, unsigned lane)
{
    const unsigned CH = 2 * B;
#pragma unroll
    for (unsigned c = 0; c < CH; c++) {
        const unsigned piece = c * RD_LANES + lane, j = piece / CH, cj = piece - j * CH, off = 16 * cj, nb = W.nb[j];
        if (off < nb) {
            const px_u4 v = *(const px_u4 *) (W.piece + 4 * (j * CH + (cj + j) % CH));
            const unsigned w[4] = { v.x, v.y, v.z, v.w }, k = nb - off < 16 ? nb - off : 16;
            unsigned char *q = (unsigned char *) (size_t) W.q0[j] + off;
            px_store_bytes_wide(q, k, w);
            px_store_bytes_wide(q + W.pitch[j], k, w);
        }
    }
}

/* a lane's part before the barrier (n == 0: no item) and after it */
PX_DEV void rd_wave_put_any(const RdParams &P, RdWave &W, unsigned lane, const unsigned pw[16], unsigned n, unsigned char *q0, unsigned long long pitch)
{
    if (P.bpp == 16) rd_wave_put<2>(W, lane, pw, n, q0, pitch); else if (P.bpp == 24) rd_wave_put<3>(W, lane, pw, n, q0, pitch); else rd_wave_put<4>(W, lane, pw, n, q0, pitch);
}
PX_DEV void rd_wave_store_any(const RdParams &P, const RdWave &W, unsigned lane)
{
    if (P.bpp == 16) rd_wave_store<2>(W, lane); else if (P.bpp == 24) rd_wave_store<3>(W, lane); else rd_wave_store<4>(W, lane);
}

#ifndef RENDER_HOST_REPLAY

/* EXCHANGE: the doubled renderers; every thread of the workgroup then stays in the loop to the end (the barriers).  So
 * this kernel keeps a loop of its own, for both builds, around frame_table.inc's stretch, search and step */
template <bool EXCHANGE>
__global__ void __launch_bounds__(256) rd_render_kernel(const OcFrame *__restrict__ frames, unsigned nframes, unsigned long long total, RdParams P)
{
    unsigned long long t0, t1;
    if (!ft_stretch(total, t0, t1)) return;
    unsigned f = ft_find(frames, nframes, t0 * FT_TILE);
    for (unsigned long long t = t0; t < t1; t++) {
        const unsigned long long it = t * FT_TILE + threadIdx.x;
        const bool valid = it < total;
        if (!EXCHANGE && !valid) break;
        unsigned pw[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 }, n = 0;
        unsigned char *q0 = nullptr;
        unsigned long long pitch = 0;
        if (valid) {
            f = ft_step(frames, nframes, f, it);
            const OcFrame F = frames[f];
            const unsigned local = (unsigned) (it - F.first);
            const unsigned row = local / F.cpr, x0 = (local - row * F.cpr) * 16;
            n = F.width - x0 < 16 ? F.width - x0 : 16;
            const size_t npix = (size_t) F.width * F.height;
            const int16_t *p = F.src + (size_t) row * F.width + x0;
            const bool color = F.layout != FIASCO_AMD_GRAY8;
            unsigned y[8], cbv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, crv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            px_load_values(p, n, y);
            if (color) { px_load_values(p + npix, n, cbv); px_load_values(p + 2 * npix, n, crv); }
            if (!EXCHANGE) { rd_item(P, color, y, cbv, crv, n, F.dst, F.pitch, row, x0); continue; }
            rd_pixels(P, color, y, cbv, crv, pw);
            q0 = rd_first(P, F.dst, F.pitch, row, x0); pitch = F.pitch;
        }
        if constexpr (EXCHANGE) {
            __shared__ RdWave waves[4];
            RdWave &W = waves[threadIdx.x / RD_LANES];
            rd_wave_put_any(P, W, threadIdx.x % RD_LANES, pw, n, q0, pitch);
            __syncthreads();
            rd_wave_store_any(P, W, threadIdx.x % RD_LANES);
            __syncthreads();
        }
    }
}

/* ------------------------------------------------------------------ launching */

static RdParams rd_params(const fiasco_amd_renderer *r)
{
    return RdParams{ r->bpp, r->doubled, r->rgb, r->r_drop, r->g_drop, r->b_drop, r->r_up, r->g_up };
}

/* oc_launch for the rendering kernel: the table is one oc_describe filled, with the surface as the target */
static bool rd_launch(const OcFrame *d_tab, unsigned n, unsigned long long total, const fiasco_amd_renderer *r, int ncu, hipStream_t stream)
{
    return ft_launch(r->doubled ? rd_render_kernel<true> : rd_render_kernel<false>, d_tab, n, total, ncu, stream, rd_params(r));
}

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_render.h) */

/* a caller's surface for a frame of width x height (color) under renderer r: oc_check_target's rules -- the size,
 * device memory, rows inside the allocation -- and the alignment of the pixels.  *out: the surface as a target of the
 * FRAME's size (what oc_describe takes), pitch filled in; *device: where it lives */
static bool rd_check_surface(unsigned i, const fiasco_amd_device_surface *in, const fiasco_amd_renderer *r, unsigned width, unsigned height, int color,
                             fiasco_amd_device_frame *out, int *device, bool c420 = false)
{
    unsigned sw = 0, sh = 0;
    size_t row = 0;
    /* c420: the frame is decoded in 4:2:0 and the size rule is that format's (libfiasco_amd_render_420.h) */
    if (!(c420 ? fiasco_amd_renderer_surface_size_420(r, width, height, &sw, &sh, &row) : fiasco_amd_renderer_surface_size(r, width, height, color, &sw, &sh, &row)))
        return false;
    if (in->width != sw || in->height != sh) {
        fa_set_error("<device surface %u>: %u x %u pixels for a frame of %u x %u%s: %u x %u.", i, in->width, in->height, width, height,
                     r->doubled ? " doubled" : "", sw, sh);
        return false;
    }
    const size_t pitch = in->pitch ? in->pitch : row, unit = r->bpp == 24 ? 1 : r->bpp / 8;
    if (pitch < row) {
        fa_set_error("<device surface %u>: pitch of %lu bytes is smaller than a row of %lu bytes.", i, (unsigned long) pitch, (unsigned long) row);
        return false;
    }
    if ((size_t) in->data % unit || pitch % unit) {
        fa_set_error("<device surface %u>: the pixels and the pitch must be aligned to the %lu bytes of a pixel.", i, (unsigned long) unit);
        return false;
    }
    /* these rows are WRITTEN: a surface whose allocation cannot be told is refused */
    char name[32];
    snprintf(name, sizeof name, "<device surface %u>", i);
    if (!ic_check_memory(name, "pixels are", "rows", in->data, (size_t) (sh - 1) * pitch + row, "pixels", device)) return false;
    out->data = in->data; out->pitch = pitch; out->plane_stride = 0;
    out->width = width; out->height = height; out->layout = color ? FIASCO_AMD_RGB8_INTERLEAVED : FIASCO_AMD_GRAY8;
    return true;
}

extern "C" int fiasco_amd_planes_render_device(const int16_t *planes, int color, unsigned width, unsigned height, const fiasco_amd_renderer_t *r,
                                               const fiasco_amd_device_surface *surface, void *stream)
{
    const char *who = "fiasco_amd_planes_render_device";
    if (!planes || !r || !surface || !surface->data) { fa_set_error("%s: no planes, no renderer or no surface", who); return 0; }
    if (!ic_have_device()) return 0;
    fiasco_amd_device_frame t;
    int tdev = -1, pdev = -1;
    if (!rd_check_surface(0, surface, r, width, height, color, &t, &tdev)) return 0;
    const size_t bytes = (size_t) width * height * (color ? 3 : 1) * 2;
    if (!ic_check_memory(who, "planes are", "planes", planes, bytes, nullptr, &pdev)) return 0;
    if ((size_t) planes & 1) { fa_set_error("%s: the planes are not aligned to their 16-bit values.", who); return 0; }
    if (pdev != tdev) {
        fa_set_error("<device surface 0>: the surface lives on device %d, the planes on device %d (no peer copy on this path).", tdev, pdev);
        return 0;
    }
    OcFrame h;
    unsigned long long total = 0;
    oc_describe(h, planes, t, total);
    return ft_run_alone(&h, sizeof h, [&](const void *d_tab, int ncu) { return rd_launch((const OcFrame *) d_tab, 1, total, r, ncu, (hipStream_t) stream); },
                        tdev, (hipStream_t) stream);
}

/* fiasco_amd_batch_decode_device_shown()'s path (smooth.inc) with surfaces for targets: the jobs, the devices and the
 * smoothing are its own, the flights' consumer launches rd_render_kernel where OcOut::render is set */
extern "C" int fiasco_amd_batch_decode_device_rendered(const fiasco_amd_batch_t *b, const fiasco_amd_renderer_t *r, int magnify, int smoothing,
                                                       const fiasco_amd_device_surface *surfaces, void *stream)
{
    OcBatch B;
    const char *who = "fiasco_amd_batch_decode_device_rendered";
    if (!oc_batch_jobs(who, !r ? "no renderer" : !surfaces ? "no surfaces" : sm_refuse(smoothing), b, nullptr, B, magnify)) return 0;
    for (unsigned i = 0; i < b->n; i++) {
        if (B.jobs[i].skip || !surfaces[i].data) continue;
        const fa_image *im = b->jobs[i].image;
        unsigned w = im->width, h = im->height;
        int sdev = -1;
        if (magnify && !fiasco_amd_magnified_size(im->width, im->height, magnify, &w, &h)) return 0;
        if (!rd_check_surface(i, &surfaces[i], r, w, h, im->color, &B.target[i], &sdev)) return 0;
        if (sdev != B.device[i]) {
            fa_set_error("<device surface %u>: the surface lives on device %d, the frame is decoded on device %d (no peer copy on this path).", i, sdev, B.device[i]);
            return 0;
        }
    }
    sm_batch_jobs(b, B, smoothing);
    return oc_decode_batch(who, b, B, 0, stream, r);
}

#endif /* RENDER_HOST_REPLAY */
