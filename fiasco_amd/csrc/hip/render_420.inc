/*
 *  render_420.inc -- frames decoded in 4:2:0 as the pixels of a display surface in device memory (included by core_hip.cpp
 *  behind render.inc, whose per-pixel arithmetic, stores and wave exchange this file uses, and output_convert_420.inc, whose
 *  planes it reads; before frame_decoder.inc, whose flights launch it).  include/libfiasco_amd_render_420.h has the rules.
 *
 *  The device decoder leaves a 4:2:0 frame as packed 12.4 planes: Y [H][W], Cb and Cr [H >> 1][W >> 1], W and H even.  The
 *  reference's viewer (bin/dwfa.c with lib/dither.c) renders such a frame with every chroma sample standing for its 2 x 2
 *  pixels.  ONE launch of rd420_render_kernel per decoder flight writes the surfaces of all frames of the flight.
 *
 *  Shape: frame_table.inc's, over the flight's table of Rd4Frame.  A work item is 8 neighbouring chroma samples of one
 *  chroma row: 16 neighbouring Y pixels in each of the two rows above them.  The chroma values are loaded once per item
 *  (two loads of 16 bytes worth of values) and serve both rows; each row then is an item of rd_render_kernel: rd_pixels,
 *  fed chroma value k >> 1 for pixel k, and rd_emit through rd_store.  The compiler sees both rows in one body and
 *  evaluates the four table entries of a chroma sample once for its four pixels.  Doubled, an item writes four surface rows;
 *  there the wave exchanges its pieces through LDS as rd_render_kernel does (RdWave), once per source row, so that
 *  neighbouring lanes store neighbouring bytes.  Global accesses apart from that exchange, everything else in registers.
 *
 *  RENDER420_HOST_REPLAY: the per-item functions alone as plain C++, render.inc's with them (tests/render_420_step_check.cpp,
 *  for the sanitizers).
 */
#ifdef RENDER420_HOST_REPLAY
#define RENDER_HOST_REPLAY 1
#include "render.inc"
#endif

struct Rd4Frame {
    const int16_t      *sy, *s0, *s1;    /* the planes: Y, Cb, Cr */
    unsigned char      *dst;             /* the surface */
    unsigned long long  pitch;
    unsigned long long  first;           /* work items of the frames before this one */
    unsigned            width, height;   /* the frame's: even */
    unsigned            cpr;             /* items per chroma row */
};

/* what item `local' of frame F reads: the values of its two Y rows and of its chroma samples.  crow: the chroma row; x0:
 * the first Y column; returns the pixels per row (2 .. 16, even) */
PX_DEV unsigned rd4_load(const Rd4Frame &F, unsigned local, unsigned y0[8], unsigned y1[8], unsigned cbv[8], unsigned crv[8], unsigned &crow, unsigned &x0)
{
    crow = local / F.cpr; x0 = (local - crow * F.cpr) * 16;
    const unsigned n = F.width - x0 < 16 ? F.width - x0 : 16, cw = F.width >> 1;
    const int16_t *p = F.sy + (size_t) crow * 2 * F.width + x0;
    const size_t c = (size_t) crow * cw + (x0 >> 1);
    px_load_values(F.s0 + c, n >> 1, cbv);
    px_load_values(F.s1 + c, n >> 1, crv);
    px_load_values(p, n, y0);
    px_load_values(p + F.width, n, y1);
    return n;
}

/* one work item without the exchange: both Y rows of its chroma samples into the surface */
PX_DEV void rd4_item(const Rd4Frame &F, unsigned local, const RdParams &P)
{
    unsigned y0[8], y1[8], cbv[8], crv[8], pw[16], crow, x0;
    const unsigned n = rd4_load(F, local, y0, y1, cbv, crv, crow, x0);
    rd_pixels<1>(P, true, y0, cbv, crv, pw);
    rd_store(P, pw, n, F.dst, F.pitch, 2 * crow, x0);
    rd_pixels<1>(P, true, y1, cbv, crv, pw);
    rd_store(P, pw, n, F.dst, F.pitch, 2 * crow + 1, x0);
}

#ifndef RENDER420_HOST_REPLAY

/* one source row of an item through the exchange of its wave: the two surface rows at q0 (n == 0: the lane has no item and
 * stores nothing of its own).  Every thread of the workgroup passes both barriers */
static __device__ __forceinline__ void rd4_exchange_row(const RdParams &P, RdWave &W, const unsigned y[8], const unsigned cbv[8], const unsigned crv[8],
                                                        unsigned n, unsigned char *q0, unsigned long long pitch)
{
    unsigned pw[16];
    rd_pixels<1>(P, true, y, cbv, crv, pw);
    rd_wave_put_any(P, W, threadIdx.x % RD_LANES, pw, n, q0, pitch);
    __syncthreads();
    rd_wave_store_any(P, W, threadIdx.x % RD_LANES);
    __syncthreads();
}

/* EXCHANGE: the doubled renderers, as in rd_render_kernel: every thread of the workgroup stays in the loop to the end and
 * passes the two barriers of each of the item's two source rows */
template <bool EXCHANGE>
__global__ void __launch_bounds__(256) rd420_render_kernel(const Rd4Frame *__restrict__ frames, unsigned nframes, unsigned long long total, RdParams P)
{
    if constexpr (!EXCHANGE) { ft_walk<rd4_item>(frames, nframes, total, P); return; }
    else {
        unsigned long long t0, t1;
        if (!ft_stretch(total, t0, t1)) return;
        unsigned f = ft_find(frames, nframes, t0 * FT_TILE);
        __shared__ RdWave waves[4];
        RdWave &W = waves[threadIdx.x / RD_LANES];
        for (unsigned long long t = t0; t < t1; t++) {
            const unsigned long long it = t * FT_TILE + threadIdx.x;
            unsigned y0[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, y1[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, cbv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 }, crv[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
            unsigned n = 0;
            unsigned char *q0 = nullptr;
            unsigned long long pitch = 0;
            if (it < total) {
                f = ft_step(frames, nframes, f, it);
                const Rd4Frame F = frames[f];
                unsigned crow, x0;
                n = rd4_load(F, (unsigned) (it - F.first), y0, y1, cbv, crv, crow, x0);
                q0 = rd_first(P, F.dst, F.pitch, 2 * crow, x0); pitch = F.pitch;
            }
            rd4_exchange_row(P, W, y0, cbv, crv, n, q0, pitch);
            rd4_exchange_row(P, W, y1, cbv, crv, n, q0 + 2 * pitch, pitch);
        }
    }
}

/* ------------------------------------------------------------------ launching */

/* a checked surface (data, pitch; width, height: the frame's) and the three planes of its frame as an entry of the table */
static void rd4_describe(Rd4Frame &d, const int16_t *sy, const int16_t *scb, const int16_t *scr, const void *data, size_t pitch, unsigned width, unsigned height,
                         unsigned long long &total)
{
    d.sy = sy; d.s0 = scb; d.s1 = scr; d.dst = (unsigned char *) data; d.pitch = pitch; d.first = total;
    d.width = width; d.height = height; d.cpr = (width + 15) / 16;
    total += (unsigned long long) d.cpr * (height >> 1);
}

/* the packed planes of a decoded 4:2:0 frame (y4_describe_packed) */
static void rd4_describe_packed(Rd4Frame &d, const int16_t *planes, const fiasco_amd_device_target_420 &t, unsigned long long &total)
{
    const size_t npix = (size_t) t.width * t.height, cpix = (size_t) (t.width >> 1) * (t.height >> 1);
    rd4_describe(d, planes, planes + npix, planes + npix + cpix, t.y, t.y_pitch, t.width, t.height, total);
}

static bool rd4_launch(const Rd4Frame *d_tab, unsigned n, unsigned long long total, const fiasco_amd_renderer *r, int ncu, hipStream_t stream)
{
    return ft_launch(r->doubled ? rd420_render_kernel<true> : rd420_render_kernel<false>, d_tab, n, total, ncu, stream, rd_params(r));
}

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_render_420.h) */

extern "C" int fiasco_amd_planes_render_device_420(const int16_t *planes_y, const int16_t *planes_cb, const int16_t *planes_cr, unsigned width, unsigned height,
                                                   const fiasco_amd_renderer_t *r, const fiasco_amd_device_surface *surface, void *stream)
{
    const char *who = "fiasco_amd_planes_render_device_420";
    if (!planes_y || !planes_cb || !planes_cr || !r || !surface || !surface->data) { fa_set_error("%s: no planes, no renderer or no surface", who); return 0; }
    if (!ic_have_device()) return 0;
    fiasco_amd_device_frame t;
    int tdev = -1;
    if (!rd_check_surface(0, surface, r, width, height, 1, &t, &tdev, true)) return 0;
    const int16_t *src[3] = { planes_y, planes_cb, planes_cr };
    const size_t cbytes = (size_t) (width >> 1) * (height >> 1) * 2, bytes[3] = { (size_t) width * height * 2, cbytes, cbytes };
    for (unsigned k = 0; k < 3; k++) {
        int pdev = -1;
        if (!ic_check_memory(who, "planes are", "planes", src[k], bytes[k], nullptr, &pdev)) return 0;
        if ((size_t) src[k] & 1) { fa_set_error("%s: the planes are not aligned to their 16-bit values.", who); return 0; }
        if (pdev != tdev) {
            fa_set_error("<device surface 0>: the surface lives on device %d, the planes on device %d (no peer copy on this path).", tdev, pdev);
            return 0;
        }
    }
    Rd4Frame h;
    unsigned long long total = 0;
    rd4_describe(h, planes_y, planes_cb, planes_cr, t.data, t.pitch, width, height, total);
    return ft_run_alone(&h, sizeof h, [&](const void *d_tab, int ncu) { return rd4_launch((const Rd4Frame *) d_tab, 1, total, r, ncu, (hipStream_t) stream); },
                        tdev, (hipStream_t) stream);
}

/* fiasco_amd_batch_decode_device_420()'s jobs with surfaces for targets: OcOut::t420 carries the checked surface of every
 * frame (y, y_pitch: its first byte and pitch; width, height: the frame's), OcOut::render the renderer, and the flights'
 * consumer launches rd420_render_kernel where both are set */
extern "C" int fiasco_amd_batch_decode_device_rendered_420(const fiasco_amd_batch_t *b, const fiasco_amd_renderer_t *r, int magnify, int smoothing,
                                                           const fiasco_amd_device_surface *surfaces, void *stream)
{
    OcBatch B;
    const char *who = "fiasco_amd_batch_decode_device_rendered_420";
    if (!oc_batch_jobs(who, !r ? "no renderer" : !surfaces ? "no surfaces" : sm_refuse(smoothing), b, nullptr, B, magnify)) return 0;
    std::vector<fiasco_amd_device_target_420> checked(b->n, fiasco_amd_device_target_420());
    for (unsigned i = 0; i < b->n; i++) {
        if (B.jobs[i].skip || !surfaces[i].data) continue;
        const fa_image *im = b->jobs[i].image;
        unsigned w = im->width, h = im->height;
        int sdev = -1;
        if (magnify && !fiasco_amd_magnified_size(im->width, im->height, magnify, &w, &h)) return 0;
        if (!rd_check_surface(i, &surfaces[i], r, w, h, 1, &B.target[i], &sdev, true)) return 0;
        if (sdev != B.device[i]) {
            fa_set_error("<device surface %u>: the surface lives on device %d, the frame is decoded on device %d (no peer copy on this path).", i, sdev, B.device[i]);
            return 0;
        }
        B.jobs[i].format_420 = 1;
        checked[i].y = (void *) B.target[i].data; checked[i].y_pitch = B.target[i].pitch; checked[i].width = w; checked[i].height = h;
    }
    sm_batch_jobs(b, B, smoothing);
    return oc_decode_batch(who, b, B, 0, stream, r, checked.data());
}

#endif /* RENDER420_HOST_REPLAY */
