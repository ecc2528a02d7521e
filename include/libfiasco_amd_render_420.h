/*
 *  libfiasco_amd_render_420.h -- frames decoded in 4:2:0 in the pixel formats of a display: what the reference's viewer
 *  shows when it plays on a screen.  bin/dwfa.c:161 switches its decoder to fiasco_d_options_set_4_2_0_format, so the chroma
 *  bands come from the automaton at half the side length (libfiasco_amd_420.h), and lib/dither.c renders that image
 *  into the XImage.  Restated on the host and as a kernel that writes surfaces in device memory (C ABI, plain types).
 *
 *  The functions have a header of their own because those of the older headers are pinned sets.  The renderer, its masks,
 *  the surface and its alignment are libfiasco_amd_render.h's; the frames, their magnifications, smoothing and per-frame
 *  refusals are libfiasco_amd_420.h's.
 *
 *  Arithmetic, for pixel (x, y) of a frame of W x H, both even, with planes Y [H][W], Cb and Cr [H >> 1][W >> 1] of 12.4 values:
 *    yval = (Y[y][x] >> 4) + 128
 *    cb   = (Cb[y >> 1][x >> 1] >> 4) clamped to -128 .. 127, cr likewise from Cr
 *    R, G, B, the pixel word of 16 and 32 bpp, the byte orders of 24 bpp, the blue that is not shifted and the doubling:
 *    libfiasco_amd_render.h, unchanged.
 *  That is: the bytes of the 4:4:4 renderer for the same Y plane with every chroma sample standing for its 2 x 2 pixels.
 *  The real reference writes exactly these bytes wherever it fills the surface in step with its planes
 *  (tests/golden/make_rendered_420.py asserts it), and, as in 4:4:4, reads past its tables where this code clamps.
 *
 *  Refused with a message (fiasco_get_error_message()), nothing written:
 *    an odd width or height (the reference's loops count pixel pairs and row pairs; fiasco_amd_magnified_size() never
 *    yields such a size for a 4:2:0 frame);
 *    24 bpp not doubled with a width that is not a multiple of 4: the reference's loops (lib/dither.c:831-931) count
 *    quadruples of a row and walk the chroma pointers by them, so its rows fall out of step with the arithmetic above
 *    (asserted by the fixture's generator on every frame of such a width: 34 x 4, 34 x 34, 38 x 70, 102 x 66);
 *    an empty frame or one beyond the library's size limit;
 *    what fiasco_amd_renderer_new() and fiasco_amd_batch_decode_device_420() refuse: in a batch a gray frame, a frame whose
 *    chroma the reference leaves zero and a smoothed state below level 1 fail alone.
 */
#ifndef LIBFIASCO_AMD_RENDER_420_H
#define LIBFIASCO_AMD_RENDER_420_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#include "libfiasco_amd_render.h"
#ifdef __cplusplus
extern "C" {
#endif

/* host code, no device needed ---------------------------------------------------------------------------------------- */

/* the size of the surface for a 4:2:0 frame of width x height and the bytes of a packed row; any of the three pointers may
 * be NULL.  1 ok / 0 + message where the shape is refused (above) */
int fiasco_amd_renderer_surface_size_420(const fiasco_amd_renderer_t *r, unsigned width, unsigned height, unsigned *out_width,
                                         unsigned *out_height, size_t *row_bytes);

/* the host restatement: planes y [height][width], cb and cr [height >> 1][width >> 1] int16 (12.4 fixed point) in host
 * memory into a packed surface of out_height * row_bytes bytes in host memory.  1 ok / 0 + message, nothing written */
int fiasco_amd_renderer_render_planes_420(const fiasco_amd_renderer_t *r, const int16_t *y, const int16_t *cb, const int16_t *cr,
                                          unsigned width, unsigned height, unsigned char *out);

/* the HIP library ---------------------------------------------------------------------------------------------------- */

/* the kernel alone: three packed planes in device memory into `surface'; runs on `stream' and waits for it on the host.
 * 1 ok / 0 + message, nothing written: the checks of fiasco_amd_planes_render_device(), applied to three planes, and the
 * size rule above */
int fiasco_amd_planes_render_device_420(const int16_t *y, const int16_t *cb, const int16_t *cr, unsigned width, unsigned height,
                                        const fiasco_amd_renderer_t *r, const fiasco_amd_device_surface *surface, void *stream);

/* The frames of the last finished pass decoded in 4:2:0 at `-m magnify -s smoothing' -- the jobs, smoothing passes and
 * per-frame refusals of fiasco_amd_batch_decode_device_420() -- and rendered: one launch of the rendering kernel per
 * flight.  surfaces[i] belongs to frame i and has the size fiasco_amd_renderer_surface_size_420() gives for the frame at
 * fiasco_amd_magnified_size(); data == NULL skips the frame.  Flights, the ordering against `stream' and the return value
 * (frames written, 0 + message when none) are those of fiasco_amd_batch_decode_device_shown(); a surface that fails its
 * checks refuses the call before anything is launched. */
int fiasco_amd_batch_decode_device_rendered_420(const fiasco_amd_batch_t *batch, const fiasco_amd_renderer_t *r, int magnify, int smoothing,
                                                const fiasco_amd_device_surface *surfaces, void *stream);

#ifdef __cplusplus
}
#endif
#endif
