/*
 *  libfiasco_amd_render.h -- decoded frames in the pixel formats of a display: what the reference's viewer puts into its
 *  XImage (fiasco_renderer_new / fiasco_renderer_render, fiasco.h:283-296, lib/dither.c), restated on the host and as a
 *  kernel that writes surfaces in device memory (C ABI, plain types).
 *
 *  The names are this library's own: an application may link the reference library beside this one.
 *  They have a header of their own because the functions of the five older headers are pinned sets.
 *
 *  A renderer is the reference's: three colour masks, 16, 24 or 32 bits per pixel, optionally every pixel doubled in both
 *  directions.  The arithmetic is the reference's too (arithmetic shifts, HAVE_SIGNED_SHIFT):
 *    colour (4:4:4)  yval = (Y >> 4) + 128; cr, cb = (Cr >> 4), (Cb >> 4) clamped to -128 .. 127
 *                    R = yval + T_rr[cr], G = yval + T_rg[cr] + T_bg[cb], B = yval + T_bb[cb]
 *                    T_x[v] = (int) (k * v + 0.5) in double, k = 1.4022, -0.7145, -0.3456, 1.7710   (lib/dither.c:151-159)
 *    gray            R = G = B = (p >> 4) + 128
 *    16, 32 bpp      with c = clip to 0 .. 255, n_x the bits set in a mask and s_x the zero bits below it
 *                    pixel = ((c(R) >> (8 - n_r)) << s_r) | ((c(G) >> (8 - n_g)) << s_g) | (c(B) >> (8 - n_b))
 *                    stored as a little-endian 16-bit or 32-bit value.
 *                    BLUE IS NOT SHIFTED: the reference shifts the entry of its blue table before it assigns it
 *                    (lib/dither.c:205-208), so the shift is lost.  With the blue mask lowest (565, 555, XRGB8888) that is
 *                    what one expects; with blue high it is what the reference writes, and it is reproduced here.
 *    24 bpp          three bytes per pixel, c(R), c(G), c(B) in memory order when red_mask > green_mask, else c(B), c(G),
 *                    c(R) (lib/dither.c:123-127); rows tightly packed.
 *    doubled         every pixel twice in its row, every row twice: a surface of 2 W x 2 H.
 *  The reference reads finite tables (its pixel tables span -1024 .. 1279, its chroma tables -1152 .. 1151, the clip table
 *  of 24 bpp -256 .. 511) and reads past them where an index leaves them; this code clamps.  Inside the tables the two agree.
 *
 *  Refused with a message (fiasco_get_error_message()), nothing written:
 *    fiasco_amd_renderer_new       a depth other than 16, 24 or 32 ("Rendering depth of XImage must be 16, 24, or 32 bpp.");
 *                                  a mask that is zero, not contiguous, wider than 8 bits or outside `bpp' bits (the
 *                                  reference shifts by a negative or word-sized count there)
 *    sizes (every entry)           shapes where the reference's loops do not fill the surface: 24 bpp not doubled with
 *                                  width * height not a multiple of 4; 24 bpp doubled with an odd width; 16 bpp gray not
 *                                  doubled with an odd width * height; an empty frame or one beyond the library's size limit
 *  4:2:0 images, what the reference's viewer renders on a screen: libfiasco_amd_render_420.h.
 */
#ifndef LIBFIASCO_AMD_RENDER_H
#define LIBFIASCO_AMD_RENDER_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* immutable after fiasco_amd_renderer_new(): threads may share one */
typedef struct fiasco_amd_renderer fiasco_amd_renderer_t;

/* a surface in device memory.  pitch: bytes from row to row, 0 = packed; a pitch above the row leaves the bytes between
 * two rows alone.  width, height: what fiasco_amd_renderer_surface_size() gives for the frame.  data: aligned to the
 * pixel size at 16 and 32 bpp (and the pitch a multiple of it); NULL in a batch call: the frame is skipped */
typedef struct fiasco_amd_device_surface {
    void    *data;
    size_t   pitch;
    unsigned width, height;
} fiasco_amd_device_surface;

/* host code, no device needed ---------------------------------------------------------------------------------------- */

/* NULL + message where refused (above) */
fiasco_amd_renderer_t *fiasco_amd_renderer_new(unsigned long red_mask, unsigned long green_mask, unsigned long blue_mask, unsigned bpp,
                                               int double_resolution);
void fiasco_amd_renderer_delete(fiasco_amd_renderer_t *r);

/* the size of the surface for a frame of width x height (color: 0 gray, else colour) and the bytes of a packed row; any
 * of the three pointers may be NULL.  1 ok / 0 + message where the shape is refused (above) */
int fiasco_amd_renderer_surface_size(const fiasco_amd_renderer_t *r, unsigned width, unsigned height, int color, unsigned *out_width,
                                     unsigned *out_height, size_t *row_bytes);

/* the host restatement: planes [bands][height][width] int16 (12.4 fixed point; 1 band gray, 3 bands Y, Cb, Cr) in host
 * memory into a packed surface of out_height * row_bytes bytes in host memory.  1 ok / 0 + message, nothing written */
int fiasco_amd_renderer_render_planes(const fiasco_amd_renderer_t *r, const int16_t *planes, int color, unsigned width, unsigned height,
                                      unsigned char *out);

/* the HIP library ---------------------------------------------------------------------------------------------------- */

/* the kernel alone: packed planes in device memory (H x W, or 3 x H x W for Y, Cb, Cr) of a frame of width x height into
 * `surface'; runs on `stream' and waits for it on the host.  1 ok / 0 + message, nothing written: planes or surface not in
 * device memory, not on one device or beyond their allocation; a surface of another size than
 * fiasco_amd_renderer_surface_size() gives; a pitch below the row; data or pitch not aligned to the pixel */
int fiasco_amd_planes_render_device(const int16_t *planes, int color, unsigned width, unsigned height, const fiasco_amd_renderer_t *r,
                                    const fiasco_amd_device_surface *surface, void *stream);

/* The frames of the last finished pass as the reference's viewer puts them on the screen at `-m magnify -s smoothing':
 * fiasco_amd_batch_decode_device_shown() (libfiasco_amd_display.h: the same flights, magnification, smoothing passes,
 * per-frame refusals and ordering against `stream') with one launch of the rendering kernel per flight where that entry
 * converts to 8-bit pixels.  surfaces[i] belongs to frame i and has the size fiasco_amd_renderer_surface_size() gives for
 * the frame at fiasco_amd_magnified_size(); data == NULL skips the frame.  Returns the number of frames written, 0 +
 * message when none; a surface that fails its checks refuses the call before anything is launched. */
int fiasco_amd_batch_decode_device_rendered(const fiasco_amd_batch_t *b, const fiasco_amd_renderer_t *r, int magnify, int smoothing,
                                            const fiasco_amd_device_surface *surfaces, void *stream);

#ifdef __cplusplus
}
#endif
#endif
