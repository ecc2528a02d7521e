/*
 *  libfiasco_amd_decoder.h -- the decoder half of fiasco.h on the device: fiasco_d_options_*, fiasco_decoder_*,
 *  fiasco_image_* and fiasco_renderer_*, with the structures of fiasco.h (C ABI), and this library's extensions around
 *  them (fiasco_amd_*).  With libfiasco_amd.h, which holds the coder half, this is the whole of fiasco.h.
 *
 *  The functions have a header of their own because those of the older headers are pinned sets.  The structures have the
 *  members of fiasco.h in its order and with its types; `delete' and `private' are spelled `delete_' and `private_', as
 *  in libfiasco_amd.h.  Every method pointer is filled in.  Messages come through fiasco_get_error_message().
 *
 *  Behaviour is the reference's (codec/dfiasco.c, codec/options.c, codec/decoder.c, lib/image.c, lib/dither.c):
 *    options       smoothing 70, magnification 0, 4:4:4; set_smoothing accepts -1 .. 100
 *    decoder_new   reads and validates the WHOLE stream (libfiasco_amd_stream.h: host code, no device needed); "-" or NULL
 *                  reads stdin; the two magnification limits with the reference's sentences
 *    get_width,    of the frames shown: the coded size shifted by the magnification, rounded up to even
 *    get_height
 *    write_frame   the next display frame decoded in 4:4:4 whatever the options say, as a raw PGM / PPM through
 *                  open_file(name, "FIASCO_IMAGES", ..); "-" or NULL: stdout
 *    get_frame     the next display frame in the format of the options, as an image
 *    image_new     a raw PGM / PPM file as an image (the PNM reader of the coder: even sides of at least 32 pixels)
 *    renderer      fiasco_amd_renderer_* of libfiasco_amd_render.h and libfiasco_amd_render_420.h behind the reference's
 *                  names: the arithmetic, the unshifted blue and the refusals are described there
 *    get_height    of an image: the WIDTH, as the reference returns it (lib/image.c:127-135); the height:
 *                  fiasco_amd_image_get_height()
 *  Where this library differs:
 *    Everything is decoded on the device, by the kernels of the stream entries (libfiasco_amd_stream.h).  What those refuse is
 *    refused here with the same message and nothing is reproduced on the CPU: half-pixel streams, tiling streams, the
 *    reductions and smoothed levels DESIGN.md 7 names, 4:2:0 frames whose chroma the reference leaves zero, a first frame
 *    that is a P or B frame, and the masks and surface shapes fiasco_amd_renderer_* refuses.  Without a usable device
 *    get_frame and write_frame fail with the library's no-device message; everything else works.
 *    get_frame on a gray stream with the 4:2:0 option set is refused ("a gray frame has no chroma bands", as the stream
 *    entries refuse it): the reference shrinks every state of such an automaton by a level, its initial basis included
 *    (enlarge_image, codec/decoder.c:796-800), and hands out a frame that is neither (tests/golden/DECODER_API.json records
 *    its md5).  write_frame, which decodes 4:4:4, works.
 *    A decoder whose calls alternate between get_frame in 4:2:0 and write_frame decodes the frames the second format
 *    needs again: reference frames live in ONE format (the reference mixes them).
 *
 *  A display frame that fails is consumed: the next call goes on with the next display frame, and the frames predicted from
 *  the failed one fail with a message that names it.  A call behind the last frame fails with "no such frame".
 *
 *  One decoder is used by one thread at a time; several decoders may run on several threads (the threading contract of
 *  INTEGRATION.md covers the device shares under them).  An image may outlive its decoder.
 */
#ifndef LIBFIASCO_AMD_DECODER_H
#define LIBFIASCO_AMD_DECODER_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#include "libfiasco_amd_render.h"
#include "libfiasco_amd_render_420.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- fiasco.h:101-108 ---- */
typedef struct fiasco_image {
    void     (*delete_)(struct fiasco_image *image);
    unsigned (*get_width)(struct fiasco_image *image);
    unsigned (*get_height)(struct fiasco_image *image);
    int      (*is_color)(struct fiasco_image *image);
    void *private_;
} fiasco_image_t;

/* ---- fiasco.h:113-127 ---- */
typedef struct fiasco_decoder {
    int             (*delete_)(struct fiasco_decoder *decoder);
    int             (*write_frame)(struct fiasco_decoder *decoder, const char *filename);
    fiasco_image_t *(*get_frame)(struct fiasco_decoder *decoder);
    unsigned        (*get_length)(struct fiasco_decoder *decoder);
    unsigned        (*get_rate)(struct fiasco_decoder *decoder);
    unsigned        (*get_width)(struct fiasco_decoder *decoder);
    unsigned        (*get_height)(struct fiasco_decoder *decoder);
    const char     *(*get_title)(struct fiasco_decoder *decoder);
    const char     *(*get_comment)(struct fiasco_decoder *decoder);
    int             (*is_color)(struct fiasco_decoder *decoder);
    void *private_;
} fiasco_decoder_t;

/* ---- fiasco.h:179-189 ---- */
typedef struct fiasco_d_options {
    void (*delete_)(struct fiasco_d_options *options);
    int  (*set_smoothing)(struct fiasco_d_options *options, int smoothing);
    int  (*set_magnification)(struct fiasco_d_options *options, int level);
    int  (*set_4_2_0_format)(struct fiasco_d_options *options, int format);
    void *private_;
} fiasco_d_options_t;

/* ---- fiasco.h:196-203 ---- */
typedef struct fiasco_renderer {
    int  (*render)(const struct fiasco_renderer *this_, unsigned char *data, const fiasco_image_t *fiasco_image);
    void (*delete_)(struct fiasco_renderer *this_);
    void *private_;
} fiasco_renderer_t;

/* ---- decoder options (fiasco.h:405-421) ---- */
fiasco_d_options_t *fiasco_d_options_new(void);
void fiasco_d_options_delete(fiasco_d_options_t *options);
int fiasco_d_options_set_smoothing(fiasco_d_options_t *options, int smoothing);
int fiasco_d_options_set_magnification(fiasco_d_options_t *options, int level);
int fiasco_d_options_set_4_2_0_format(fiasco_d_options_t *options, int format);

/* ---- decoder (fiasco.h:223-257) ---- */
fiasco_decoder_t *fiasco_decoder_new(const char *filename, const fiasco_d_options_t *options);
int fiasco_decoder_delete(fiasco_decoder_t *decoder);
int fiasco_decoder_write_frame(fiasco_decoder_t *decoder, const char *filename);
fiasco_image_t *fiasco_decoder_get_frame(fiasco_decoder_t *decoder);
unsigned fiasco_decoder_get_width(fiasco_decoder_t *decoder);
unsigned fiasco_decoder_get_height(fiasco_decoder_t *decoder);
int fiasco_decoder_is_color(fiasco_decoder_t *decoder);
unsigned fiasco_decoder_get_rate(fiasco_decoder_t *decoder);
unsigned fiasco_decoder_get_length(fiasco_decoder_t *decoder);
const char *fiasco_decoder_get_title(fiasco_decoder_t *decoder);
const char *fiasco_decoder_get_comment(fiasco_decoder_t *decoder);

/* ---- images (fiasco.h:264-276) ---- */
fiasco_image_t *fiasco_image_new(const char *filename);
void fiasco_image_delete(fiasco_image_t *image);
unsigned fiasco_image_get_width(fiasco_image_t *image);
unsigned fiasco_image_get_height(fiasco_image_t *image);
int fiasco_image_is_color(fiasco_image_t *image);

/* ---- renderer (fiasco.h:283-296).  render: an image from get_frame is rendered on the device, by the kernels of
 *      fiasco_amd_planes_render_device[_420](), into a staging surface the renderer keeps, and copied to `ximage' (packed,
 *      out_height * row_bytes bytes of fiasco_amd_renderer_surface_size[_420]()); an image from fiasco_image_new that was
 *      never asked for its device planes runs the host loops ---- */
fiasco_renderer_t *fiasco_renderer_new(unsigned long red_mask, unsigned long green_mask, unsigned long blue_mask, unsigned bpp,
                                       int double_resolution);
void fiasco_renderer_delete(fiasco_renderer_t *renderer);
int fiasco_renderer_render(const fiasco_renderer_t *renderer, unsigned char *ximage, const fiasco_image_t *fiasco_image);

/* ---- extensions ---- */

/* a decoder over a stream in memory (len bytes, not kept) */
fiasco_decoder_t *fiasco_amd_decoder_new_memory(const unsigned char *data, size_t len, const fiasco_d_options_t *options);
/* How many display frames one call may decode: a call for display frame d decodes d, what it is predicted from, and the
 * display frames up to d + n - 1 whose flights can go along; the following calls hand those out without device work.  Every
 * coded frame is decoded once per decoder.  The default is 32, one flight of the decoder; 1: strictly one display frame
 * per call (and the frames it needs).  n == 0 is refused.  What was decoded ahead stays decoded.  The decoder keeps its HIP
 * stream, events and arena from its first call to its end, and takes the buffers of images that were deleted for the frames
 * to come: at a steady pace a call allocates nothing */
int fiasco_amd_decoder_set_read_ahead(fiasco_decoder_t *decoder, unsigned n);
/* the display frames consumed so far: handed out, written, or failed (a call that is refused as a whole -- no device, past
 * the end, 4:2:0 on a gray stream, a stream the walk refuses -- consumes nothing); -1 + message for what is no decoder */
int fiasco_amd_decoder_position(const fiasco_decoder_t *decoder);
/* the height of the image (fiasco_image_get_height() returns the width, as the reference does); 0 + message */
unsigned fiasco_amd_image_get_height(const fiasco_image_t *image);
/* 0: 4:4:4 (and gray), 1: 4:2:0; -1 + message for what is no image */
int fiasco_amd_image_format(const fiasco_image_t *image);
/* the 12.4 planes of the image on the host, in the layout of fiasco_amd_stream_decode_planes[_420]() (libfiasco_amd_stream.h):
 * all bands back to back; 4:2:0: Y, then Cb and Cr of (width >> 1) x (height >> 1) values.  For a decoded frame these are
 * the planes the reference's fiasco_decoder_get_frame() hands out, smoothed where smoothing applies */
int fiasco_amd_image_planes(const fiasco_image_t *image, int16_t *out);
/* the same planes where they live: planes[b] in device memory on *device (planes[1], planes[2]: NULL for a gray image).
 * For a decoded frame they are complete since get_frame returned; an image from fiasco_image_new is uploaded by the first
 * call.  The memory belongs to the image, and goes back to its decoder when the image is deleted: a later frame is decoded
 * into it, on the decoder's own stream.  Work the caller queued on the planes -- kernels or copies on streams of its own --
 * must have COMPLETED before fiasco_image_delete(); deleting does not wait for it */
int fiasco_amd_image_planes_device(const fiasco_image_t *image, const int16_t *planes[3], int *device);
/* fiasco_renderer_render() into a surface in device memory (libfiasco_amd_render.h: its size, pitch and alignment rules),
 * on hip_stream, by fiasco_amd_planes_render_device[_420]() and with its ordering: behind what the stream holds, and
 * complete when the call returns */
int fiasco_amd_renderer_render_device(const fiasco_renderer_t *renderer, const fiasco_amd_device_surface *surface, const fiasco_image_t *image,
                                      void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
