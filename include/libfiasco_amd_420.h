/*
 *  libfiasco_amd_420.h -- decoded frames of a staged batch in 4:2:0, as NV12 / NV21 / I420 buffers in device memory
 *  (C ABI, plain types).
 *
 *  The reference's decoder has the mode (fiasco_d_options_set_4_2_0_format; codec/decoder.c:324-327, :463, :522, :792-838,
 *  :928).  It does not subsample a decoded frame: enlarge_image gives every state behind the root of the Y band one more
 *  step of reduction, and the chroma bands are decoded from the automaton at half the side length.  At magnification M
 *    a Y state       is shown at level coded + 2 M,     its x and y shifted by M
 *    a chroma state  is shown at level coded + 2 M - 2, its x and y shifted by M - 1
 *    max_level       the largest SHOWN level of a state with a linear combination (decode_image :455-457)
 *    the Y plane     W x H, the size of fiasco_amd_magnified_size() (always even), made of the Y states shown at max_level
 *    Cb, Cr          (W >> 1) x (H >> 1) (alloc_image, lib/image.c:209-211), made of the chroma states shown at max_level:
 *                    coded level max_level - 2 M + 2, two levels higher in the tree than the Y states (alloc_state_images
 *                    :918-937); all of them decoded at level max_level, placed at their shifted coordinates in planes of
 *                    half the pitch and cropped (:502-529)
 *  Unsmoothed, the Y plane is the 4:4:4 Y plane at M; the chroma planes are the 4:4:4 chroma planes at M - 1 wherever that
 *  magnification exists and has half the size, a crop of them where the halves were rounded up (102 x 66: 51 x 33 of 52 x 34),
 *  and exist where M - 1 is refused (48 x 70 at M = 0).
 *  Smoothing (smooth_image, :674-768) walks the SHIFTED automaton: the Y plane is blended along the Y borders at shift M and
 *  then along the Cb borders at shift M - 1 (x, y << (M - 1) or >> (1 - M), level + 2 M - 2), both against the full-size Y
 *  plane.  A smoothed 4:2:0 frame is therefore NOT the smoothed 4:4:4 frame with other chroma: its Y plane differs.
 *
 *  Refused with a message, the frame fails alone and nothing of it is reproduced:
 *    a gray frame;
 *    a frame whose chroma bands have no state at coded level max_level - 2 M + 2 because their roots lie below it: the
 *    reference points nothing at the chroma planes then and hands out calloc's zeros (a flat 64 x 64 colour image at
 *    `cfiasco' defaults: 0 of 1024 chroma samples non-zero) -- the message names max_level and the level of the chroma root;
 *    a band whose shown level would be clamped at 0 (level of the linear combinations below twice the reduction, the
 *    reduction of the chroma bands being one more);
 *    a smoothed state that falls below level 1 (libfiasco_amd_display.h), with the chroma shift for the Cb states.
 *  Intra frames of staged batches.  4:2:0 into display surfaces: libfiasco_amd_render_420.h.  Not built: RGB8 targets from
 *  4:2:0 planes, distortion in 4:2:0, P/B frames and the outputs of a video.  (The way back in, NV12 / NV21 / I420 input:
 *  libfiasco_amd_ycbcr.h.)
 */
#ifndef LIBFIASCO_AMD_420_H
#define LIBFIASCO_AMD_420_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Where a frame of width x height goes: 8-bit Y rows y_pitch bytes apart, and (width >> 1) x (height >> 1) chroma samples
 * in rows c_pitch bytes apart.  c_step 1: two planes, cb and cr (I420; YV12 is the same with the pointers swapped).  c_step
 * 2: ONE plane of interleaved pairs, cr == cb + 1 (NV12) or cb == cr + 1 (NV21); anything else is refused.  A pitch of 0
 * means packed (width; (width >> 1) * c_step).  y == NULL: the frame is skipped.  All of it is device memory and written. */
typedef struct fiasco_amd_device_target_420 {
    void *y;
    size_t y_pitch;
    void *cb, *cr;
    size_t c_pitch;
    unsigned c_step;
    unsigned width, height;
} fiasco_amd_device_target_420;

/* The frames of the batch's last finished pass in 4:2:0 at `magnify' and `smoothing' (-1: the value of each frame's stream
 * header, 0: none, 1 .. 100 per cent) into targets[i] (b->n entries).  Flights, the ordering against `stream', the return
 * value (frames written) and per-frame failure are those of fiasco_amd_batch_decode_device_shown() (libfiasco_amd_display.h).
 * Bytes: Y, Cb and Cr alike clip255((p >> 4) + 128) -- gray_write (lib/image.c:450-480) for Y, and the byte
 * fiasco_amd_batch_decode_psnr() and the distortion kernel compare a chroma plane as.
 * Refused with a message, nothing written: b == NULL, an empty batch, no targets, a smoothing out of range; a target with
 * a c_step other than 1 or 2, with c_step 2 and pointers that are not one byte apart, with a pitch below its row, of
 * another size than the frame's at `magnify' (the message names both), whose Y and chroma ranges overlap; no device; no
 * finished pass; a frame the size rule refuses at `magnify'; a target that is not device memory, whose rows leave their
 * allocation, or that lives on another device than the one the frame's share decodes on. */
int fiasco_amd_batch_decode_device_420(const fiasco_amd_batch_t *batch, int magnify, int smoothing,
                                       const fiasco_amd_device_target_420 *targets, void *stream);

/* The unsmoothed 12.4 planes of frame i in 4:2:0 at `magnify' on the host, packed: Y [H][W], Cb [H / 2][W / 2],
 * Cr [H / 2][W / 2] (W x H of fiasco_amd_magnified_size()): W * H * 3 / 2 values.  The refusals above that concern the
 * frame come first and need no device; a library whose decoder does not decode 4:2:0 (the test oracle's) is refused with
 * a message that names its backend.  1 ok / 0 + message. */
int fiasco_amd_batch_decode_planes_420(const fiasco_amd_batch_t *batch, unsigned i, int magnify, int16_t *out);

/* The borders the reference smooths the Y plane of the 4:2:0 frame along (host code: every build of the library): the Y
 * passes by ascending level at shift `magnify', then the Cb passes by ascending level at shift `magnify' - 1, all against
 * the size of fiasco_amd_magnified_size().  Checks, the 16-bit coordinate limit and the return value are those of
 * fiasco_amd_batch_smoothing_borders_magnified(); the frame's own refusals above apply. */
int fiasco_amd_batch_smoothing_borders_420(const fiasco_amd_batch_t *batch, unsigned i, int magnify, fiasco_amd_border *out, unsigned cap);

/* The conversion kernel alone, on `stream' itself: three packed planes of 12.4 values in device memory -- Y
 * [height][width], Cb and Cr [height >> 1][width >> 1] -- into `target'.  width, height: even, 2 .. 8192, and the
 * target's.  The call waits on the host.  1 ok / 0 + message. */
int fiasco_amd_planes_to_420_device(const int16_t *planes_y, const int16_t *planes_cb, const int16_t *planes_cr,
                                    unsigned width, unsigned height, const fiasco_amd_device_target_420 *target, void *stream);

#ifdef __cplusplus
}
#endif
#endif
