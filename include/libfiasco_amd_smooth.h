/*
 *  libfiasco_amd_smooth.h -- decoded frames of a staged batch as the reference's decoder DISPLAYS them: smoothed along
 *  the borders of their partition, on the device (HIP library only; C ABI, plain types).
 *
 *  The entries are the smoothed siblings of fiasco_amd_batch_decode_device(),
 *  fiasco_amd_batch_decode_distortion_device() and fiasco_amd_planes_to_pixels_device() (libfiasco_amd_hip.h).  They have
 *  a header of their own because the functions of libfiasco_amd.h and libfiasco_amd_hip.h are a pinned set, as those of
 *  libfiasco_amd_video.h are.  All return what their siblings return, 0 + fiasco_get_error_message() on failure.
 */
#ifndef LIBFIASCO_AMD_SMOOTH_H
#define LIBFIASCO_AMD_SMOOTH_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Smoothing: `dfiasco' shows no frame as `-s 0' decodes it.  It blends the luminance plane along every border of the
 * partition (smooth_image, codec/decoder.c:674-768; the borders: fiasco_amd_batch_smoothing_borders(), libfiasco_amd.h)
 * with the percentage of `-s N' or, without -s, of the stream header (70 from a default options object).  Here that
 * step runs on the device between the decoder's kernels and their consumers (csrc/hip/smooth.inc): one launch per pass
 * of the border list for all frames of a decoder flight.  The pixels written and the distortion measured are then those
 * of the frame the reference's decoder displays.
 *   smoothing     -1: every frame at the value of its own stream header; 0: none -- the bytes and sums of the
 *                 unsmoothed siblings; 1 .. 100: that percentage.  Anything else is refused.
 * fiasco_amd_batch_decode_device_smoothed(), fiasco_amd_batch_decode_distortion_device_smoothed(): every rule, refusal
 * and return value of fiasco_amd_batch_decode_device() / fiasco_amd_batch_decode_distortion_device().  Intra frames at
 * the coded size; the frames of a video are not smoothed, magnified frames and thumbnails are libfiasco_amd_display.h's. */
int fiasco_amd_batch_decode_device_smoothed(const fiasco_amd_batch_t *b, int smoothing, const fiasco_amd_device_target *targets, void *stream);
int fiasco_amd_batch_decode_distortion_device_smoothed(const fiasco_amd_batch_t *b, int smoothing, unsigned long long *sse, unsigned *maxdiff,
                                                       const fiasco_amd_device_target *targets, void *stream);
/* the step alone, on `stream' itself: y_plane [height][width] int16 (12.4 fixed point) in device memory is changed in
 * place along `borders' (n entries in host memory, in the order and with the pass numbering of
 * fiasco_amd_batch_smoothing_borders()); smoothing 0 .. 100 (0 and an empty list change nothing).  The call waits on
 * the host.  1 ok / 0 + message.  Refused with a message, nothing written: a plane that is not device memory or
 * leaves its allocation; width or height outside 1 .. 8192; smoothing out of range; a border that leaves the plane
 * (odd level: 1 <= y < height, x + len <= width; even level: 1 <= x < width, y + len <= height), is empty or longer than
 * the side of its level; passes that do not ascend from 0 without gaps; two levels in one pass. */
int fiasco_amd_smooth_planes_device(int16_t *y_plane, unsigned width, unsigned height, const fiasco_amd_border *borders, unsigned n,
                                    int smoothing, void *stream);

#ifdef __cplusplus
}
#endif
#endif
