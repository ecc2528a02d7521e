/*
 *  libfiasco_amd_display.h -- decoded frames of a staged batch as `dfiasco' SHOWS them at every magnification: magnified
 *  frames and thumbnails smoothed along the borders of their partition, on the device (C ABI, plain types).
 *
 *  `dfiasco -m M' smooths the frame it shows at every M: get_next_frame (codec/decoder.c:317-377) lets enlarge_image
 *  shift x, y and the level of every state, decodes, and smooth_image walks the shifted automaton.  The entries here are
 *  the siblings of fiasco_amd_batch_decode_device_magnified() / _thumbnails() (libfiasco_amd_hip.h) and of the smoothed
 *  entries (libfiasco_amd_smooth.h) that do both.  They have a header of their own because the functions of the four
 *  older headers are pinned sets.  All return what their siblings return, 0 + fiasco_get_error_message() on failure.
 *
 *  The border list at magnification M is the coded list (fiasco_amd_batch_smoothing_borders(), libfiasco_amd.h) with
 *  x and y shifted by M, the level raised by 2 M, the length the side of the new level clipped at the size of
 *  fiasco_amd_magnified_size(); a border that begins outside that size is left out.  Passes in the coded order: Y by
 *  ascending level, then Cb by ascending level.  That is the reference's plane as long as every listed state keeps a
 *  level of at least 1.  A state of level <= 2 k at reduction k falls to level 0: enlarge_image clamps the level and floors
 *  the coordinates, the cut lands on the block's own edge, borders of a pass share pixels, and at (0, 0) smooth_image reads
 *  and writes the word before the plane.  The reference's own result is undefined there; such a frame is REFUSED with a
 *  message that names the magnification and the level.  States of `cfiasco' defaults have level >= 7 (every reduction down
 *  to -3 is smoothed), those of -z 1 .. 3 level >= 5 (down to -2).
 */
#ifndef LIBFIASCO_AMD_DISPLAY_H
#define LIBFIASCO_AMD_DISPLAY_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fiasco_amd_batch_smoothing_borders() of frame i as `dfiasco -m magnify' shows it (host code: every build of the
 * library).  magnify == 0: exactly the coded list.  Returns the number of borders (out may be NULL: count only); 0 +
 * message: no finished intra automaton, more than cap, a magnification the size rule refuses (its message), or a frame with
 * a listed state whose shifted level is below 1. */
int fiasco_amd_batch_smoothing_borders_magnified(const fiasco_amd_batch_t *batch, unsigned i, int magnify, fiasco_amd_border *out, unsigned cap);

/* The bytes `dfiasco -m magnify -s smoothing -o' writes, in device memory: fiasco_amd_batch_decode_device_magnified() with
 * the smoothing step of fiasco_amd_batch_decode_device_smoothed() behind the decoder's kernels.  smoothing: -1 the value of
 * each frame's own stream header (what `dfiasco -m magnify -o' shows), 0 none, 1 .. 100 per cent.  Every target has the
 * size of fiasco_amd_magnified_size().  A frame that cannot be smoothed at `magnify' fails alone, before anything of its
 * flight is uploaded; the others are written (the return value counts them, the message names the frame). */
int fiasco_amd_batch_decode_device_shown(const fiasco_amd_batch_t *b, int magnify, int smoothing, const fiasco_amd_device_target *targets, void *stream);

/* fiasco_amd_batch_decode_device_thumbnails() with both outputs smoothed: the frame along the coded list, the thumbnail
 * along the list at -reduce, from ONE decode.  The frame has the bytes of fiasco_amd_batch_decode_device_smoothed(), the
 * thumbnail those of fiasco_amd_batch_decode_device_shown(b, -reduce, smoothing, ...).  A frame whose thumbnail cannot be
 * smoothed fails alone: neither of its two targets is written. */
int fiasco_amd_batch_decode_device_thumbnails_shown(const fiasco_amd_batch_t *b, int smoothing, const fiasco_amd_device_target *targets, unsigned reduce,
                                                    const fiasco_amd_device_target *thumbs, void *stream);

/* fiasco_amd_smooth_planes_device() (libfiasco_amd_smooth.h: same arguments, rules and refusals) through the FUSED
 * kernel: one launch, one workgroup that runs every pass of the plane with a barrier between two passes, where the
 * sibling launches once per pass.  Whatever fiasco_amd_smooth_fused() says.  Same result. */
int fiasco_amd_smooth_planes_device_fused(int16_t *y_plane, unsigned width, unsigned height, const fiasco_amd_border *borders, unsigned n,
                                          int smoothing, void *stream);

/* Which smoothed planes of a decoder flight take the fused kernel: a pure function of what the check of a border list
 * counts -- its pixel pairs and its passes.  1: one launch for all passes of the plane; 0: one launch per pass, shared
 * with the other planes of the flight.  Monotone in `pairs' (DESIGN.md 3 has the measurement behind the threshold). */
int fiasco_amd_smooth_fused(unsigned long long pairs, unsigned npasses);

#ifdef __cplusplus
}
#endif
#endif
