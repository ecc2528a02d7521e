/*
 *  libfiasco_amd_stream.h -- .fco streams read back: the reader, the frames of a stream written again, and -- HIP library
 *  only -- its frames decoded on the device as `dfiasco' writes them, video frames included (C ABI, plain types).
 *
 *  open, open_file, free, get_info, frame_type, coding_order, rewrite and smoothing_borders are host C; the decode entries
 *  need the HIP core.  They have a header of their own because the functions of libfiasco_amd.h and libfiasco_amd_hip.h
 *  are a pinned set.  All return 1 / non-NULL (or a count) on success, 0 / NULL + fiasco_get_error_message() otherwise.
 */
#ifndef LIBFIASCO_AMD_STREAM_H
#define LIBFIASCO_AMD_STREAM_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#include "libfiasco_amd_420.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fiasco_amd_stream fiasco_amd_stream_t;

/* The stream in `data' (len bytes; not kept) or in file `name' (looked up like every FIASCO file: the directory given,
 * then FIASCO_DATA).  Open parses EVERYTHING: the header, the basis the header names, and every frame into an automaton
 * of its own.  A stream is untrusted input: every read is checked against the buffer and every index a decoder follows
 * is validated before open returns; nothing that fails reaches the device.  Refused with a message: a wrong magic or
 * file format release; truncation anywhere; a tiling flag of 1 (no coder writes it); a basis that cannot be loaded; a
 * symbol outside its alphabet; a tree, an edge, a level, a vector or a frame number no coder can have written.
 * Half-pixel streams are read; decoding them is refused. */
fiasco_amd_stream_t *fiasco_amd_stream_open(const unsigned char *data, size_t len);
fiasco_amd_stream_t *fiasco_amd_stream_open_file(const char *name);
void fiasco_amd_stream_free(fiasco_amd_stream_t *stream);

/* What the header says.  The strings belong to the stream */
typedef struct fiasco_amd_stream_info {
    unsigned    width, height;
    int         color;
    unsigned    frames, fps;
    unsigned    smoothing;                    /* the header's percentage: what `dfiasco' smooths with when no -s is given */
    const char *title, *comment, *basis_name;
    unsigned    rpf_mantissa, dc_rpf_mantissa, d_rpf_mantissa, d_dc_rpf_mantissa;
    int         B_as_past_ref;
    int         half_pixel;
} fiasco_amd_stream_info;
int fiasco_amd_stream_get_info(const fiasco_amd_stream_t *stream, fiasco_amd_stream_info *info);

/* type of display frame `display': 0 I, 1 P, 2 B; -1 + message when there is no such frame */
int fiasco_amd_stream_frame_type(const fiasco_amd_stream_t *stream, unsigned display);
/* the display numbers in the order the frames are coded in; returns their number (order may be NULL: count only) */
int fiasco_amd_stream_coding_order(const fiasco_amd_stream_t *stream, unsigned *order, unsigned cap);

/* Every frame through the writer again (free with fiasco_amd_free): for a stream one of the coders wrote, the bytes
 * that were opened.  The round trip that pins reader and writer against each other, and a re-mux. */
int fiasco_amd_stream_rewrite(const fiasco_amd_stream_t *stream, unsigned char **out, size_t *out_len);

/* The borders `dfiasco -m magnify' smooths display frame `display' along -- those of the frame's own automaton, whatever
 * its type --, as fiasco_amd_batch_smoothing_borders_magnified() lists them, or fiasco_amd_batch_smoothing_borders_420()
 * with format_420 != 0.  Returns their number (out may be NULL: count only); 0 + message as those do. */
int fiasco_amd_stream_smoothing_borders(const fiasco_amd_stream_t *stream, unsigned display, int magnify, int format_420,
                                        fiasco_amd_border *out, unsigned cap);

/* Display frames first .. first + count - 1 into targets[0 .. count - 1] (data == NULL: not this frame), the bytes
 * `dfiasco -m magnify -s smoothing -o' writes for them: decoded on the device at that magnification, P and B frames
 * predicted from the UNSMOOTHED frames before them at the same magnification, smoothed along the borders of their own
 * automaton.  smoothing: -1 the header's value, 0 none, 1 .. 100 per cent.  The frames the wanted ones are predicted
 * from are decoded on the way.  Target validation, stream ordering and the size rule are those of
 * fiasco_amd_batch_decode_device_shown(); a stream decodes on ONE device share, where its targets must live.  Returns
 * the number of frames written.  A frame that fails leaves its target alone and takes the frames predicted from it
 * along; the message names the first such frame and the cause. */
int fiasco_amd_stream_decode_device(const fiasco_amd_stream_t *stream, unsigned first, unsigned count, int magnify, int smoothing,
                                    const fiasco_amd_device_target *targets, void *hip_stream);
/* the same in 4:2:0, into NV12 / NV21 / I420 buffers as fiasco_amd_batch_decode_device_420() writes them: the reference
 * frames are 4:2:0 frames too, the vectors of the chroma bands halved toward zero (restore_mc, codec/motion.c:51) */
int fiasco_amd_stream_decode_device_420(const fiasco_amd_stream_t *stream, unsigned first, unsigned count, int magnify, int smoothing,
                                        const fiasco_amd_device_target_420 *targets, void *hip_stream);

/* The unsmoothed planes of display frame `display' at `magnify' on the host, 12.4 fixed point: all bands back to back
 * at the size of fiasco_amd_magnified_size(); _420: Y at that size, then Cb and Cr of (width >> 1) x (height >> 1)
 * values.  The reference frames are decoded on the way. */
int fiasco_amd_stream_decode_planes(const fiasco_amd_stream_t *stream, unsigned display, int magnify, int16_t *out);
int fiasco_amd_stream_decode_planes_420(const fiasco_amd_stream_t *stream, unsigned display, int magnify, int16_t *out);

#ifdef __cplusplus
}
#endif
#endif
