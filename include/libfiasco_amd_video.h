/*
 *  libfiasco_amd_video.h -- videos beyond fiasco_coder(): the whole stream of a sequence in one call, the coder's
 *  reconstructed frames on the host, and -- HIP library only -- videos whose frames lie in device memory, with every
 *  reconstructed frame and its exact distortion delivered back into device memory (C ABI, plain types).
 *
 *  The first three entries are host C and exist in every build of the library; the two device entries exist where the
 *  HIP core is linked.  All return 1 / non-NULL on success, 0 / NULL + fiasco_get_error_message() otherwise.
 */
#ifndef LIBFIASCO_AMD_VIDEO_H
#define LIBFIASCO_AMD_VIDEO_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#include "libfiasco_amd_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Everything in one process (world == 1): probe, search with speculation until every GOP started from what the GOP
 * before it left, the flags resolved, the frames written -- the whole stream with its header, the bytes fiasco_coder()
 * writes into its file, in memory (free with fiasco_amd_free).  For callers whose frames have no file names (sequences
 * opened from memory, or from device memory: libfiasco_amd_hip.h). */
int      fiasco_amd_seq_encode(fiasco_amd_seq_t *seq, unsigned char **out, size_t *out_len);
/* The coder's own reconstruction of every frame: decode_image + restore_mc (codec/coder.c:647-651), the frame the next
 * P or B frame is predicted from.  Its yardstick is the reference CODER's planes, not dfiasco's output: `dfiasco -s 0'
 * shows the same pixels only at the default mantissas 3 / 5.  keep != 0: from now on every search
 * reconstructs every frame of the GOPs it searches -- B frames, the last frame of a GOP and the frames of an all-intra
 * sequence included, which a search otherwise skips -- and keeps its planes on the host; keep == 0 drops them.
 * fiasco_amd_seq_reconstructed_planes(): the planes of display frame `display', all bands back to back (width * height
 * int16 each, 12.4 fixed point; gray: one band), and its frame type (0 I, 1 P, 2 B; may be NULL) -- the sibling of
 * fiasco_amd_batch_decode_planes() for videos.  Refused with a message: keep not set, a frame whose GOP this process
 * has not searched.  A GOP that is searched again overwrites its frames: after the last search they belong to the
 * stream that is written. */
int      fiasco_amd_seq_keep_reconstructed(fiasco_amd_seq_t *seq, int keep);
int      fiasco_amd_seq_reconstructed_planes(const fiasco_amd_seq_t *seq, unsigned display, int16_t *out, int *frame_type);

/* Videos in device memory.  fiasco_amd_seq_open_device() is fiasco_amd_seq_open() (libfiasco_amd.h) without PNM: the
 * frames of a video in DISPLAY order where a decoder or renderer left them, with the layouts, pitch and plane stride of
 * fiasco_amd_batch_stage_device().  The handle works with every fiasco_amd_seq_* call and with fiasco_amd_seq_free().
 * Open converts ONCE every frame this rank will ever search -- the frames of its groups of pictures (gop % world ==
 * rank) and display frame 0, which the probe searches on every rank -- into the coder's int16 12.4 planes, in a buffer
 * the sequence owns on the device of the share that searches the frame's GOP: one launch of the conversion kernel per
 * share.  The buffer takes frames x bands x width x height x 2 bytes.  The searches read the planes in place; no host
 * planes exist unless somebody asks for them.
 *   stream        as fiasco_amd_batch_stage_device().  Open waits on the host for its conversions (it is not a hot
 *                 call) and makes `stream' wait for them too: the caller may overwrite or free the sources right
 *                 after the call.
 * Refused with a message, nothing allocated: n == 0; no HIP device; every refusal of a frame that
 * fiasco_amd_batch_stage_device() knows; frames of different sizes or colour models (the sequence engine's messages:
 * "all images of a sequence have to be of the same size."); no room in HBM ("out of HBM"); a frame on a device other
 * than the one its GOP is searched on (no peer copy on this path). */
fiasco_amd_seq_t *fiasco_amd_seq_open_device(unsigned n, const fiasco_amd_device_frame *frames, void *stream,
                                             float quality, const fiasco_c_options_t *options,
                                             unsigned rank, unsigned world);

/* The way back for videos: every reconstructed frame as 8-bit pixels in device memory, and its exact distortion.  While
 * outputs are set, every search (fiasco_amd_seq_search, fiasco_amd_seq_encode) reconstructs EVERY frame of the GOPs it
 * searches -- B frames, the last frame of a GOP and the frames of an all-intra sequence included, which a search
 * otherwise skips -- and the decoder flights that run anyway deliver, for display frame i:
 *   targets[i]    the pixels, by the conversion kernel of fiasco_amd_batch_decode_device() (same layouts and bytes);
 *   sse, maxdiff  per band the exact integer sum of squared differences and the largest absolute difference between the
 *                 reconstruction and the frame's original planes, both as the bytes clip255((p >> 4) + 128): the rules
 *                 of fiasco_amd_batch_decode_distortion_device().  The original of a device-fed frame is read where
 *                 open left it; the original of a PNM-fed frame is copied into the flight's arena;
 *   written[i]    0 when a search of the frame's GOP begins, 1 when its outputs have been delivered, 0 when the GOP failed.
 * A GOP that is searched again (the speculated minimum level of a colour stream was wrong) overwrites its frames: what is
 * in the arrays after the last search belongs to the stream that is written.  GOPs of other ranks are never touched.
 * WHAT THESE FRAMES ARE: the coder's own reconstruction (decode_image + restore_mc, codec/coder.c:647-651), the frame
 * the next P or B frame is predicted from.  Their yardstick is the reference CODER's planes; `dfiasco -s 0' shows the
 * same pixels only at the default mantissas 3 / 5.
 * The arrays are borrowed until they are replaced or the sequence is freed.  Every target is validated at the call as
 * fiasco_amd_batch_decode_device() validates it -- device memory, rows inside the allocation, pitch, size, layout against
 * colour model, the device of the share that decodes the frame's GOP -- and on a refusal nothing is set.  out == NULL
 * (or no targets, sse and maxdiff): no outputs again.  Works for PNM-fed and device-fed sequences. */
typedef struct fiasco_amd_seq_outputs {
    const fiasco_amd_device_target *targets;  /* [n] display order, or NULL; targets[i].data == NULL: not this frame */
    unsigned long long *sse;                  /* [n][3] host memory, or NULL */
    unsigned           *maxdiff;              /* [n][3] host memory, or NULL */
    unsigned char      *written;              /* [n] host memory, or NULL */
    void               *stream;               /* as fiasco_amd_batch_decode_device() */
} fiasco_amd_seq_outputs;
int fiasco_amd_seq_set_outputs_device(fiasco_amd_seq_t *seq, const fiasco_amd_seq_outputs *out);   /* NULL: none again */

#ifdef __cplusplus
}
#endif
#endif
