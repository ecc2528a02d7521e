/*
 *  libfiasco_amd_ycbcr.h -- frames that are YCbCr already: NV12, NV21, I420 / YV12 and planar 4:4:4 bytes into the coder
 *  (C ABI, plain types).
 *
 *  The entries of libfiasco_amd.h take PNM and those of libfiasco_amd_hip.h 8-bit gray and RGB; both turn RGB into YCbCr
 *  with the reference's double-precision sums (lib/image.c:365-389).  A hardware video decoder leaves NV12, and this
 *  library's own fiasco_amd_batch_decode_device_420() (libfiasco_amd_420.h) leaves NV12, NV21 or I420: such a frame is
 *  taken as it is.  The reference has no such input -- cfiasco reads PNM only, read_image always allocates 4:4:4 and the
 *  coder codes three full-size bands; FORMAT_4_2_0 occurs on the decoder's side and in restore_mc alone -- so the
 *  conversion is this library's own definition, chosen so that nothing is rounded:
 *
 *      Y [y][x] = (Ybyte [y][x]            - 128) * 16
 *      Cb[y][x] = (Cbbyte[y >> s][x >> s]  - 128) * 16         s = 1 for 4:2:0, 0 for 4:4:4
 *      Cr[y][x] = (Crbyte[y >> s][x >> s]  - 128) * 16
 *
 *  The bytes are the codec's own YCbCr: what fiasco_amd_batch_decode_device_420() writes with clip255((p >> 4) + 128)
 *  and what the distortion kernel compares.  No range or matrix conversion happens: a limited-range or BT.709 source is
 *  the caller's business.  A 4:2:0 chroma sample is replicated over its 2 x 2 pixels: the coder codes full-size bands,
 *  and replication is the one upsampling that invents no value -- clip255((planes >> 4) + 128) sampled at (2 i, 2 j)
 *  gives every frame back byte for byte.  Sizes: the PNM reader's rules and messages (sides even, 32 .. 8192), so the
 *  chroma planes of a 4:2:0 frame are exactly (width / 2) x (height / 2).
 *  Not built: a plane on another device than the share that converts it (no peer copy on this path), NV24 (4:4:4 with
 *  interleaved chroma), 10-bit P010, range or matrix conversion.
 */
#ifndef LIBFIASCO_AMD_YCBCR_H
#define LIBFIASCO_AMD_YCBCR_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One frame: the fields of fiasco_amd_device_target_420 (libfiasco_amd_420.h) with the same meaning, read instead of
 * written, so that the buffers that call filled go straight back in; plus the subsampling. */
typedef struct fiasco_amd_ycbcr_frame {
    const void *y;  size_t y_pitch;          /* 0 = packed */
    const void *cb, *cr; size_t c_pitch;     /* 0 = packed: (width >> s) * c_step */
    unsigned c_step;        /* 1: two planes (I420; YV12 with the pointers swapped; 4:4:4 planar)
                               2: one plane of pairs, cr == cb + 1 (NV12) or cb == cr + 1 (NV21) */
    unsigned subsampling;   /* 0: 4:4:4, 1: 4:2:0 */
    unsigned width, height;
} fiasco_amd_ycbcr_frame;

/* Host memory, in every build of the library: fiasco_amd_batch_stage() and fiasco_amd_seq_open() (libfiasco_amd.h) with
 * YCbCr bytes in place of PNM.  The frames are converted during the call and not referred to afterwards.  The batch and
 * the sequence work with every call of their kind; the frames are colour frames.  NULL + message: n == 0, a quality that
 * is not positive, a NULL plane, c_step other than 1 or 2, c_step 2 with pointers that are not one byte apart or with
 * subsampling 0, subsampling above 1, a size the PNM reader refuses, a pitch below a row. */
fiasco_amd_batch_t *fiasco_amd_batch_stage_ycbcr(unsigned n, const fiasco_amd_ycbcr_frame *frames, float quality,
                                                 const fiasco_c_options_t *options);
fiasco_amd_seq_t *fiasco_amd_seq_open_ycbcr(unsigned n, const fiasco_amd_ycbcr_frame *frames, float quality,
                                            const fiasco_c_options_t *options, unsigned rank, unsigned world);

/* Device memory (the HIP library): fiasco_amd_batch_stage_device(), fiasco_amd_batch_upload_device()
 * (libfiasco_amd_hip.h) and fiasco_amd_seq_open_device() (libfiasco_amd_video.h) in everything but the pixels -- ONE
 * launch of icy_convert_kernel (csrc/hip/input_convert_ycbcr.inc) per device share writes the planes of all its frames;
 * `stream' orders the call in both directions; the upload does not wait on the host for the device; every share gets its
 * memory before any share converts; replacement frames keep the size and colour model, and _upload(), _upload_device()
 * and _upload_device_ycbcr() may follow one another in any order; a video is converted once at open, on the share that
 * searches each group of pictures.  fiasco_amd_batch_input_planes(), the decoded-PSNR calls, the distortion calls and the
 * device outputs of a sequence work on such frames unchanged.
 * Refused with a message, nothing allocated or changed: what the host entries refuse; per plane what the RGB entries
 * refuse (not device memory, rows beyond the allocation); a YCbCr frame replacing a frame of a gray batch ("colour
 * model"); a plane on another device than the share that converts the frame (the message names both devices). */
fiasco_amd_batch_t *fiasco_amd_batch_stage_device_ycbcr(unsigned n, const fiasco_amd_ycbcr_frame *frames, void *stream,
                                                        float quality, const fiasco_c_options_t *options);
int fiasco_amd_batch_upload_device_ycbcr(fiasco_amd_batch_t *b, const fiasco_amd_ycbcr_frame *frames, void *stream);
fiasco_amd_seq_t *fiasco_amd_seq_open_device_ycbcr(unsigned n, const fiasco_amd_ycbcr_frame *frames, void *stream, float quality,
                                                   const fiasco_c_options_t *options, unsigned rank, unsigned world);

#ifdef __cplusplus
}
#endif
#endif
