/*
 *  libfiasco_amd_hip.h -- measurement hooks of the HIP hot path (C ABI, plain types).
 *
 *  The data-path boundary itself is fiasco_coder() / fiasco_amd_encode_batch() in
 *  libfiasco_amd.h; what is declared here only reports what the device coder did, so that
 *  bench.py can compute the roofline figures from the coder's OWN per-call counters
 *   and from HIP-event time measured on the stream the kernel ran on.
 */
#ifndef LIBFIASCO_AMD_HIP_H
#define LIBFIASCO_AMD_HIP_H 1
#include <stddef.h>
#include <stdint.h>
#include "libfiasco_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct fiasco_amd_stats {
    double             kernel_ms;   /* sum of HIP-event durations of fiasco_frame_kernel     */
    unsigned long long launches;    /* kernel launches                                       */
    unsigned long long frames;      /* frames encoded successfully                           */
    /* algorithmic bytes, summed per call from the coder's counters:
     *   bytes_mp   = sum over matching-pursuit calls of 4*D*(2+S) + 4*2^L
     *   bytes_img  = sum over init_range blocks of N*(128+4*NS) + 4*2^lc_max
     *   bytes_gram = sum over appended states of 4*(NL-1)*(s+1)*(1+E) + 4*(NL-1)*(s+1)     */
    unsigned long long bytes_mp, bytes_img, bytes_gram;
    unsigned long long n_mp, n_steps, n_blocks, n_appends, n_fulleval;
    /* per-phase time summed over frames, 100 MHz ticks of workgroup lane 0:
     * init_range, matching pursuit, incremental <block,state> tables, state append
     * (images + Gram rows), serial partition-search bookkeeping, whole frame */
    unsigned long long t_init, t_approx, t_ipis, t_append, t_serial, t_total;
    /* inside matching pursuit: candidate-parallel phase, ordered-replay phase (ticks); number
     * of 64-candidate blocks whose survivors were fully evaluated */
    unsigned long long t_mpA, t_mpB, n_blockevals;
    unsigned long long dbg[8];      /* free-form developer counters */
    /* states of the finished automata (sum / largest) and frames that were encoded a second time
     * because the capacity guess of their slab was too small */
    unsigned long long states_sum, states_max, reencodes;
    /* frames launched per kernel build: default 256 / 1024 threads, big 256 / 512 threads, default
     * 1024 threads with triangular Gram tables */
    unsigned long long frames_by_build[5];
    /* block-level speculation (several workgroups per frame, launches that leave workgroup slots of
     * the chip free): frames encoded that way, blocks whose subtree search was handed to a verifier
     * workgroup, verdicts that confirmed / contradicted the chain's guess, verifications given up
     * after a bounded wait, blocks the chain searched itself, ticks (100 MHz) it waited for verdicts */
    unsigned long long spec_frames, spec_tasks, spec_confirmed, spec_wrong, spec_timeout, spec_inline, spec_wait;
    /* blocks whose <sub-block, state> tables a table worker had ready for the chain / had not */
    unsigned long long spec_tab_used, spec_tab_missed;
    /* wrong guesses after which the chain took over the verifier's state instead of searching the block again */
    unsigned long long spec_adopted;
    /* the device decoder (csrc/hip/frame_decoder.inc): frames decoded, their algorithmic bytes
     * (2 bytes per pixel of every level image written and per (pixel, term) read, + the frame), device time of
     * the flights in microseconds (HIP events around uploads + kernels of a flight of <= 32 frames) */
    unsigned long long decoder_frames, decoder_bytes, decoder_us;
    /* big frames whose table passes were built by several workgroups (frame_coder.h FcCoop), and how many each */
    unsigned long long coop_frames, coop_workgroups;
    /* speculating frames with append helpers (frame_coder.h FcSpecCtl.app_*): Gram rows of appended states that were
     * dealt to the helpers, ticks (100 MHz) the chains waited for them */
    unsigned long long spec_app_rows, spec_app_wait;
} fiasco_amd_stats;

void fiasco_amd_get_stats(fiasco_amd_stats *out);
void fiasco_amd_reset_stats(void);

/* The launcher's choice for a launch of `frames` frames on a device with `cus` compute units: how many
 * workgroups a frame gets (chain + table workers + verifiers, block-level speculation; 0 = one workgroup per
 * frame).  `big_frames`: frames beyond 2048 pixels in a dimension (4K); `narrow_only`: every frame fits the
 * 256-thread build (at most 3072 states with the verifiers' ids); `occupancy`: workgroups of that build a CU
 * holds at once.  A pure function (no device needed); FIASCO_AMD_SPEC overrides it at run time. */
int fiasco_amd_spec_workgroups(unsigned frames, int cus, int big_frames, int narrow_only, int occupancy);

/* name of the hot-path backend linked into this library: "hip-gfx950" for the product,
 * "oracle-cpu" for the test-only oracle library (reference seam: codec/approx.h:24-27,
 * codec/ip.h:22-34, codec/subdivide.h -- the functions the backend replaces). */
const char *fiasco_amd_core_name(void);

/* One process per GPU (BASELINE config 4: frames dealt round robin to the ranks, item i on rank
 * i mod world): the finished streams of all ranks meet on `root` -- the job's only communication, three small
 * collectives over RCCL / xGMI (counts + failure flags, a status round once every rank has its buffers, then lengths +
 * payloads in one padded all-gather).  EVERY rank must call it; a failure of one rank (a device error, no memory for
 * the payload, a deal that is not round robin: rank r must hold ceil((total - r) / world) streams) travels in the
 * next message and all ranks return 0 together before the big all-gather -- nobody is left waiting in a collective.
 * (Exception: a rank that cannot allocate the first 24 (world + 1) bytes of device memory.)  `comm` is the caller's
 * ncclComm_t, `stream` a hipStream_t (or NULL); every rank passes its n_local streams.  On `root`: *all / *all_len hold
 * the *n_all streams of the job in item order (free each with fiasco_amd_free(), the two arrays with free()); the other
 * ranks get *n_all = 0.  RCCL is taken from the process at run time (no link-time dependency).  1 ok / 0 + message.
 * In the reference nothing corresponds: it is single threaded (codec/coder.c:490-668 is the loop that is sharded). */
int fiasco_amd_rccl_gather(void *comm, void *stream, int rank, int world, int root,
                           unsigned n_local, const unsigned char *const *data, const size_t *len,
                           unsigned char ***all, size_t **all_len, unsigned *n_all);

/* Devices.  Frames are independent units: every batch entry -- fiasco_amd_encode_batch(),
 * the staged batches, fiasco_coder() on an all-intra stream or a video (its groups of pictures) -- spreads
 * its frames round robin over the devices of the process, one host thread + stream + slab pool per
 * device, results in input order, no collective.  The devices are: FIASCO_AMD_DEVICES="0,1,..." from the
 * environment if set; else what fiasco_amd_set_devices() chose; else the ONE device of
 * fiasco_amd_set_device() (one process per GPU: the multi-process harness); else every visible device.
 * An id may be listed twice (two shares on one GPU).  Replacement of staged inputs (fiasco_amd_batch_upload) works
 * with several devices too: one pinned host buffer, every share copies the planes of ITS frames.  All return 1 on
 * success, 0 + error message.
 *   Threading.  Calls on DISTINCT batch, sequence and options objects may run at the same time from several host
 * threads, on any mix of entries (fiasco_coder(), fiasco_amd_encode_batch(), staged batches, sequences, the decoding
 * entries, fiasco_amd_get_stats() / _reset_stats()): what they share inside -- the slab pool, the counters and the
 * log2 correction table of a device share -- is locked, and the table is built once whoever asks first.  ONE batch or
 * sequence object is used by one thread at a time.  Calls that spread over more than one device share run one after
 * the other (the shares' worker threads belong to the process, shares.inc for_each_share); a call with one part runs
 * on its calling thread beside them.  fiasco_amd_set_devices(), fiasco_amd_set_device(), fiasco_amd_set_limits() and
 * fiasco_amd_release_memory() must not run while other calls do: they change the device list and the limits that
 * running calls read, and hand the pools' memory back.  The fiasco_amd_selftest_*() entries are meant for one thread;
 * fiasco_amd_selftest_log2_max_ulp() reports the largest distance any comparison of the process has seen. */
/* workgroups per frame the launcher gives the table passes of `frames` big frames (prediction, P/B frames, -z 1/2)
 * on a chip of `cus` CUs: 1, 2, 4 or 8 (csrc/hip/frame_coder.h FcCoop); pure function */
unsigned fiasco_amd_coop_workgroups(unsigned frames, int cus);
/* append helpers per frame the launcher adds to a launch of `frames` speculating frames with G workgroups each
 * (wide_build: the 1024-thread build, frames beyond 3072 states): workgroups that build their shares of the Gram row of
 * every state the chain appends (codec/control.c:48-131, codec/ip.c:184-260; csrc/hip/frame_coder.h FcSpecCtl.app_*).
 * A pure function of its arguments (no device). */
int fiasco_amd_spec_append_helpers(unsigned frames, int cus, int G, int wide_build);
/* which of `shares` device shares of the process takes a job (a pure function, no device): share_key == 0 -> the job's
 * index in the call, round robin (frames of a batch); share_key = key + 1 -> key mod shares whatever the
 * index and however many jobs the call holds.  The sequence engine keys the frames of a video and the decodes of their
 * reference frames by their group of pictures, so a GOP never changes its device (codec/coder.c:490-668 is the loop
 * that is sharded; the reference has one device: the host). */
unsigned fiasco_amd_share_of(unsigned share_key, unsigned index, unsigned shares);
int fiasco_amd_set_device(int device);
int fiasco_amd_set_devices(const int *ids, int n);      /* n = 0: back to the automatic choice */
int fiasco_amd_device_count(void);                      /* shares a batch is split into */

/* Frames that already live in device memory.  The batch entries of libfiasco_amd.h take PNM bytes on the host; these
 * take 8-bit pixels where a decoder, a renderer or a tensor library left them, and ONE kernel launch per device share
 * converts all of them into the coder's planes -- bit for bit what the PNM reader writes (lib/image.c:365-389: gray
 * (g - 128) * 16; colour the three double-precision sums, left to right, * 16, truncated) -- inside HBM.
 *   layout        GRAY8: height x width bytes; RGB8_INTERLEAVED: height x width x 3, PPM order R, G, B;
 *                 RGB8_PLANAR: 3 x height x width, planes plane_stride bytes apart
 *   pitch         bytes between rows, >= width * bytes per pixel (a frame cut out of a larger picture); 0 = packed
 *   stream        the hipStream_t on which the caller's pixels become ready (NULL: the default stream).  The library
 *                 makes its conversion wait for what `stream' holds at the call and makes `stream' wait for the
 *                 conversion: the caller may overwrite or free the source in stream order right after the call.
 * fiasco_amd_batch_stage_device() is fiasco_amd_batch_stage() without PNM: same options, same size rules and messages
 * (sides even, 32 .. 8192), and the batch works with every batch call of libfiasco_amd.h; _upload() and
 * _upload_device() may follow each other in any order.  fiasco_amd_batch_upload_device() is fiasco_amd_batch_upload():
 * new frames of the same size and colour model for every slot, converted into the buffer the running pass does not
 * read and taken over by the next submit.  It does not wait on the host for the caller's stream or for the conversion;
 * its one host wait is for the descriptor table of the upload before, a few KiB copied a pass earlier.  Refused with
 * a message, the batch unchanged:
 * n == 0, a pointer that is not device memory (hipPointerGetAttributes) or whose rows leave its allocation, a pitch
 * smaller than a row, a layout that contradicts the batch's colour model.  With several device shares every share
 * converts its own frames on its own device (a source on another device is fetched over the peer link first).
 * fiasco_amd_batch_input_planes(): the planes the coder sees for frame i, all bands back to back (width * height
 * int16 each, 12.4 fixed point), for PNM-fed and device-fed batches.  The decoded-PSNR calls fetch the original the
 * same way when a frame has no host copy.  Videos: fiasco_amd_seq_open_device() (libfiasco_amd_video.h); fiasco_coder() takes file names. */
enum { FIASCO_AMD_GRAY8 = 0, FIASCO_AMD_RGB8_INTERLEAVED = 1, FIASCO_AMD_RGB8_PLANAR = 2 };
typedef struct fiasco_amd_device_frame {
    const void *data;        /* device memory */
    size_t pitch;            /* bytes between rows; 0 = tightly packed */
    size_t plane_stride;     /* bytes between colour planes (PLANAR); 0 = pitch * height */
    unsigned width, height;
    int layout;
} fiasco_amd_device_frame;

fiasco_amd_batch_t *fiasco_amd_batch_stage_device(unsigned n, const fiasco_amd_device_frame *frames,
                                                  void *stream, float quality, const fiasco_c_options_t *options);
int fiasco_amd_batch_upload_device(fiasco_amd_batch_t *b, const fiasco_amd_device_frame *frames, void *stream);
int fiasco_amd_batch_input_planes(const fiasco_amd_batch_t *b, unsigned i, int16_t *out);

/* The way back: decoded frames as 8-bit pixels in device memory.  The device decoder (csrc/hip/frame_decoder.inc)
 * reconstructs a frame in HBM; ONE kernel launch per flight of <= 32 frames (csrc/hip/output_convert.inc) then writes
 * the bytes `dfiasco -s 0 -o' puts into its PGM / PPM -- lib/image.c gray_write :450-480: clip255((p >> 4) + 128);
 * color_write :534-582 with the chroma tables of :487-532 -- into buffers the caller owns.  No pixel crosses to the
 * host.  A target has the fields of fiasco_amd_device_frame with the same meaning (layout, pitch, plane_stride; 0 =
 * packed), its memory is written.
 * fiasco_amd_batch_decode_device(): the frames of the batch's last finished pass into targets[i] (b->n entries).
 * Frames without a finished intra automaton are skipped as fiasco_amd_batch_decode_psnr_all() skips them, and so is
 * frame i when targets[i].data == NULL.  Returns the number of frames written; 0 + message when nothing could be done.
 *   stream        the hipStream_t on which the targets were last used (NULL: the default stream).  The conversion
 *                 waits for what `stream' holds at the call, and `stream' is made to wait for the conversion: the
 *                 caller may read the pixels in stream order without a host synchronisation.  The call itself waits
 *                 on the host for the decoder's flights.
 * Refused with a message, nothing written: b == NULL, an empty batch, no finished pass; a target that is not device
 * memory (hipPointerGetAttributes) or whose rows leave its allocation; a pitch smaller than a row; a width or height
 * other than the frame's; a layout that contradicts the colour model (GRAY8 <-> gray, the RGB8 layouts <-> colour); a
 * target on a device other than the one the frame's share decodes on (the message names both; there is no peer copy on
 * this path).  Intra frames only; the frame of `dfiasco -s 0'; smoothed: fiasco_amd_batch_decode_device_smoothed()
 * (libfiasco_amd_smooth.h); magnified: fiasco_amd_batch_decode_device_magnified() below.
 * fiasco_amd_planes_to_pixels_device(): the conversion alone, on `stream' itself: planes [bands][height][width] int16
 * (12.4 fixed point, bands = color ? 3 : 1) in device memory -> target.  1 ok / 0 + message. */
typedef struct fiasco_amd_device_target {
    void *data;              /* device memory, written */
    size_t pitch;            /* bytes between rows; 0 = tightly packed */
    size_t plane_stride;     /* bytes between colour planes (PLANAR); 0 = pitch * height */
    unsigned width, height;
    int layout;
} fiasco_amd_device_target;

int fiasco_amd_batch_decode_device(const fiasco_amd_batch_t *b, const fiasco_amd_device_target *targets, void *stream);
int fiasco_amd_planes_to_pixels_device(const int16_t *planes, int color, const fiasco_amd_device_target *target, void *stream);

/* How good is what was just coded: the decoded frames of a staged batch compared with their originals in device memory
 * (csrc/hip/distortion.inc).  Behind the kernels of every decoder flight ONE reduction kernel compares the decoded
 * planes with the original planes, both as the bytes fiasco_amd_batch_decode_psnr() compares -- clip255((p >> 4) + 128),
 * Y, Cb and Cr as planes -- and returns per frame and band the EXACT integer sum of the squared differences and the
 * largest absolute difference: 12 bytes per band cross to the host, no plane.  (The PSNR calls sum in float as
 * bin/pnmpsnr.c does; below 2^24 that sum is this one, beyond it rounds.)  The original of a frame that was handed over
 * in device memory is read where the input conversion left it when that is the device the frame is decoded on; every
 * other original is copied up from its host planes.  Intra frames of staged batches only; the unsmoothed frame (the
 * smoothed one: fiasco_amd_batch_decode_distortion_device_smoothed(), libfiasco_amd_smooth.h).
 * fiasco_amd_batch_decode_distortion_device(): */
/* frames of the last finished pass: decoded on the device, compared with their originals on the device.
 * sse / maxdiff: [b->n][3], either may be NULL; bands a frame does not have and skipped frames get 0.
 * targets: NULL, or b->n targets with the rules, layouts and bytes of fiasco_amd_batch_decode_device()
 * (data == NULL: measured, not written) -- one decode serves both.  Returns the number of frames measured. */
int fiasco_amd_batch_decode_distortion_device(const fiasco_amd_batch_t *b, unsigned long long *sse, unsigned *maxdiff,
                                              const fiasco_amd_device_target *targets, void *stream);
/* Refused with a message, nothing written: b == NULL, an empty batch, no finished pass; sse, maxdiff and targets all
 * NULL; every target refusal of fiasco_amd_batch_decode_device(). */
/* the reduction alone, on `stream': two sets of planes [bands][height][width] int16 in device memory,
 * width, height 1 .. 8192 (any parity), bands 1 or 3; the call waits on the host.  1 ok / 0 + message. */
int fiasco_amd_planes_distortion_device(const int16_t *a, const int16_t *b, int bands, unsigned width, unsigned height,
                                        unsigned long long sse[3], unsigned maxdiff[3], void *stream);
/* Refused with a message, nothing written: a pointer that is not device memory, planes that leave their allocation,
 * planes on different devices, a size or a band count out of range. */

/* Magnification: the reference's decoder shows a stream at 2^M times its side length (`dfiasco -m M', enlarge_image,
 * codec/decoder.c:776-840): M < 0 gives thumbnails, M > 0 enlargements, both computed from the automaton, not scaled
 * from pixels -- 2 M is added to the level of every state and the coordinates are shifted by M.  The device decoder's
 * recursion never asks for the level of a state, so the frame at M is the images of the same states at level + 2 M
 * (csrc/hip/frame_decoder.inc).  Intra frames of staged batches; unsmoothed (`-s 0'): libfiasco_amd_display.h has the smoothed siblings.
 * fiasco_amd_magnified_size(): the size a frame of width x height is shown at, and whether the reference decodes it
 * at all (codec/dfiasco.c:104-137, codec/decoder.c:329-342) -- a pure function, no device.
 *   magnify > 0   width << magnify, height << magnify; refused if width * height << 2 n > 2048 * 2048 for an n in
 *                 1 .. magnify
 *   magnify < 0   k = -magnify: width >> k, height >> k, each rounded up to even; refused if width >> n < 32 or
 *                 height >> n < 32 for an n in 0 .. k
 * 1 + the size (out_w, out_h may be NULL), or 0 + a message that ends with the largest / smallest value the frame
 * allows ("Maximum value is 2.", "Minimum value is -1."), as the reference's message does.  The limits are the
 * reference's although this library codes sides up to 8192: only what the reference decodes can be pinned. */
int fiasco_amd_magnified_size(unsigned width, unsigned height, int magnify, unsigned *out_w, unsigned *out_h);
/* fiasco_amd_batch_decode_device() at a magnification: every target has the size of fiasco_amd_magnified_size(); the
 * bytes are those of `dfiasco -s 0 -m magnify -o'.  magnify == 0 gives the bytes of fiasco_amd_batch_decode_device().
 * Refused with a message, nothing written: every refusal of that call; a finished intra frame of the batch the size rule
 * refuses at `magnify'; a target of another size, the coded one included (the message names the target's size, the
 * coded one and the magnified one).  A frame fails alone, with a message, when its level of linear combinations + 2 magnify
 * is above 24, or when it is below 0: blocks smaller than the reduction, which the reference shows by clamping their
 * level at 0 so that several land on one pixel -- refused here, not reproduced.  An enlargement costs 4^magnify times
 * the level images of the full-size decode, in time and in device memory. */
int fiasco_amd_batch_decode_device_magnified(const fiasco_amd_batch_t *b, int magnify, const fiasco_amd_device_target *targets, void *stream);
/* fiasco_amd_batch_decode_planes() (libfiasco_amd.h) at a magnification, the host route: int16 12.4 planes
 * [bands][height'][width'] of the magnified size.  Refusals as that call's, the size rule's, and the two a frame fails
 * with above.  A library whose decoder hands back the coded size (the test oracle's) is refused with a message saying
 * that its backend does not magnify.  1 ok / 0 + message. */
int fiasco_amd_batch_decode_planes_magnified(const fiasco_amd_batch_t *b, unsigned i, int magnify, int16_t *out);
/* One decode, the frame and its thumbnail: fiasco_amd_batch_decode_device() into targets[i] -- targets may be NULL, and
 * targets[i].data may be NULL: the thumbnail alone -- and the frame at magnification -reduce (reduce >= 1) into
 * thumbs[i] (b->n entries, the size of fiasco_amd_magnified_size(); data == NULL: none for this frame; a frame with
 * neither is skipped).  The thumbnail consists of the level images the decoder has written on its way to the full frame:
 * behind the level launches of a flight ONE launch gathers them into reduced planes (dec_thumb_kernel) and one more
 * conversion launch writes them.  The bytes are those of fiasco_amd_batch_decode_device_magnified(b, -reduce, ...).
 * Refused with a message, nothing written: every refusal of fiasco_amd_batch_decode_device() for either set of targets;
 * thumbs == NULL; reduce == 0; a frame with a thumbnail the size rule refuses at -reduce.  A frame whose blocks are smaller
 * than the reduction fails alone, nothing of it written.  Returns the number of frames decoded. */
int fiasco_amd_batch_decode_device_thumbnails(const fiasco_amd_batch_t *b, const fiasco_amd_device_target *targets, unsigned reduce,
                                              const fiasco_amd_device_target *thumbs, void *stream);

/* The launcher keeps the per-frame HBM slabs of finished calls in a process-wide pool
 * (hipMalloc of hundreds of MB per frame is slow); this returns the pool to the driver. */
void fiasco_amd_release_memory(void);

/* Self test of the one libm function the rate models need on both sides of the seam: double
 * log2 of a float probability (codec/coeff.c:232-237, codec/domain-pool.c:772,
 * codec/bintree.c:67).  Evaluates it on the device for EVERY float with a biased exponent in
 * [exp_lo, exp_hi] (1..127: all of (0, 1]) and compares with the host's libm bit for bit.
 * n_double: arguments whose double results differ; n_float: those whose (float) -log2 differ
 * too (first_bad = one of them).  Returns 1 when the run completed. */
int fiasco_amd_selftest_log2(unsigned exp_lo, unsigned exp_hi, unsigned long long *n_checked,
                             unsigned long long *n_double, unsigned long long *n_float,
                             float *first_bad);

/* The same comparison through the table the frame kernel consults for the arguments on which the
 * two libm's differ (built once per process and device, cached under $FIASCO_AMD_CACHE or
 * /tmp): n_double must be 0 -- the coefficient prices, which subtract these doubles from a float
 * sum (codec/coeff.c:228-236), are then the host's for every probability that can occur.
 * n_entries = size of the table. */
/* largest distance, in ulps, between a device and a host logarithm seen by the comparisons so far */
unsigned long long fiasco_amd_selftest_log2_max_ulp(void);
int fiasco_amd_selftest_log2_patched(unsigned exp_lo, unsigned exp_hi, unsigned long long *n_checked,
                                     unsigned long long *n_double, unsigned long long *n_entries);

#ifdef __cplusplus
}
#endif
#endif
