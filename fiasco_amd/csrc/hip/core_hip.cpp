/*
 *  core_hip.cpp -- host launcher of the device frame coder: implements the seam of
 *  fa_host.h (fa_core_stage / fa_core_run / fa_core_unstage / fa_core_encode_frames) on
 *  top of the HIP runtime.
 *
 *  stage : carve one HBM slab per frame (layout: frame_coder.h) from a process-wide slab
 *          pool, upload the int16 pixel plane; the basis automaton travels inside the
 *          DevFrame descriptor.  After stage the inputs are resident in HBM.
 *  run   : ONE persistent kernel launch with one workgroup per staged frame (all frames in
 *          flight at once); every frame packs its finished automaton into a per-launch
 *          buffer, which comes down with ONE device->host copy on a second stream (double
 *          buffered: the next launch does not wait for it).  Frames whose state capacity
 *          guess was too small are re-staged with a larger slab and relaunched.
 *  There is no CPU fallback: without a usable GPU every job fails with an error message.
 *
 *  This file is the translation unit: what every part needs (switches, the state of a device, the table of kernel
 *  builds, buffers) and, below that, the parts themselves -- one include file per concern, in the order they build on
 *  each other.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stddef.h>
#include <math.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <pthread.h>
#include <unistd.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <algorithm>
#include <atomic>
#include <string>
#include <utility>
#include <vector>
#include "fa_host.h"
#include "frame_coder.h"
#include "libfiasco_amd_hip.h"
#include "libfiasco_amd_video.h"
#include "libfiasco_amd_smooth.h"
#include "libfiasco_amd_display.h"
#include "libfiasco_amd_render.h"
#include "libfiasco_amd_render_420.h"
#include "libfiasco_amd_420.h"
#include "libfiasco_amd_ycbcr.h"
#include "libfiasco_amd_stream.h"

/* Developer and test switches (FIASCO_AMD_SPEC, _NO_WIDE, _FORCE_TRI, _CAP_GUESS, _QUEUE_SLABS, _TRACE, ...)
 * are honoured only when FIASCO_AMD_DEBUG is set to something other than 0: a drop-in library must not
 * change its behaviour because of a stray variable in a user's environment.  What a user may set without
 * it: FIASCO_AMD_CACHE (cache directory), FIASCO_AMD_NO_LOG2_TABLE (encode without the log2 correction
 * table), FIASCO_AMD_DEVICES (devices the batch entries spread their frames over, shares.inc). */
extern "C" const char *fa_knob(const char *name)
{
    const char *d = getenv("FIASCO_AMD_DEBUG");
    return d && *d && strcmp(d, "0") != 0 ? getenv(name) : nullptr;
}
/* a numeric switch: its value, or `d' when it is not set (callers check the range themselves) */
static long long knob_int(const char *name, long long d)
{
    const char *e = fa_knob(name);
    return e ? atoll(e) : d;
}

/* ------------------------------------------------------------------ per-device state
 * DevState, the state of share 0 (g_state0), the calling thread's share (t_dev) and the lock every share has */
#include "dev_state.h"

/* the kernel builds (frame_coder.hip, one object per build: Makefile FC_BUILDS) */
typedef void launch_fn(DevFrame *d_frames, unsigned n, unsigned nlend, unsigned long long *ring, unsigned *ctr,
                       const unsigned *ptrmask, unsigned long long queue_wait_ticks, unsigned coopW, hipStream_t stream);
/* block-level speculation (frame_coder.h, FcSpecCtl): n frames with G workgroups and H append helpers each */
typedef void spec_launch_fn(DevFrame *d_frames, DevFrame *d_vframes, unsigned n, unsigned G, unsigned H, hipStream_t stream);
extern "C" launch_fn fc_launch, fc_launch_wide, fc_launch_big, fc_launch_big_wide, fc_launch_wide_tri, fc_launch_big_hm,
                     fc_launch_big_gm;
extern "C" spec_launch_fn fc_launch_spec, fc_launch_spec_wide;
extern "C" unsigned fc_spec_slot_bytes(void), fc_spec_slot_bytes_wide(void), fc_spec_ctl_bytes(void);
/* workgroups (= frames) of a kernel build that one CU holds at once, as the runtime computes it
 * from the build's registers and LDS (frame_coder.hip FC_OCCUPANCY) */
extern "C" int fc_occupancy(void), fc_occupancy_wide(void), fc_occupancy_big(void), fc_occupancy_big_wide(void),
               fc_occupancy_spec(void);

/* The nine kernel builds in the order a launch orders its frames and starts them.  wide: 1024 threads per
 * workgroup (default geometry) or 512 (big); tri: triangular Gram tables; hm, gm: the big build with larger
 * coefficient models / the other model registries; spec: several workgroups per frame.  Only the builds up to
 * B_WIDE_TRI take frames that borrow a slab (queue_eligible). */
enum Build { B_DEFAULT, B_WIDE, B_BIG, B_BIG_WIDE, B_WIDE_TRI, B_BIG_HM, B_BIG_GM, B_SPEC, B_SPEC_WIDE, N_BUILDS };
struct BuildInfo {
    launch_fn      *launch;         /* one workgroup per frame, or the frame queue */
    spec_launch_fn *spec_launch;    /* the speculating builds instead */
    int             stats_slot;     /* fiasco_amd_stats.frames_by_build[]; -1: counted in spec_frames */
    int           (*occupancy)(void);   /* what frames_per_cu() answers for frames of the build */
};
static const BuildInfo k_build[N_BUILDS] = {
    { fc_launch,          nullptr,              0, fc_occupancy },
    { fc_launch_wide,     nullptr,              1, fc_occupancy_wide },
    { fc_launch_big,      nullptr,              2, fc_occupancy_big },
    { fc_launch_big_wide, nullptr,              3, fc_occupancy_big_wide },
    { fc_launch_wide_tri, nullptr,              4, fc_occupancy_wide },
    { fc_launch_big_hm,   nullptr,              3, fc_occupancy_big_wide },
    { fc_launch_big_gm,   nullptr,              3, fc_occupancy_big_wide },
    { nullptr,            fc_launch_spec,      -1, fc_occupancy },
    { nullptr,            fc_launch_spec_wide, -1, fc_occupancy_wide },
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

/* a device buffer (or pinned host buffer) of at least `need' elements: kept while it is large enough, else
 * allocated afresh; false, with the buffer empty, when there is no room (each caller decides what that means) */
template <typename T> static bool grow_buffer(T *&p, size_t &n, size_t need, bool pinned = false)
{
    if (need <= n) return true;
    if (p) (void) (pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr; n = 0;
    if ((pinned ? hipHostMalloc((void **) &p, need * sizeof(T), hipHostMallocDefault) : hipMalloc((void **) &p, need * sizeof(T)))
        != hipSuccess) { p = nullptr; (void) hipGetLastError(); return false; }
    n = need;
    return true;
}

/* ------------------------------------------------------------------ the parts
 * What one of them uses of a later one: */
struct Staged;                                  /* enc_stage.inc */
/* input_convert.inc: the planes of every slot's frame from 8-bit pixels in device memory into up_dev[parity].  The frames
 * of a call are of ONE kind -- gray / RGB (fiasco_amd_device_frame, ic_convert_kernel) or YCbCr (fiasco_amd_ycbcr_frame,
 * input_convert_ycbcr.inc icy_convert_kernel) -- and everything between the entry points and the launch sees them through
 * the kind: "describe this frame" and "launch" */
struct IcKind {
    const char *what;               /* "device frame", "YCbCr frame": how the messages name a frame */
    size_t frame_bytes;             /* the caller's struct, checked and with its pitches filled in */
    size_t entry_bytes;             /* the kernel's descriptor of a frame */
    void (*geometry)(const void *frame, unsigned *width, unsigned *height, int *color);
    int  (*device_of)(const void *frame);           /* where the pixels lie; -1: unknown */
    /* what to fetch over the peer link first when that is another device: bytes from *first on; 0: the kind has no peer copy */
    size_t (*peer_extent)(const void *frame, const void **first);
    /* the table entry of `frame', read at src (NULL: where the frame says; else a copy of peer_extent bytes) and written to
     * dst; total: the work items of the frames before it, moved on */
    void (*describe)(void *entry, const void *frame, const void *src, int16_t *dst, unsigned long long &total);
    /* ONE launch for the n frames of the table at d_tab (device memory) on `stream' */
    bool (*launch)(const void *d_tab, unsigned n, unsigned long long total, int ncu, hipStream_t stream);
};
/* room for a table entry of either kind: a share's table is allocated for this size per frame, so that uploads of both
 * kinds may follow one another without the table ever being freed and allocated again on the hot call */
enum { IC_ENTRY_MAX = 96 };
struct IcInput {
    const IcKind *kind;
    const void   *frames;           /* one per job, kind->frame_bytes apart */
    const void *at(size_t i) const { return (const char *) frames + i * kind->frame_bytes; }
};
static bool ic_convert(Staged *S, const IcInput &in, int parity, hipEvent_t ready, bool next, bool prepare_only);

#include "log2_table.inc"       /* log2 on the device against the host's: self test kernel, comparison, correction table, its disk cache */
#include "slab_pool.inc"        /* the pool of HBM slabs of a device: pool_device, slab_acquire, slab_release */
#include "enc_layout.inc"       /* which kernel build a frame needs, the layout of its slab, what the device coder refuses */
#include "enc_policy.inc"       /* capacity memory; workgroups per frame (coop, speculation, append helpers) and their query entries */
#include "enc_stage.inc"        /* FrameSlot, Staged; frames into slabs and the frame queue; replacement inputs of a staged batch */
#include "enc_launch.inc"       /* a wave of launches, its download and outcome: collect .. core1_submit, core1_finish2 */
#include "shares.inc"           /* the devices of the process and their DevStates, share workers, the dealing rule, fa_core_*() */
#include "rccl_gather.inc"      /* fiasco_amd_rccl_gather: the streams of all ranks onto one */

/* ------------------------------------------------------------------ the device decoder and its outlets
 * What the five files below agree on.  The decoder (frame_decoder.inc) works in flights of at most DEC_FLIGHT frames:
 * the tables a flight uploads (DecDesc, SmDesc, OcFrame, DsPlane) and the result array of its measuring launch
 * (distortion.inc DS_SLOTS) have room for that many. */
enum { DEC_FLIGHT = 32 };

struct OcOut;                                   /* output_convert.inc */
struct DsOut;                                   /* distortion.inc */
static int decode_frames(unsigned n, fa_dec_job *jobs, const OcOut *out, const DsOut *ds, bool images = false);      /* frame_decoder.inc */

#include "px_access.inc"          /* the partial 16-byte accesses of the pixel kernels below; the one host-replay switch */
#include "frame_table.inc"        /* how those kernels walk the frames of a launch, how they are launched */
#include "input_convert.inc"
#include "input_convert_ycbcr.inc" /* beside input_convert.inc: NV12 / NV21 / I420 / planar 4:4:4 bytes instead of gray and RGB, through the same plumbing */
#include "output_convert.inc"
#include "distortion.inc"
#include "smooth.inc"
#include "render.inc"             /* beside output_convert.inc: display surfaces instead of 8-bit pixels; its batch entry is smooth.inc's with surfaces */
#include "output_convert_420.inc" /* beside output_convert.inc: NV12 / NV21 / I420 buffers of frames decoded in 4:2:0 */
#include "render_420.inc"         /* behind both: display surfaces of frames decoded in 4:2:0 */
#include "frame_decoder.inc"
#include "stream_decode.inc"        /* behind the decoder: the frames of a .fco stream that was read, video frames included, into device buffers */
#include "decoder_outlet.inc"       /* beside it: the shown planes of such frames into the images of a fiasco_decoder_t (fa_decoder.c) */
