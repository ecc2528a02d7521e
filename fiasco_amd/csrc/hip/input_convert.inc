/*
 *  input_convert.inc -- frames that already live in device memory (included by core_hip.cpp).
 *
 *  The PNM entries parse a header on the host, convert every pixel there (host/fa_image.c convert_planes, reference
 *  lib/image.c:365-389) and copy the 12.4 fixed-point planes through pinned memory into HBM.  Here the 8-bit pixels
 *  are in HBM already: ONE launch of ic_convert_kernel per device share writes the planes of all its frames into the
 *  input buffer that the hand-over of replacement frames uses anyway (Staged::up_dev, FrameSlot::ext_pix / ext_next).
 *  The host never sees a pixel; fa_image_host_planes() fetches planes back for the few calls that want them.
 *
 *  Arithmetic: exactly convert_planes().  gray (g - 128) * 16; colour the three sums in double, evaluated left to
 *  right, * 16 last, truncated toward zero to int and narrowed.  Nothing may be contracted into a fused multiply-add:
 *  the file is built with -ffp-contract=off and the function says so again.
 *
 *  Shape: frame_table.inc's -- one table entry per frame (IcFrame), one sequence of work items.  A work item is 16
 *  neighbouring pixels of one row -- one 16-byte load per 8-bit plane (three for interleaved RGB) where the address allows
 *  it, byte loads otherwise (a ragged row end, a source that starts at an odd column), and 32 bytes of int16 per band,
 *  stored as 16-byte vectors (8- or 4-byte ones where a row of the plane does not start on a 16-byte boundary).
 *  Neighbouring lanes take neighbouring items, so a wave reads 1 KiB and writes 2 KiB per band contiguously.
 *
 *  Build (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): ic_convert_kernel 132 VGPRs, 56 SGPRs,
 *  no scratch, no LDS, 3 waves per SIMD; global_ accesses only.
 */

struct IcFrame {
    const unsigned char *src;        /* first pixel */
    int16_t            *dst;         /* planes [bands][height][width] */
    unsigned long long  pitch, plane_stride;
    unsigned long long  first;       /* work items of the frames before this one */
    unsigned            width, height, layout, cpr;    /* cpr: items per row */
};

PX_DEV unsigned ic_byte(const unsigned *w, unsigned k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }
PX_DEV unsigned ic_pair(int lo, int hi) { return ((unsigned) lo & 0xffffu) | ((unsigned) hi << 16); }

/* work item `local' of frame F */
PX_DEV void ic_item(const IcFrame &F, unsigned local)
{
#pragma clang fp contract(off)
    const unsigned row = local / F.cpr, x0 = (local - row * F.cpr) * 16;
    const unsigned n = F.width - x0 < 16 ? F.width - x0 : 16;
    const size_t npix = (size_t) F.width * F.height;
    int16_t *q = F.dst + (size_t) row * F.width + x0;
    const unsigned char *p = F.src + (size_t) row * F.pitch;
    unsigned out[8];
    if (F.layout == FIASCO_AMD_GRAY8) {
        unsigned w[4];
        px_load_bytes_vec(p + x0, n, w);
#pragma unroll
        for (unsigned k = 0; k < 8; k++)
            out[k] = ic_pair(((int) ic_byte(w, 2 * k) - 128) * 16, ((int) ic_byte(w, 2 * k + 1) - 128) * 16);
        px_store_values(q, n, out);
        return;
    }
    unsigned w[12];
    if (F.layout == FIASCO_AMD_RGB8_INTERLEAVED) {
        const unsigned char *s = p + (size_t) x0 * 3;
        const unsigned nb = n * 3;
        px_load_bytes_vec(s, nb >= 16 ? 16 : nb, w);
        px_load_bytes_vec(s + 16, nb >= 32 ? 16 : nb > 16 ? nb - 16 : 0, w + 4);
        px_load_bytes_vec(s + 32, nb >= 48 ? 16 : nb > 32 ? nb - 32 : 0, w + 8);
    } else {
        px_load_bytes_vec(p + x0, n, w);
        px_load_bytes_vec(p + F.plane_stride + x0, n, w + 4);
        px_load_bytes_vec(p + 2 * F.plane_stride + x0, n, w + 8);
    }
    int y[16], cb[16], cr[16];
#pragma unroll
    for (unsigned k = 0; k < 16; k++) {
        int r, g, bl;
        if (F.layout == FIASCO_AMD_RGB8_INTERLEAVED) { r = (int) ic_byte(w, 3 * k); g = (int) ic_byte(w, 3 * k + 1); bl = (int) ic_byte(w, 3 * k + 2); }
        else { r = (int) ic_byte(w, k); g = (int) ic_byte(w + 4, k); bl = (int) ic_byte(w + 8, k); }
        /* host/fa_image.c:108-110, character for character: double arithmetic, left to right, C truncation */
        y[k]  = (int) ((+0.2989 * r + 0.5866 * g + 0.1145 * bl - 128) * 16);
        cb[k] = (int) ((-0.1687 * r - 0.3312 * g + 0.5000 * bl) * 16);
        cr[k] = (int) ((+0.5000 * r - 0.4183 * g - 0.0816 * bl) * 16);
    }
#pragma unroll
    for (unsigned k = 0; k < 8; k++) out[k] = ic_pair(y[2 * k], y[2 * k + 1]);
    px_store_values(q, n, out);
#pragma unroll
    for (unsigned k = 0; k < 8; k++) out[k] = ic_pair(cb[2 * k], cb[2 * k + 1]);
    px_store_values(q + npix, n, out);
#pragma unroll
    for (unsigned k = 0; k < 8; k++) out[k] = ic_pair(cr[2 * k], cr[2 * k + 1]);
    px_store_values(q + 2 * npix, n, out);
}

__global__ void __launch_bounds__(256) ic_convert_kernel(const IcFrame *__restrict__ frames, unsigned nframes, unsigned long long total)
{
    ft_walk<ic_item>(frames, nframes, total);
}

/* ------------------------------------------------------------------ one share */

static size_t ic_row_bytes(const fiasco_amd_device_frame &f) { return (size_t) f.width * (f.layout == FIASCO_AMD_RGB8_INTERLEAVED ? 3 : 1); }
/* bytes from the first to behind the last pixel (pitch and plane_stride filled in) */
static size_t ic_extent(const fiasco_amd_device_frame &f)
{
    return (f.layout == FIASCO_AMD_RGB8_PLANAR ? 2 * f.plane_stride : 0) + (size_t) (f.height - 1) * f.pitch + ic_row_bytes(f);
}

/* the entry of the descriptor table for frame f, read at src (f.data, or where a copy of its bytes lies) and written to
 * dst; total: the work items of the frames before it, moved on */
static void ic_describe(IcFrame &d, const fiasco_amd_device_frame &f, const void *src, int16_t *dst, unsigned long long &total)
{
    d.src = (const unsigned char *) src; d.dst = dst;
    d.pitch = f.pitch; d.plane_stride = f.plane_stride; d.first = total;
    d.width = f.width; d.height = f.height; d.layout = (unsigned) f.layout; d.cpr = (f.width + 15) / 16;
    total += (unsigned long long) d.cpr * f.height;
}

static bool ic_launch(const IcFrame *d_tab, unsigned n, unsigned long long total, int ncu, hipStream_t stream)
{
    return ft_launch(ic_convert_kernel, d_tab, n, total, ncu, stream);
}

/* the device a pointer's memory lies on; -1: unknown */
static int ic_device_of_pointer(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess) return at.device;
    (void) hipGetLastError();
    return -1;
}

static_assert(sizeof(IcFrame) <= IC_ENTRY_MAX, "IC_ENTRY_MAX (core_hip.cpp) is the room of a table entry");

/* gray and RGB frames as a kind (core_hip.cpp IcKind) */
static const IcKind IC_RGB = {
    "device frame", sizeof(fiasco_amd_device_frame), sizeof(IcFrame),
    [](const void *f, unsigned *w, unsigned *h, int *color) {
        const fiasco_amd_device_frame &F = *(const fiasco_amd_device_frame *) f;
        *w = F.width; *h = F.height; *color = F.layout != FIASCO_AMD_GRAY8;
    },
    [](const void *f) { return ic_device_of_pointer(((const fiasco_amd_device_frame *) f)->data); },
    [](const void *f, const void **first) { *first = ((const fiasco_amd_device_frame *) f)->data; return ic_extent(*(const fiasco_amd_device_frame *) f); },
    [](void *entry, const void *f, const void *src, int16_t *dst, unsigned long long &total) {
        const fiasco_amd_device_frame &F = *(const fiasco_amd_device_frame *) f;
        ic_describe(*(IcFrame *) entry, F, src ? src : F.data, dst, total);
    },
    [](const void *d_tab, unsigned n, unsigned long long total, int ncu, hipStream_t stream) { return ic_launch((const IcFrame *) d_tab, n, total, ncu, stream); },
};

/* the planes of a frame of the kind's geometry, as they lie in the input buffer */
static size_t ic_planes_bytes(const fa_image *im) { return align_up((size_t) im->width * im->height * (im->color ? 3 : 1) * 2, 256); }

/* The planes of every slot's frame into up_dev[parity], by one kernel launch on the upload stream after `ready'.
 * in.at(j) belongs to jobs[j]; its pitches are filled in and everything was checked (ic_check_frame, icy_check_frame).
 * next: the frames of the NEXT pass (ext_next, taken over by the next submit), else of the first pass (ext_pix).
 * Records ev_up behind the kernel.  Nothing here waits on the host for the device, but for the descriptor table of
 * the upload before this one, which a whole pass ago left the pinned memory.
 * prepare_only: everything that can run out of memory -- stream, events, the input buffer, the staging buffer, the
 * descriptor table -- and nothing else: no buffer is written, no slot changed.  The upload entries prepare
 * every share before any share converts, so that a share without memory refuses the upload while the batch is whole. */
static bool ic_convert(Staged *S, const IcInput &in, int parity, hipEvent_t ready, bool next, bool prepare_only)
{
    const size_t ns = S->slots.size();
    const IcKind &K = *in.kind;
    if (!ns) return true;
    if (!S->ustream && hipStreamCreateWithFlags(&S->ustream, hipStreamNonBlocking) != hipSuccess) { S->ustream = nullptr; goto hip_failed; }
    if (!S->ev_up && hipEventCreateWithFlags(&S->ev_up, hipEventDisableTiming) != hipSuccess) { S->ev_up = nullptr; goto hip_failed; }
    if (!S->ev_ic && hipEventCreateWithFlags(&S->ev_ic, hipEventDisableTiming) != hipSuccess) { S->ev_ic = nullptr; goto hip_failed; }
    {
        int here = -1;
        if (hipGetDevice(&here) != hipSuccess) goto hip_failed;
        size_t need = 0, peer_need = 0;
        std::vector<int> srcdev(ns, here);
        for (size_t k = 0; k < ns; k++) {
            const void *f = in.at(S->slots[k].job);
            const int dev = K.device_of(f);
            need += ic_planes_bytes(S->jobs[S->slots[k].job].image);
            if (dev >= 0) srcdev[k] = dev;
            if (srcdev[k] == here) continue;
            const void *first = nullptr;
            const size_t ext = K.peer_extent(f, &first);
            if (!ext) {
                fa_set_error("<%s %u>: its planes live on device %d, the share that converts the frame works on device %d (no peer copy on this path).",
                             K.what, S->slots[k].job, srcdev[k], here);
                return false;
            }
            peer_need += align_up(ext, 256);
        }
        if (!grow_buffer(S->up_dev[parity], S->up_dev_bytes[parity], need)
            || (peer_need && !grow_buffer(S->peer_buf, S->peer_bytes, peer_need))) {
            fa_set_error("out of HBM: no room for %.1f MiB of frames", (need + peer_need) / 1048576.0);
            return false;
        }
        if (ns * IC_ENTRY_MAX > S->ic_cap) {        /* the slots of a share only grow at staging: once per batch */
            if (S->ic_tab) (void) hipHostFree(S->ic_tab);
            if (S->d_ic) (void) hipFree(S->d_ic);
            S->ic_tab = S->d_ic = nullptr; S->ic_cap = 0;
            if (hipHostMalloc((void **) &S->ic_tab, ns * IC_ENTRY_MAX, hipHostMallocDefault) != hipSuccess
                || hipMalloc((void **) &S->d_ic, ns * IC_ENTRY_MAX) != hipSuccess) goto hip_failed;
            S->ic_cap = ns * IC_ENTRY_MAX;
        }
        if (prepare_only) return true;
        if (hipEventSynchronize(S->ev_ic) != hipSuccess) goto hip_failed;
        if (hipStreamWaitEvent(S->ustream, ready, 0) != hipSuccess) goto hip_failed;
        unsigned long long total = 0;
        size_t at = 0, peer_at = 0;
        std::vector<const int16_t *> planes(ns);
        for (size_t k = 0; k < ns; k++) {
            const void *f = in.at(S->slots[k].job);
            const void *src = nullptr;
            if (srcdev[k] != here) {
                /* a source on another device: its bytes, rows and gaps as they lie, over the peer link first */
                const void *first = nullptr;
                const size_t ext = K.peer_extent(f, &first);
                if (hipMemcpyPeerAsync(S->peer_buf + peer_at, here, first, srcdev[k], ext, S->ustream) != hipSuccess) goto hip_failed;
                src = S->peer_buf + peer_at;
                peer_at += align_up(ext, 256);
            }
            planes[k] = (const int16_t *) (S->up_dev[parity] + at);
            K.describe(S->ic_tab + k * K.entry_bytes, f, src, (int16_t *) (S->up_dev[parity] + at), total);
            at += ic_planes_bytes(S->jobs[S->slots[k].job].image);
        }
        if (hipMemcpyAsync(S->d_ic, S->ic_tab, ns * K.entry_bytes, hipMemcpyHostToDevice, S->ustream) != hipSuccess
            || hipEventRecord(S->ev_ic, S->ustream) != hipSuccess) goto hip_failed;
        if (!K.launch(S->d_ic, (unsigned) ns, total, S->ncu, S->ustream) || hipEventRecord(S->ev_up, S->ustream) != hipSuccess) goto hip_failed;
        for (size_t k = 0; k < ns; k++) {
            FrameSlot &fs = S->slots[k];
            fa_image *im = (fa_image *) S->jobs[fs.job].image;
            if (next) fs.ext_next = planes[k]; else { fs.ext_pix = planes[k]; fs.F.pix16 = planes[k]; }
            im->src_dev = planes[k]; im->src_dev_id = here; im->src_owner = S;
        }
        if (next) S->up_pending = true;
    }
    return true;
hip_failed:
    fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
    return false;
}

/* fa_image_fetch (fa_host.h): the planes of a device-fed frame into im->pixels[], which fa_image_host_planes allocated */
static int ic_fetch(fa_image *im)
{
    Staged *S = (Staged *) im->src_owner;
    const size_t npix = (size_t) im->width * im->height;
    int cur = -1, ok = 1;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    if (im->src_dev_id >= 0 && cur != im->src_dev_id) (void) hipSetDevice(im->src_dev_id);
    if (S && S->ustream) ok = hipStreamSynchronize(S->ustream) == hipSuccess;       /* the conversion may still run */
    for (int b = 0; ok && b < (im->color ? 3 : 1); b++)
        ok = hipMemcpy(im->pixels[b], im->src_dev + (size_t) b * npix, npix * 2, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
    if (cur >= 0 && im->src_dev_id >= 0 && cur != im->src_dev_id) (void) hipSetDevice(cur);
    return ok;
}

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_hip.h) */

/* `bytes' from p on: device memory, inside the allocation the pointer belongs to (the kernel reads or writes what the
 * descriptor says).  name: "<device frame 3>"; what: "pixels are", "Y plane is"; rows: "rows", "Y rows" (one: a singular,
 * "plane").  An allocation that the runtime cannot tell passes where the memory is only read (unknown == NULL) and is
 * refused where it is written: unknown names what the message then speaks of, "pixels", "Y plane".  *device: where p lives */
static bool ic_check_memory(const char *name, const char *what, const char *rows, const void *p, size_t bytes,
                            const char *unknown = nullptr, int *device = nullptr, bool one = false)
{
    hipPointerAttribute_t at;
    if (!p || hipPointerGetAttributes(&at, p) != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void) hipGetLastError();
        fa_set_error("%s: the %s not in device memory.", name, what);
        return false;
    }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t) p) != hipSuccess) {
        (void) hipGetLastError();
        if (unknown) {
            fa_set_error("%s: the device allocation of the %s cannot be determined.", name, unknown);
            return false;
        }
    } else if ((const char *) p + bytes > (const char *) base + size) {
        fa_set_error("%s: the %s %s %lu bytes beyond the end of %s device allocation.", name, rows, one ? "reaches" : "reach",
                     (unsigned long) ((const char *) p + bytes - ((const char *) base + size)), one ? "its" : "their");
        return false;
    }
    if (device) *device = at.device;
    return true;
}

/* one caller's frame (what: "device frame", or "device target" for output_convert.inc): the size rules and messages of the PNM reader, pitch, layout, and that its rows lie in device
 * memory.  *out = the frame with pitch and plane_stride filled in. */
static bool ic_check_frame(const char *what, unsigned i, const fiasco_amd_device_frame *in, fiasco_amd_device_frame *out)
{
    char name[32];
    snprintf(name, sizeof name, "<%s %u>", what, i);
    *out = *in;
    if (in->layout != FIASCO_AMD_GRAY8 && in->layout != FIASCO_AMD_RGB8_INTERLEAVED && in->layout != FIASCO_AMD_RGB8_PLANAR) {
        fa_set_error("%s: unknown pixel layout %d.", name, in->layout);
        return false;
    }
    if (!fa_image_check_size(in->width, in->height, name)) return false;
    const size_t row = ic_row_bytes(*in);
    if (!out->pitch) out->pitch = row;
    if (out->pitch < row) {
        fa_set_error("%s: pitch of %lu bytes is smaller than a row of %lu bytes.", name, (unsigned long) out->pitch, (unsigned long) row);
        return false;
    }
    if (!out->plane_stride) out->plane_stride = out->pitch * in->height;
    return ic_check_memory(name, "pixels are", "rows", in->data, ic_extent(*out));
}

static bool ic_have_device(void)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0) return true;
    (void) hipGetLastError();
    fa_set_error("libfiasco_amd: no HIP device available (the hot path has no CPU fallback)");
    return false;
}

/* the event that says "what `stream' holds now is done"; the caller destroys it (the waits hold on to what they need) */
static hipEvent_t ic_mark_ready(void *stream)
{
    hipEvent_t ev = nullptr;
    if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess || hipEventRecord(ev, (hipStream_t) stream) != hipSuccess) {
        fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
        if (ev) (void) hipEventDestroy(ev);
        return nullptr;
    }
    return ev;
}

/* the caller's stream waits for the conversions of every share: the source may then be reused in stream order */
static void ic_release_source(MultiStaged *M, void *stream)
{
    for (size_t k = 0; k < M->parts.size(); k++) {
        Staged *S = (Staged *) M->parts[k].staged;
        if (S && S->ev_up && hipStreamWaitEvent((hipStream_t) stream, S->ev_up, 0) != hipSuccess) (void) hipGetLastError();
    }
}

/* a frame of the kind's geometry without host planes (fa_image_host_planes) */
static fa_image *ic_image_of(const IcInput &in, unsigned i)
{
    fa_image *im = (fa_image *) calloc(1, sizeof(fa_image));
    if (!im) { fa_set_error("Out of memory!"); return nullptr; }
    in.kind->geometry(in.at(i), &im->width, &im->height, &im->color);
    return im;
}

/* fiasco_amd_batch_stage_device() and its YCbCr sibling behind their checks: `in' holds n checked frames */
static fiasco_amd_batch_t *ic_stage_batch(unsigned n, const IcInput &in, void *stream, float quality, const fiasco_c_options_t *options)
{
    fiasco_c_options_t *defaults = nullptr;
    const fa_options *op;
    fiasco_amd_batch_t *b = nullptr;
    hipEvent_t ready = nullptr;
    bool ok = false;

    if (options) { op = fa_cast_options(options); if (!op) return nullptr; }
    else { defaults = fiasco_c_options_new(); if (!defaults) return nullptr; op = fa_cast_options(defaults); }
    b = (fiasco_amd_batch_t *) calloc(1, sizeof *b);
    if (b) {
        b->jobs  = (fa_job *) calloc(n, sizeof *b->jobs);
        b->ims   = (fa_image **) calloc(n, sizeof *b->ims);
        b->infos = (fa_info *) calloc(n, sizeof *b->infos);
    }
    if (!b || !b->jobs || !b->ims || !b->infos) { fa_set_error("Out of memory!"); goto done; }
    b->n = n;
    b->normal_domains = op->normal_domains;
    b->delta_domains  = op->delta_domains;
    b->prediction     = op->prediction;
    for (unsigned i = 0; i < n; i++) {
        fa_cparams cp;
        b->ims[i] = ic_image_of(in, i);
        if (!b->ims[i]) goto done;
        if (!fa_setup_params(op, quality, b->ims[i]->width, b->ims[i]->height, b->ims[i]->color, 1, &b->infos[i], &cp)
            || !fa_prepare_job(&b->jobs[i], b->ims[i], &cp, op->basis_name)) goto done;
    }
    fa_image_fetch = ic_fetch;
    ready = ic_mark_ready(stream);
    if (!ready) goto done;
    b->staged = stage_shares(n, b->jobs, &in, ready);
    ic_release_source((MultiStaged *) b->staged, stream);
    ok = true;
    for (size_t k = 0; k < ((MultiStaged *) b->staged)->parts.size(); k++) {
        /* a share that could not convert its frames (no memory, a device error): NULL + message, like a PNM that
         * cannot be read.  What the device coder refuses for a frame's options stays a per-frame message. */
        const Staged *S = (const Staged *) ((MultiStaged *) b->staged)->parts[k].staged;
        if (S && S->ic_failed[0]) { fa_set_error("%s", S->ic_failed); ok = false; }
    }
done:
    if (ready) (void) hipEventDestroy(ready);
    if (defaults) fiasco_c_options_delete(defaults);
    if (!ok) { fiasco_amd_batch_free(b); b = nullptr; }
    return b;
}

extern "C" fiasco_amd_batch_t *fiasco_amd_batch_stage_device(unsigned n, const fiasco_amd_device_frame *frames, void *stream,
                                                             float quality, const fiasco_c_options_t *options)
{
    std::vector<fiasco_amd_device_frame> fr(n);
    if (!n || !frames) { fa_set_error("No frames to stage."); return nullptr; }
    if (quality <= 0) { fa_set_error("Compression quality has to be positive."); return nullptr; }
    if (!ic_have_device()) return nullptr;
    for (unsigned i = 0; i < n; i++) if (!ic_check_frame("device frame", i, &frames[i], &fr[i])) return nullptr;
    return ic_stage_batch(n, IcInput{ &IC_RGB, fr.data() }, stream, quality, options);
}

/* what an upload keeps of one share, to put it back when a share fails */
struct IcShareUndo {
    IcInput                              frames = { nullptr, nullptr };   /* the share's frames in the order of its jobs (Part::frames_of) */
    std::vector<const fa_image *>        image;     /* jobs[].image before */
    std::vector<const int16_t *>         ext_next;  /* slots[].ext_next before */
    bool up_pending = false;
    bool good = false;
    char why[256] = "";                             /* the share's message: the error message is per thread */
};

/* the staged batch takes replacement frames at all */
static bool ic_upload_ready(fiasco_amd_batch_t *b, const void *frames)
{
    if (!b || !b->staged || !b->n) { fa_set_error("Batch is not staged."); return false; }
    if (!frames) { fa_set_error("No frames to stage."); return false; }
    return true;
}

/* fiasco_amd_batch_upload_device() and its YCbCr sibling behind their checks: `in' holds b->n checked frames */
static int ic_upload_batch(fiasco_amd_batch_t *b, const IcInput &in, void *stream)
{
    MultiStaged *M = (MultiStaged *) b->staged;
    for (unsigned i = 0; i < b->n; i++) {
        const fa_image *old = b->ims[i];
        unsigned w, h;
        int color;
        in.kind->geometry(in.at(i), &w, &h, &color);
        if (w != old->width || h != old->height || (color != 0) != (old->color != 0)) {
            fa_set_error("`<%s %u>': replacement frames must keep the size and colour model of the batch.", in.kind->what, i);
            return 0;
        }
    }
    for (size_t k = 0; k < M->parts.size(); k++) {
        const Staged *S = (const Staged *) M->parts[k].staged;
        if (!S || !S->ok) { fa_set_error("Batch is not staged."); return 0; }
    }
    fa_image **nims = (fa_image **) calloc(b->n, sizeof *nims);
    hipEvent_t ready = nims ? ic_mark_ready(stream) : nullptr;
    bool ok = nims && ready;
    if (!nims) fa_set_error("Out of memory!");
    for (unsigned i = 0; ok && i < b->n; i++) {
        nims[i] = ic_image_of(in, i);
        if (!nims[i]) { ok = false; break; }
    }
    if (ok) {
        /* the shares convert the frames of THEIR jobs.  First every share gets its memory (nothing is written: a share
         * that has none refuses the upload and the batch is whole), then every share converts.  A device error after
         * that puts the slots and the images back as they were; the planes of an earlier upload that no submit had
         * taken over yet may be overwritten by then, and the error says so. */
        std::vector<IcShareUndo> sh(M->parts.size());
        for (size_t k = 0; k < M->parts.size(); k++) {
            Staged *S = (Staged *) M->parts[k].staged;
            for (unsigned j = 0; j < S->n; j++) {
                sh[k].image.push_back(S->jobs[j].image);
                S->jobs[j].image = nims[M->parts[k].job_index(j)];
            }
            sh[k].frames = M->parts[k].frames_of(in);
            for (size_t j = 0; j < S->slots.size(); j++) sh[k].ext_next.push_back(S->slots[j].ext_next);
            sh[k].up_pending = S->up_pending;
        }
        /* one step of every share; false and the message of a share that failed */
        auto all_shares = [&](bool prepare_only) {
            for_each_share(M, [&](size_t k) {
                Staged *S = (Staged *) M->parts[k].staged;
                sh[k].good = ic_convert(S, sh[k].frames, S->up_parity ^ 1, ready, true, prepare_only);
                if (!sh[k].good) snprintf(sh[k].why, sizeof sh[k].why, "%s", fiasco_get_error_message());
            });
            bool all = true;
            for (size_t k = 0; k < M->parts.size(); k++)
                if (!sh[k].good) {
                    all = false;
                    fa_set_error("%s%s", sh[k].why, !prepare_only && sh[k].up_pending ? " (the frames of the upload before, not yet submitted, are lost)" : "");
                }
            return all;
        };
        ok = all_shares(true);
        const bool touched = ok;
        if (ok) ok = all_shares(false);
        if (!ok)
            for (size_t k = 0; k < M->parts.size(); k++) {
                Staged *S = (Staged *) M->parts[k].staged;
                for (unsigned j = 0; j < S->n; j++) S->jobs[j].image = sh[k].image[j];
                for (size_t j = 0; touched && j < S->slots.size(); j++) S->slots[j].ext_next = sh[k].ext_next[j];
                if (touched) S->up_pending = sh[k].up_pending;
            }
        ic_release_source(M, stream);
    }
    if (ready) (void) hipEventDestroy(ready);
    if (!ok) {
        if (nims) for (unsigned i = 0; i < b->n; i++) free(nims[i]);
        free(nims);
        return 0;
    }
    fa_image_fetch = ic_fetch;
    if (b->prev_ims) {
        for (unsigned i = 0; i < b->n; i++) fa_image_free(b->prev_ims[i]);
        free(b->prev_ims);
    }
    b->prev_ims = b->ims;                      /* alive until the next upload */
    b->ims = nims;
    for (unsigned i = 0; i < b->n; i++) b->jobs[i].image = nims[i];
    return 1;
}

extern "C" int fiasco_amd_batch_upload_device(fiasco_amd_batch_t *b, const fiasco_amd_device_frame *frames, void *stream)
{
    if (!ic_upload_ready(b, frames)) return 0;
    std::vector<fiasco_amd_device_frame> fr(b->n);
    for (unsigned i = 0; i < b->n; i++) if (!ic_check_frame("device frame", i, &frames[i], &fr[i])) return 0;
    return ic_upload_batch(b, IcInput{ &IC_RGB, fr.data() }, stream);
}

/* ------------------------------------------------------------------ videos in device memory
 *
 * fiasco_amd_seq_open_device(): the frames of a video as they lie in device memory.  Open converts ONCE every frame this
 * rank will ever search -- the frames of its groups of pictures and display frame 0, which fa_seq_probe searches on
 * every rank -- into int16 planes in a buffer the sequence owns, on the device of the share that searches the frame's
 * GOP (fa_share_of(gop + 1, ., shares); frame 0: share 0, where the probe runs and where GOP 0 is searched).  One launch
 * of the kind's kernel per share.  Open waits on the host for the conversions: the searches that follow have no ordering
 * question left, and the caller's stream is made to wait as well.  A search then stages the planes in place
 * (FrameSlot::ext_pix, core1_stage). */
struct SeqPlanes { std::vector<std::pair<int, void *> > bufs; };     /* (device, allocation) */

static void seq_planes_release(void *ctx)
{
    SeqPlanes *P = (SeqPlanes *) ctx;
    if (!P) return;
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    for (size_t k = 0; k < P->bufs.size(); k++) {
        if (P->bufs[k].first >= 0 && P->bufs[k].first != cur) (void) hipSetDevice(P->bufs[k].first);
        (void) hipFree(P->bufs[k].second);
        if (P->bufs[k].first >= 0 && P->bufs[k].first != cur && cur >= 0) (void) hipSetDevice(cur);
    }
    delete P;
}

/* what every open of a video refuses before it looks at a frame */
static bool ic_seq_open_ready(unsigned n, const void *frames, float quality, unsigned rank, unsigned world)
{
    if (!n || !frames) { fa_set_error("No frames to open."); return false; }
    if (quality <= 0) { fa_set_error("Compression quality has to be positive."); return false; }
    if (world == 0 || rank >= world) { fa_set_error("rank %d of %d?", (int) rank, (int) world); return false; }
    return ic_have_device();
}

/* fiasco_amd_seq_open_device() and its YCbCr sibling behind their checks: `in' holds n checked frames */
static fiasco_amd_seq_t *ic_seq_open(unsigned n, const IcInput &in, void *stream, float quality, const fiasco_c_options_t *options,
                                     unsigned rank, unsigned world)
{
    const IcKind &K = *in.kind;
    std::vector<int> srcdev(n, -1);
    for (unsigned i = 0; i < n; i++) srcdev[i] = K.device_of(in.at(i));
    fiasco_c_options_t *defaults = nullptr;
    const fa_options *op;
    if (options) { op = fa_cast_options(options); if (!op) return nullptr; }
    else { defaults = fiasco_c_options_new(); if (!defaults) return nullptr; op = fa_cast_options(defaults); }
    /* the sequence engine: sizes and colour models, the coding order, the groups of pictures (nothing on a device yet) */
    fa_image **images = (fa_image **) calloc(n, sizeof *images);
    bool ok = images != nullptr;
    for (unsigned i = 0; ok && i < n; i++) {
        images[i] = ic_image_of(in, i);
        if (!images[i]) { ok = false; break; }
        images[i]->src_dev_id = -1;
    }
    if (!ok) {
        for (unsigned i = 0; images && i < n; i++) fa_image_free(images[i]);
        free(images);
        if (defaults) fiasco_c_options_delete(defaults);
        fa_set_error("Out of memory!");
        return nullptr;
    }
    fa_seq *s = fa_seq_open_images(op, quality, n, images, rank, world);       /* takes the images, also when it refuses */
    fiasco_amd_seq_t *q = s ? fa_seq_handle(s, defaults) : nullptr;
    if (!q) {
        fa_seq_free(s);
        if (defaults) fiasco_c_options_delete(defaults);
        return nullptr;
    }
    /* which frames, on which share */
    resolve_devices();
    const size_t D = g_devices.size();
    std::vector<std::vector<unsigned> > mine(D);
    std::vector<unsigned char> taken(n, 0);
    for (unsigned k = 0; k < fa_seq_frames(s); k++) {
        const unsigned g = fa_seq_gop_of(s, k), d = fa_seq_display_of(s, k);
        if (!fa_seq_is_mine(s, g) && d != 0) continue;
        if (taken[d]) continue;
        taken[d] = 1;
        mine[fa_share_of(g + 1, 0, (unsigned) D)].push_back(d);
    }
    const size_t frame_b = ic_planes_bytes(images[0]);
    SeqPlanes *P = new SeqPlanes;
    hipEvent_t ready = ic_mark_ready(stream);
    std::vector<size_t> share;
    for (size_t k = 0; k < D; k++) if (!mine[k].empty()) share.push_back(k);
    std::vector<std::string> why(share.size());
    std::vector<void *> got(share.size(), nullptr);
    std::vector<int> gotdev(share.size(), -1);
    std::vector<hipEvent_t> done(share.size(), nullptr);
    if (ready)
        for_shares(share, [&](size_t part) {
            const std::vector<unsigned> &ds = mine[share[part]];
            int here = -1;
            hipStream_t st = nullptr;
            char *buf = nullptr;
            char *d_tab = nullptr;
            std::vector<char> tab(ds.size() * K.entry_bytes);
            unsigned long long total = 0;
            auto fail = [&](const char *msg) { why[part] = msg; (void) hipGetLastError(); };
            if (hipGetDevice(&here) != hipSuccess) { fail("HIP error: no current device"); return; }
            for (unsigned d : ds)
                if (srcdev[d] != here) {
                    char msg[200];
                    snprintf(msg, sizeof msg, "<%s %u>: the pixels live on device %d, its group of pictures is searched on device %d "
                             "(no peer copy on this path).", K.what, d, srcdev[d], here);
                    why[part] = msg;
                    return;
                }
            if (hipMalloc((void **) &buf, frame_b * ds.size()) != hipSuccess) {
                char msg[200];
                snprintf(msg, sizeof msg, "out of HBM: no room for %.1f MiB of frames", frame_b * ds.size() / 1048576.0);
                (void) hipGetLastError();
                why[part] = msg;
                return;
            }
            got[part] = buf; gotdev[part] = here;
            for (size_t j = 0; j < ds.size(); j++) K.describe(tab.data() + j * K.entry_bytes, in.at(ds[j]), nullptr, (int16_t *) (buf + j * frame_b), total);
            bool fine = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess
                        && hipEventCreateWithFlags(&done[part], hipEventDisableTiming) == hipSuccess
                        && hipMalloc((void **) &d_tab, tab.size()) == hipSuccess
                        && hipStreamWaitEvent(st, ready, 0) == hipSuccess
                        && hipMemcpyAsync(d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice, st) == hipSuccess
                        && K.launch(d_tab, (unsigned) ds.size(), total, ft_cus(), st)
                        && hipEventRecord(done[part], st) == hipSuccess
                        && hipStreamSynchronize(st) == hipSuccess;          /* the one host wait of open */
            if (!fine) { why[part] = std::string("HIP error: ") + hipGetErrorString(hipGetLastError()); }
            if (d_tab) (void) hipFree(d_tab);
            if (st) (void) hipStreamDestroy(st);
            if (fine)
                for (size_t j = 0; j < ds.size(); j++) {
                    fa_image *im = fa_seq_image(s, ds[j]);
                    im->src_dev = (const int16_t *) (buf + j * frame_b); im->src_dev_id = here; im->src_owner = nullptr;
                }
        });
    ok = ready != nullptr;
    for (size_t k = 0; k < share.size(); k++) {
        if (got[k]) P->bufs.push_back(std::make_pair(gotdev[k], got[k]));
        if (done[k]) {
            /* the caller's stream behind the conversions: the sources may be overwritten or freed in stream order */
            if (hipStreamWaitEvent((hipStream_t) stream, done[k], 0) != hipSuccess) (void) hipGetLastError();
            (void) hipEventDestroy(done[k]);
        }
        if (!why[k].empty()) { fa_set_error("%s", why[k].c_str()); ok = false; }
    }
    if (ready) (void) hipEventDestroy(ready);
    fa_seq_on_free(s, seq_planes_release, P);
    fa_image_fetch = ic_fetch;
    if (!ok) {
        std::string msg = fiasco_get_error_message();
        fiasco_amd_seq_free(q);                     /* gives the buffers back */
        fa_set_error("%s", msg.c_str());
        return nullptr;
    }
    return q;
}

extern "C" fiasco_amd_seq_t *fiasco_amd_seq_open_device(unsigned n, const fiasco_amd_device_frame *frames, void *stream, float quality,
                                                        const fiasco_c_options_t *options, unsigned rank, unsigned world)
{
    if (!ic_seq_open_ready(n, frames, quality, rank, world)) return nullptr;
    std::vector<fiasco_amd_device_frame> fr(n);
    for (unsigned i = 0; i < n; i++) if (!ic_check_frame("device frame", i, &frames[i], &fr[i])) return nullptr;
    return ic_seq_open(n, IcInput{ &IC_RGB, fr.data() }, stream, quality, options, rank, world);
}
