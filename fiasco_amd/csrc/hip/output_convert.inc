/*
 *  output_convert.inc -- decoded frames as 8-bit pixels in device memory (included by core_hip.cpp between
 *  input_convert.inc, whose mirror image this is, and frame_decoder.inc, whose flights launch it).
 *
 *  The device decoder leaves the planes [bands][height][width] of a frame in HBM as 12.4 fixed point.  Its other
 *  outlets copy them to the host; here ONE launch of oc_convert_kernel per decoder flight turns the planes of all
 *  frames of the flight into the bytes the reference's write_image puts into a PGM / PPM (`dfiasco -s 0 -o'), inside
 *  buffers the caller owns: gray, interleaved R, G, B or three planes.  No pixel crosses to the host.
 *
 *  Arithmetic: the reference's (lib/image.c), integer results, arithmetic shift (HAVE_SIGNED_SHIFT, as the decoder):
 *    gray    clip255((p >> 4) + 128)                                              gray_write  :450-480
 *    colour  yval = (Y >> 4) + 128, cb = clamp(Cb >> 4, -128, 127), cr likewise   color_write :534-582
 *            R = clip255(yval + T_rr[cr]), G = clip255(yval + T_rg[cr] + T_bg[cb]), B = clip255(yval + T_bb[cb])
 *            T_x[v] = (int) (k * v + 0.5) in double, truncated toward zero, k = 1.4022, -0.7145, -0.3456, 1.7710
 *                                                                                 init_chroma_tables :487-532
 *  The four table entries of a pixel are evaluated where they are needed -- a multiplication, an addition and a
 *  conversion in double each, written as the reference writes them; nothing may be contracted into a fused
 *  multiply-add (-ffp-contract=off, and the function says so again).  The kernel moves 3 bytes per pixel and band and
 *  is bound by that.
 *  clip255 and the clamp of the chroma values are the mathematical ones.  The reference reads tables of finite size:
 *  its clip table spans -256 .. 511 (lib/misc.c:318-347), its chroma tables -384 .. 383 with the end values repeated
 *  beyond -128 .. 127.  Wherever its indices stay inside them the two agree; outside the reference reads past its
 *  arrays, and this code clamps.
 *
 *  Shape: frame_table.inc's -- one table entry per frame (OcFrame), one sequence of work items.  A work item is 16
 *  neighbouring pixels of one row -- two 16-byte loads per band where the row of the plane allows it (a row of odd
 *  width / 8 does not start on 16 bytes: 8-, 4- or 2-byte loads then), one 16-byte store for gray and per plane, three
 *  for interleaved RGB, byte stores at a ragged row end or an unaligned target.
 *
 *  Build (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): oc_convert_kernel 65 VGPRs, 51 SGPRs,
 *  no scratch, no LDS, 7 waves per SIMD; global_ accesses only.
 */

struct OcFrame {
    const int16_t      *src;         /* planes [bands][height][width] */
    unsigned char      *dst;         /* first pixel */
    unsigned long long  pitch, plane_stride;
    unsigned long long  first;       /* work items of the frames before this one */
    unsigned            width, height, layout, cpr;    /* cpr: items per row */
};

/* byte k of 16 in four words that begin as zero */
PX_DEV void oc_put(unsigned *w, unsigned k, unsigned byte) { w[k >> 2] |= byte << (8 * (k & 3)); }

/* work item `local' of frame F */
PX_DEV void oc_item(const OcFrame &F, unsigned local)
{
#pragma clang fp contract(off)
    const unsigned row = local / F.cpr, x0 = (local - row * F.cpr) * 16;
    const unsigned n = F.width - x0 < 16 ? F.width - x0 : 16;
    const size_t npix = (size_t) F.width * F.height;
    const int16_t *p = F.src + (size_t) row * F.width + x0;
    unsigned char *q = F.dst + (size_t) row * F.pitch;
    unsigned y[8];
    px_load_values(p, n, y);
    if (F.layout == FIASCO_AMD_GRAY8) {
        unsigned w[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (unsigned k = 0; k < 16; k++) oc_put(w, k, px_clip255(px_int(y, k) + 128));
        px_store_bytes_vec(q + x0, n, w);
        return;
    }
    unsigned cbv[8], crv[8];
    px_load_values(p + npix, n, cbv);
    px_load_values(p + 2 * npix, n, crv);
    unsigned w[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
    for (unsigned k = 0; k < 16; k++) {
        const int yval = px_int(y, k) + 128;
        int cb = px_int(cbv, k), cr = px_int(crv, k);
        cb = cb < -128 ? -128 : cb > 127 ? 127 : cb;
        cr = cr < -128 ? -128 : cr > 127 ? 127 : cr;
        /* lib/image.c:508-511, character for character: double arithmetic, C truncation */
        const int rr = (int) ( 1.4022 * cr + 0.5);
        const int rg = (int) (-0.7145 * cr + 0.5);
        const int bg = (int) (-0.3456 * cb + 0.5);
        const int bb = (int) ( 1.7710 * cb + 0.5);
        const unsigned r = px_clip255(yval + rr), g = px_clip255(yval + rg + bg), bl = px_clip255(yval + bb);
        if (F.layout == FIASCO_AMD_RGB8_INTERLEAVED) { oc_put(w, 3 * k, r); oc_put(w, 3 * k + 1, g); oc_put(w, 3 * k + 2, bl); }
        else { oc_put(w, k, r); oc_put(w + 4, k, g); oc_put(w + 8, k, bl); }
    }
    if (F.layout == FIASCO_AMD_RGB8_INTERLEAVED) {
        unsigned char *d = q + (size_t) x0 * 3;
        const unsigned nb = n * 3;
        px_store_bytes_vec(d, nb >= 16 ? 16 : nb, w);
        px_store_bytes_vec(d + 16, nb >= 32 ? 16 : nb > 16 ? nb - 16 : 0, w + 4);
        px_store_bytes_vec(d + 32, nb >= 48 ? 16 : nb > 32 ? nb - 32 : 0, w + 8);
    } else {
        px_store_bytes_vec(q + x0, n, w);
        px_store_bytes_vec(q + F.plane_stride + x0, n, w + 4);
        px_store_bytes_vec(q + 2 * F.plane_stride + x0, n, w + 8);
    }
}

__global__ void __launch_bounds__(256) oc_convert_kernel(const OcFrame *__restrict__ frames, unsigned nframes, unsigned long long total)
{
    ft_walk<oc_item>(frames, nframes, total);
}

/* ------------------------------------------------------------------ launching */

/* what the decoder is told about the batch call it serves: frame i of the jobs goes to target[i] (checked, pitch and
 * plane stride filled in) and nowhere else -- no host image, no copy to the host; done[i] = 1 once it is written */
struct OcOut {
    const fiasco_amd_device_frame *target;      /* [n] by job index; data == NULL: the job is skipped anyway */
    unsigned char *done;                        /* [n] */
    hipEvent_t     ready;                       /* what the caller's stream held at the call */
    hipStream_t    caller;                      /* made to wait for the conversions */
    /* thumbnails beside the frames (fiasco_amd_batch_decode_device_thumbnails): thumb == NULL: none */
    const fiasco_amd_device_frame *thumb = nullptr;     /* [n] by job index, of the size at magnification -reduce; data == NULL: none */
    unsigned char *thumb_done = nullptr;                /* [n] */
    unsigned       reduce = 0;
    /* display surfaces instead of 8-bit pixels (fiasco_amd_batch_decode_device_rendered, render.inc): target[] describes
     * the surfaces (width, height: the frame's) and the flight launches rd_render_kernel; NULL: oc_convert_kernel */
    const fiasco_amd_renderer *render = nullptr;
    /* 4:2:0 buffers instead (fiasco_amd_batch_decode_device_420, output_convert_420.inc): t420[] are the checked targets
     * by job index, target[] only says which frames are wanted, and the flight launches oc420_convert_kernel.  With
     * `render' set as well (fiasco_amd_batch_decode_device_rendered_420, render_420.inc) t420[i].y, y_pitch, width and
     * height describe the checked surface of frame i, and the flight launches rd420_render_kernel */
    const fiasco_amd_device_target_420 *t420 = nullptr;
    /* the shown planes themselves instead (the images of a decoder, decoder_outlet.inc): target[] only says which frames are
     * wanted (ready and caller are not used: nobody else knows the buffers).  planes[i] is a buffer of planes_bytes bytes on
     * device planes_dev[i], made BEFORE the call; the flight copies the planes the other consumers would read -- smoothed
     * where smoothing applies, 4:4:4 or 4:2:0 as the jobs say -- into it on its stream, and allocates nothing.  A frame
     * whose values do not fill the buffer exactly, or that is decoded on another device, fails */
    int16_t *const *planes = nullptr;                   /* [n] */
    const int      *planes_dev = nullptr;               /* [n] */
    size_t          planes_bytes = 0;
    /* what a share keeps between calls for a caller that comes again (a decoder): see DecKeep, frame_decoder.inc */
    struct DecKeep *keep = nullptr;
};

static void oc_describe(OcFrame &d, const int16_t *planes, const fiasco_amd_device_frame &t, unsigned long long &total)
{
    d.src = planes; d.dst = (unsigned char *) t.data;
    d.pitch = t.pitch; d.plane_stride = t.plane_stride; d.first = total;
    d.width = t.width; d.height = t.height; d.layout = (unsigned) t.layout; d.cpr = (t.width + 15) / 16;
    total += (unsigned long long) d.cpr * t.height;
}

static bool oc_launch(const OcFrame *d_tab, unsigned n, unsigned long long total, int ncu, hipStream_t stream)
{
    return ft_launch(oc_convert_kernel, d_tab, n, total, ncu, stream);
}

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_hip.h) */

/* a caller's target for a frame of width x height (color): ic_check_frame's rules -- device memory, pitch, rows inside
 * the allocation -- and that size and layout are the frame's.  *out: the target with pitch and plane stride filled in */
static bool oc_check_target(unsigned i, const fiasco_amd_device_target *in, unsigned width, unsigned height, int color,
                            fiasco_amd_device_frame *out, int *device, unsigned coded_w = 0, unsigned coded_h = 0, int magnify = 0)
{
    fiasco_amd_device_frame t;
    t.data = in->data; t.pitch = in->pitch; t.plane_stride = in->plane_stride;
    t.width = in->width; t.height = in->height; t.layout = in->layout;
    if (!ic_check_frame("device target", i, &t, out)) return false;
    if (in->width != width || in->height != height) {
        if (magnify) fa_set_error("<device target %u>: %u x %u pixels for a frame of %u x %u at magnification %d: %u x %u.", i, in->width, in->height,
                                  coded_w, coded_h, magnify, width, height);
        else fa_set_error("<device target %u>: %u x %u pixels for a frame of %u x %u.", i, in->width, in->height, width, height);
        return false;
    }
    if ((in->layout != FIASCO_AMD_GRAY8) != (color != 0)) {
        fa_set_error("<device target %u>: the layout contradicts the colour model of the frame (GRAY8 for gray, RGB8 for colour).", i);
        return false;
    }
    /* these rows are WRITTEN: a target whose allocation cannot be told (ic_check_frame lets that pass) is refused */
    char name[32];
    snprintf(name, sizeof name, "<device target %u>", i);
    return ic_check_memory(name, "pixels are", "rows", in->data, ic_extent(*out), "pixels", device);
}

/* What the two batch entry points (this one and fiasco_amd_batch_decode_distortion_device, distortion.inc) have in
 * common: the batch has a finished pass; every finished intra frame becomes a job of the decoder, the others are
 * skipped; a frame with a target (targets may be NULL) has it checked and lives where the frame will be decoded.
 * who: the entry point, for the messages; refuse: what it holds against its own arguments, if anything.
 * magnify: the frames are decoded at that magnification (fa_dec_job.magnify) and the targets have that size; a frame
 * the size rule refuses at it refuses the call.  thumbs, reduce: NULL, or a second set of targets of the size at
 * magnification -reduce, checked the same way (B.thumb). */
struct OcBatch {
    std::vector<fa_dec_job> jobs;                         /* [n]; skip = 1: no finished intra frame */
    std::vector<fiasco_amd_device_frame> target;          /* [n] checked, pitch and plane stride filled in; data == NULL: none */
    std::vector<fiasco_amd_device_frame> thumb;           /* [n] likewise */
    std::vector<int> device;                              /* [n] the device the job is decoded on */
};

/* one target of frame i, to be decoded on device `dev', at `magnify' */
static bool oc_batch_target(unsigned i, const fiasco_amd_device_target *in, const fa_image *im, int magnify, int dev, fiasco_amd_device_frame *out)
{
    unsigned w = im->width, h = im->height;
    int tdev = -1;
    if (magnify && !fiasco_amd_magnified_size(im->width, im->height, magnify, &w, &h)) return false;
    if (!oc_check_target(i, in, w, h, im->color, out, &tdev, im->width, im->height, magnify)) return false;
    if (tdev != dev) {
        fa_set_error("<device target %u>: the target lives on device %d, the frame is decoded on device %d (no peer copy on this path).", i, tdev, dev);
        return false;
    }
    return true;
}

static bool oc_batch_jobs(const char *who, const char *refuse, const fiasco_amd_batch_t *b, const fiasco_amd_device_target *targets, OcBatch &B,
                          int magnify = 0, const fiasco_amd_device_target *thumbs = nullptr, unsigned reduce = 0)
{
    if (!b || !b->n) { fa_set_error("%s: empty batch", who); return false; }
    if (refuse) { fa_set_error("%s: %s", who, refuse); return false; }
    if (!ic_have_device()) return false;
    const unsigned n = b->n;
    bool finished = false;
    for (unsigned i = 0; i < n; i++) finished = finished || (b->jobs[i].status && b->jobs[i].wfa);
    if (!finished) { fa_set_error("%s: the batch has no finished pass", who); return false; }
    B.jobs.assign(n, fa_dec_job()); B.target.assign(n, fiasco_amd_device_frame()); B.thumb.assign(n, fiasco_amd_device_frame()); B.device.assign(n, -1);
    const size_t shares = dec_shares(n, B.jobs.data());
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    for (unsigned i = 0; i < n; i++) {
        const fa_job *job = &b->jobs[i];
        fa_dec_job &d = B.jobs[i];
        fa_dec_job_of(job, magnify, &d);
        if (d.skip) continue;
        B.device[i] = dec_device_of(B.jobs.data(), i, shares, cur);
        if (magnify && !fiasco_amd_magnified_size(job->image->width, job->image->height, magnify, nullptr, nullptr)) return false;
        if (targets && targets[i].data && !oc_batch_target(i, &targets[i], job->image, magnify, B.device[i], &B.target[i])) return false;
        if (thumbs && thumbs[i].data && !oc_batch_target(i, &thumbs[i], job->image, -(int) reduce, B.device[i], &B.thumb[i])) return false;
    }
    return true;
}

/* the three batch entries: the frames with a target (checked, in B) through the decoder, each at the magnification of
 * its job, and with reduce != 0 the thumbnails of B.thumb beside them */
static int oc_decode_batch(const char *who, const fiasco_amd_batch_t *b, OcBatch &B, unsigned reduce, void *stream, const fiasco_amd_renderer *render = nullptr,
                           const fiasco_amd_device_target_420 *t420 = nullptr)
{
    const unsigned n = b->n;
    std::vector<unsigned char> done(n, 0), thumb_done(n, 0);
    unsigned wanted = 0;
    for (unsigned i = 0; i < n; i++) {
        if (!B.target[i].data && !B.thumb[i].data) B.jobs[i].skip = 1;     /* a frame without a target is skipped */
        wanted += !B.jobs[i].skip;
    }
    if (!wanted) { fa_set_error("%s: no frame with a finished intra automaton and a target", who); return 0; }
    OcOut out;
    out.target = B.target.data(); out.done = done.data(); out.caller = (hipStream_t) stream;
    if (reduce) { out.thumb = B.thumb.data(); out.thumb_done = thumb_done.data(); out.reduce = reduce; }
    out.render = render; out.t420 = t420;
    out.ready = ic_mark_ready(stream);
    if (!out.ready) return 0;
    const int good = decode_frames(n, B.jobs.data(), &out, nullptr);
    (void) hipEventDestroy(out.ready);
    for (unsigned i = 0; i < n; i++)
        if (!B.jobs[i].skip && ((B.target[i].data && !done[i]) || (B.thumb[i].data && !thumb_done[i])))
            fa_set_error("<device target %u>: %s", i, B.jobs[i].errmsg[0] ? B.jobs[i].errmsg : "decoder failed");
    return good;
}

extern "C" int fiasco_amd_batch_decode_device(const fiasco_amd_batch_t *b, const fiasco_amd_device_target *targets, void *stream)
{
    OcBatch B;
    if (!oc_batch_jobs("fiasco_amd_batch_decode_device", targets ? nullptr : "no targets", b, targets, B)) return 0;
    return oc_decode_batch("fiasco_amd_batch_decode_device", b, B, 0, stream);
}

extern "C" int fiasco_amd_batch_decode_device_magnified(const fiasco_amd_batch_t *b, int magnify, const fiasco_amd_device_target *targets, void *stream)
{
    OcBatch B;
    if (!oc_batch_jobs("fiasco_amd_batch_decode_device_magnified", targets ? nullptr : "no targets", b, targets, B, magnify)) return 0;
    return oc_decode_batch("fiasco_amd_batch_decode_device_magnified", b, B, 0, stream);
}

extern "C" int fiasco_amd_batch_decode_device_thumbnails(const fiasco_amd_batch_t *b, const fiasco_amd_device_target *targets, unsigned reduce,
                                                         const fiasco_amd_device_target *thumbs, void *stream)
{
    OcBatch B;
    const char *refuse = !thumbs ? "no thumbnails" : !reduce ? "a reduction of at least 1 (half the side length) is needed" : reduce > 15 ? "reduction out of range" : nullptr;
    if (!oc_batch_jobs("fiasco_amd_batch_decode_device_thumbnails", refuse, b, targets, B, 0, thumbs, reduce)) return 0;
    return oc_decode_batch("fiasco_amd_batch_decode_device_thumbnails", b, B, reduce, stream);
}

extern "C" int fiasco_amd_planes_to_pixels_device(const int16_t *planes, int color, const fiasco_amd_device_target *target, void *stream)
{
    if (!planes || !target || !target->data) { fa_set_error("fiasco_amd_planes_to_pixels_device: no planes or no target"); return 0; }
    if (!ic_have_device()) return 0;
    fiasco_amd_device_frame t;
    int tdev = -1, pdev = -1;
    if (!oc_check_target(0, target, target->width, target->height, color, &t, &tdev)) return 0;
    const size_t bytes = (size_t) t.width * t.height * (color ? 3 : 1) * 2;
    if (!ic_check_memory("fiasco_amd_planes_to_pixels_device", "planes are", "planes", planes, bytes, nullptr, &pdev)) return 0;
    if (pdev != tdev) {
        fa_set_error("<device target 0>: the target lives on device %d, the planes on device %d (no peer copy on this path).", tdev, pdev);
        return 0;
    }
    OcFrame h;
    unsigned long long total = 0;
    oc_describe(h, planes, t, total);
    return ft_run_alone(&h, sizeof h, [&](const void *d_tab, int ncu) { return oc_launch((const OcFrame *) d_tab, 1, total, ncu, (hipStream_t) stream); },
                        tdev, (hipStream_t) stream);
}

/* ------------------------------------------------------------------ the outputs of a video
 *
 * fiasco_amd_seq_set_outputs_device(): from now on every search of the sequence reconstructs every frame of the GOPs it
 * searches and the decoder's flights deliver it (fa_dec_job's consumer fields, frame_decoder.inc).  Every target is
 * checked here, before any launch, by the rules of fiasco_amd_batch_decode_device(); the device it must live on is the
 * one of the share that decodes the frame's group of pictures. */
extern "C" int fiasco_amd_seq_set_outputs_device(fiasco_amd_seq_t *seq, const fiasco_amd_seq_outputs *o)
{
    fa_seq *s = fa_seq_of_handle(seq);
    if (!s) { fa_set_error("fiasco_amd_seq_set_outputs_device: no sequence"); return 0; }
    if (!o || (!o->targets && !o->sse && !o->maxdiff)) { fa_seq_set_outputs(s, nullptr, 0, nullptr, nullptr, nullptr, nullptr); return 1; }
    if (!ic_have_device()) return 0;
    unsigned w = 0, h = 0;
    int color = 0, cur = -1;
    fa_seq_size(s, &w, &h, &color);
    resolve_devices();
    const size_t D = g_devices.size();
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    for (unsigned k = 0; o->targets && k < fa_seq_frames(s); k++) {
        const unsigned d = fa_seq_display_of(s, k);
        if (!o->targets[d].data) continue;
        fiasco_amd_device_frame checked;
        int tdev = -1, dev = g_devices[fa_share_of(fa_seq_gop_of(s, k) + 1, 0, (unsigned) D)];
        if (dev < 0) dev = cur;
        if (!oc_check_target(d, &o->targets[d], w, h, color, &checked, &tdev)) return 0;
        if (tdev != dev) {
            fa_set_error("<device target %u>: the target lives on device %d, the frame is decoded on device %d (no peer copy on this path).", d, tdev, dev);
            return 0;
        }
    }
    if (o->written) memset(o->written, 0, fa_seq_nframes(s));
    fa_seq_set_outputs(s, o->targets, sizeof(fiasco_amd_device_target), o->sse, o->maxdiff, o->written, o->stream);
    return 1;
}
