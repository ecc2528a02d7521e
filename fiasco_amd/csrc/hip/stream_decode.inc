/*
 *  stream_decode.inc -- the frames of a .fco stream that was read, into the caller's device buffers (included by
 *  core_hip.cpp behind frame_decoder.inc; include/libfiasco_amd_stream.h).
 *
 *  The walk is the host's (fa_stream_walk, csrc/host/fa_stream.c): it hands over the frames whose reference frames are
 *  decoded, as decoder jobs with from_stream set.  Here every such call becomes one decode_frames() with the targets of
 *  the frames that are wanted attached as the batch entries attach theirs (OcOut): an all-intra stream runs in the
 *  usual flights, a run of B frames as one flight where B_as_past_ref is 0 (with the default of 1 every later B frame is
 *  predicted from the one before it: one frame per flight), a chain of P frames one frame per flight.  No frame comes to the host:
 *  a frame somebody is predicted from keeps its planes on the device (keep_dev), the others leave nothing behind.
 *  All jobs carry one share key, so a stream decodes on one device; the targets are checked against that device before
 *  the first launch.
 */
struct StreamRun {
    const fiasco_amd_device_frame *target;          /* [count] by display - first, checked; data == NULL: not wanted */
    const fiasco_amd_device_target_420 *t420;       /* the same for a 4:2:0 call (target[].data then only says "wanted"), or nullptr */
    unsigned first;
    hipStream_t caller;
    hipEvent_t ready;
};

static void stream_run(void *ctx, unsigned n, fa_dec_job *jobs, const unsigned *display, const uint8_t *wanted)
{
    const StreamRun *R = (const StreamRun *) ctx;
    std::vector<fiasco_amd_device_frame> target(n, fiasco_amd_device_frame());
    std::vector<fiasco_amd_device_target_420> t420(n, fiasco_amd_device_target_420());
    std::vector<unsigned char> done(n, 0);
    for (unsigned i = 0; i < n; i++) {
        if (!wanted[i]) continue;
        target[i] = R->target[display[i] - R->first];
        if (R->t420) t420[i] = R->t420[display[i] - R->first];
    }
    OcOut out;
    out.target = target.data(); out.done = done.data(); out.caller = R->caller; out.ready = R->ready;
    if (R->t420) out.t420 = t420.data();
    (void) decode_frames(n, jobs, &out, nullptr, false);
    /* a frame that was decoded and not written did not succeed */
    for (unsigned i = 0; i < n; i++)
        if (jobs[i].out && target[i].data && !done[i]) {
            fa_image_free(jobs[i].out);
            dec_fail(&jobs[i], "device decoder: the frame was not written");
        }
}

/* the device a walked stream decodes on: the share of its one key */
static int stream_device()
{
    fa_dec_job probe = fa_dec_job();
    int cur = -1;
    probe.share_key = 1;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    return dec_device_of(&probe, 0, dec_shares(1, &probe), cur);
}

static int stream_decode(const char *who, const fiasco_amd_stream_t *s, unsigned first, unsigned count, int magnify, int smoothing,
                         const fiasco_amd_device_target *targets, const fiasco_amd_device_target_420 *targets420, void *stream)
{
    if (!s) { fa_set_error("%s: no stream", who); return 0; }
    const fa_info *wi = fa_stream_info(s);
    const char *refuse = targets || targets420 ? sm_refuse(smoothing) : "no targets";
    if (!count || first >= wi->frames || count > wi->frames - first) refuse = "no such frames";
    if (refuse) { fa_set_error("%s: %s", who, refuse); return 0; }
    unsigned w = wi->width, h = wi->height;
    if (magnify && !fiasco_amd_magnified_size(wi->width, wi->height, magnify, &w, &h)) return 0;
    if (targets420 && !wi->color) { fa_set_error("%s: 4:2:0: a gray frame has no chroma bands", who); return 0; }
    std::vector<fiasco_amd_device_frame> checked(count, fiasco_amd_device_frame());
    std::vector<fiasco_amd_device_target_420> checked420(targets420 ? count : 0, fiasco_amd_device_target_420());
    for (unsigned i = 0; targets420 && i < count; i++)
        if (targets420[i].y && !y4_check_geometry(i, &targets420[i], w, h, &checked420[i], wi->width, wi->height, magnify)) return 0;
    if (!ic_have_device()) return 0;
    const int dev = stream_device();
    unsigned wantedn = 0;
    for (unsigned i = 0; i < count; i++) {
        int tdev = -1;
        if (targets420) {
            if (!targets420[i].y) continue;
            if (!y4_check_memory(i, checked420[i], &tdev)) return 0;
            checked[i].data = checked420[i].y; checked[i].width = w; checked[i].height = h;
        } else {
            if (!targets[i].data) continue;
            if (!oc_check_target(i, &targets[i], w, h, wi->color, &checked[i], &tdev, wi->width, wi->height, magnify)) return 0;
        }
        if (tdev != dev) {
            fa_set_error("<%s %u>: the target lives on device %d, the frame is decoded on device %d (no peer copy on this path).",
                         targets420 ? "4:2:0 target" : "device target", i, tdev, dev);
            return 0;
        }
        wantedn++;
    }
    if (!wantedn) { fa_set_error("%s: no frame with a target", who); return 0; }
    /* only the frames with a target, and what they are predicted from */
    StreamRun R;
    R.target = checked.data(); R.t420 = targets420 ? checked420.data() : nullptr; R.first = first; R.caller = (hipStream_t) stream;
    R.ready = ic_mark_ready(stream);
    if (!R.ready) return 0;
    std::vector<uint8_t> mask(count, 0);
    for (unsigned i = 0; i < count; i++) mask[i] = checked[i].data != nullptr;
    const int good = fa_stream_walk(s, who, first, count, mask.data(), magnify, smoothing, targets420 != nullptr, stream_run, &R, 0, nullptr, nullptr);
    (void) hipEventDestroy(R.ready);
    return good;
}

extern "C" int fiasco_amd_stream_decode_device(const fiasco_amd_stream_t *s, unsigned first, unsigned count, int magnify, int smoothing,
                                               const fiasco_amd_device_target *targets, void *hip_stream)
{
    return stream_decode("fiasco_amd_stream_decode_device", s, first, count, magnify, smoothing, targets, nullptr, hip_stream);
}

extern "C" int fiasco_amd_stream_decode_device_420(const fiasco_amd_stream_t *s, unsigned first, unsigned count, int magnify, int smoothing,
                                                   const fiasco_amd_device_target_420 *targets, void *hip_stream)
{
    return stream_decode("fiasco_amd_stream_decode_device_420", s, first, count, magnify, smoothing, nullptr, targets, hip_stream);
}
