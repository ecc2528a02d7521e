/*
 *  decoder_outlet.inc -- the device side of the decoder objects of include/libfiasco_amd_decoder.h (included by
 *  core_hip.cpp behind stream_decode.inc; csrc/host/fa_decoder.c holds the objects and calls these through fa_host.h).
 *
 *  A decoder plays a stream through a cursor (fa_cursor, csrc/host/fa_stream.c).  Every call of the cursor becomes one
 *  decode_frames() with the planes outlet attached (OcOut::planes): the flight copies the shown planes of each wanted
 *  frame into a device buffer the frame's image will own.  No kernel is added: the planes of a frame lie packed, Y / Cb /
 *  Cr back to back, which is the layout an image keeps, so the outlet is one copy on the flight's stream.  The copy is
 *  complete when the call returns (dec_flight_wait).  The buffers are there before the flight starts -- recycled from the
 *  decoder's images that went, or allocated here -- and the share's stream, events and arena are the decoder's own
 *  (DecKeep, frame_decoder.inc), so once a decoder has run, a call adds no allocation and no stream to its flights.  The rest is what an image needs around its buffer: release,
 *  download, the upload of an image that was read from a file, and a staging surface that grows.
 */
/* the calling thread on `device' for the life of the object; device < 0: where it is */
struct DevBind {
    int prev = -1; bool moved = false;
    explicit DevBind(int device)
    {
        if (device < 0 || hipGetDevice(&prev) != hipSuccess) { (void) hipGetLastError(); return; }
        if (prev != device) moved = hipSetDevice(device) == hipSuccess;
    }
    ~DevBind() { if (moved) (void) hipSetDevice(prev); }
};

extern "C" void fa_dev_outlet_run(void *ctx, unsigned n, fa_dec_job *jobs, const unsigned *display, const uint8_t *wanted)
{
    const fa_outlet *O = (const fa_outlet *) ctx;
    std::vector<fiasco_amd_device_frame> target(n, fiasco_amd_device_frame());
    std::vector<unsigned char> done(n, 0);
    std::vector<int16_t *> planes(n, nullptr);
    std::vector<int> dev(n, -1);
    static char mark;
    /* the buffers first, before anything of the flight is queued: one the decoder has back from an image that went
     * (O->take), else a new one on the device the stream decodes on */
    const int sdev = stream_device();
    bool room = true;
    for (unsigned i = 0; i < n; i++) {
        if (!wanted[i]) continue;
        planes[i] = (int16_t *) O->take(O->pool, O->bytes, sdev);
        if (!planes[i]) {
            DevBind on(sdev);
            if (hipMalloc((void **) &planes[i], O->bytes ? O->bytes : 1) != hipSuccess) { (void) hipGetLastError(); planes[i] = nullptr; room = false; }
        }
        dev[i] = sdev;
        target[i].data = &mark;                     /* says "wanted", nothing is written there */
    }
    if (!*O->keep) *O->keep = new (std::nothrow) DecKeep();
    OcOut out;
    out.target = target.data(); out.done = done.data(); out.caller = nullptr; out.ready = nullptr;
    out.planes = planes.data(); out.planes_dev = dev.data(); out.planes_bytes = O->bytes; out.keep = (DecKeep *) *O->keep;
    if (room) (void) decode_frames(n, jobs, &out, nullptr, false);
    for (unsigned i = 0; i < n; i++) {
        if (!room) { jobs[i].out = nullptr; dec_fail(&jobs[i], "device decoder: out of device memory"); }
        if (!wanted[i]) continue;
        if (jobs[i].out && done[i]) { O->planes[display[i]] = planes[i]; O->device[display[i]] = dev[i]; continue; }
        if (planes[i]) fa_dev_free(planes[i], dev[i]);
        if (jobs[i].out) { fa_image_free(jobs[i].out); dec_fail(&jobs[i], "device decoder: the frame was not written"); }
    }
}

extern "C" void fa_dev_keep_free(void *keep)
{
    DecKeep *K = (DecKeep *) keep;
    if (!K) return;
    dec_keep_release(*K);
    delete K;
}

extern "C" int fa_dev_available(void) { return ic_have_device() ? 1 : 0; }

extern "C" void fa_dev_free(void *p, int device)
{
    if (!p) return;
    DevBind on(device);
    if (hipFree(p) != hipSuccess) (void) hipGetLastError();
}

extern "C" void *fa_dev_upload(const void *host, size_t bytes, int *device)
{
    void *p = nullptr;
    if (!ic_have_device()) return nullptr;
    const int dev = stream_device();
    DevBind on(dev);
    if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess || hipMemcpy(p, host, bytes, hipMemcpyHostToDevice) != hipSuccess) {
        fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
        if (p) (void) hipFree(p);
        return nullptr;
    }
    int cur = dev;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = dev; }
    if (device) *device = cur;
    return p;
}

extern "C" int fa_dev_download(void *host, const void *dev, size_t bytes, int device)
{
    DevBind on(device);
    if (hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) == hipSuccess) return 1;
    fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
    return 0;
}

extern "C" int fa_dev_reserve(void **buf, size_t *cap, size_t bytes, int device)
{
    if (*buf && *cap >= bytes) return 1;
    DevBind on(device);
    if (*buf) (void) hipFree(*buf);
    *buf = nullptr; *cap = 0;
    if (hipMalloc(buf, bytes) != hipSuccess) { *buf = nullptr; fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError())); return 0; }
    *cap = bytes;
    return 1;
}
