/*
 *  distortion.inc -- how far a decoded frame is from its original, measured in device memory (included by
 *  core_hip.cpp between output_convert.inc, whose loads, clips and batch preamble it uses, and frame_decoder.inc, whose
 *  flights launch it; core_hip.cpp declares what the three share ahead of them: DEC_FLIGHT, decode_frames()).
 *
 *  The device decoder leaves the planes [bands][height][width] of a frame in HBM as 12.4 fixed point; the original
 *  planes of a device-fed frame lie there already, those of a PNM-fed frame are copied up.  ONE launch of
 *  ds_distortion_kernel per decoder flight compares the two for all frames of the flight and leaves, per frame and
 *  band, the sum of the squared errors and the largest absolute error: 12 bytes per band cross to the host, no plane.
 *
 *  Arithmetic: both sides as the bytes psnr_of() (host/fa_batch_decode.c) and fiasco_amd_batch_decode_plane() form,
 *    a = clip255((orig >> 4) + 128), c = clip255((dec >> 4) + 128)      arithmetic shift, lib/image.c gray_write
 *    d = a - c,  sse += d * d,  maxdiff = max(maxdiff, |d|)
 *  Colour compares Y, Cb and Cr as planes, as psnr_of() does.  Everything is an integer: the sum is exact, the order
 *  of the additions does not matter and two runs give the same bits.  (psnr_of() sums in float like bin/pnmpsnr.c:
 *  below 2^24 its sum is this one, beyond it rounds at every addition.)
 *  Widths: |d| <= 255, d * d <= 65 025; the 16 pixels of a work item add up to at most 1 040 400, held in 32 bits;
 *  everything a thread adds beyond one item, the wave's and the workgroup's sums are 64 bits (one frame of
 *  8192 x 8192 reaches 4.4e12).
 *
 *  Shape: a work item is 16 neighbouring pixels of one row of one plane -- two 16-byte loads per side where the row
 *  allows it (px_load_values: a row of a plane is width * 2 bytes from the last and need not start on 16 bytes), pixels
 *  beyond the end of the row read as zero on both sides and add nothing.  blockIdx.y names the plane (DsPlane: one
 *  band of one frame), the workgroups of one plane stride over its items; a thread's sums go through the wave by
 *  shuffles, through the four waves by LDS, and ONE 64-bit atomicAdd and ONE atomicMax per workgroup reach the
 *  result array, which the launcher zeroes on the same stream before every launch.
 */

struct DsPlane {
    const int16_t *a, *b;            /* original and decoded plane [height][width] */
    unsigned width, height, cpr;     /* cpr: items per row */
    unsigned slot;                   /* frame of the launch * 3 + band: where the results go */
};

enum { DS_SLOTS = DEC_FLIGHT * 3 };  /* a decoder flight: three bands per frame */
/* the result array of a launch: sums first, then the maxima */
#define DS_RES_BYTES ((size_t) DS_SLOTS * (sizeof(unsigned long long) + sizeof(unsigned)))

__global__ void __launch_bounds__(256) ds_distortion_kernel(const DsPlane *__restrict__ planes, unsigned long long *__restrict__ sse,
                                                            unsigned *__restrict__ maxdiff)
{
    __shared__ unsigned long long s_sum[4];
    __shared__ unsigned s_max[4];
    const DsPlane P = planes[blockIdx.y];
    const unsigned items = P.cpr * P.height;                    /* <= 512 * 8192 */
    if (blockIdx.x * 256u >= items) return;                     /* the whole workgroup: a smaller plane of the flight */
    unsigned long long sum = 0;
    unsigned mx = 0;
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < items; it += gridDim.x * 256u) {
        const unsigned row = it / P.cpr, x0 = (it - row * P.cpr) * 16;
        const unsigned n = P.width - x0 < 16 ? P.width - x0 : 16;
        const size_t at = (size_t) row * P.width + x0;
        unsigned va[8], vb[8];
        px_load_values(P.a + at, n, va);
        px_load_values(P.b + at, n, vb);
        unsigned part = 0;                                      /* <= 16 * 255 * 255 */
#pragma unroll
        for (unsigned k = 0; k < 16; k++) {
            const int d = (int) px_clip255(px_int(va, k) + 128) - (int) px_clip255(px_int(vb, k) + 128);
            const unsigned ad = (unsigned) (d < 0 ? -d : d);
            part += ad * ad;
            mx = ad > mx ? ad : mx;
        }
        sum += part;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        const unsigned o = __shfl_down(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_max[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (unsigned w = 1; w < 4; w++) { sum += s_sum[w]; mx = s_max[w] > mx ? s_max[w] : mx; }
        atomicAdd(&sse[P.slot], sum);
        atomicMax(&maxdiff[P.slot], mx);
    }
}

/* ------------------------------------------------------------------ launching */

/* what the decoder is told about the batch call it serves (beside OcOut): frame i of the jobs is compared with its
 * original behind the kernels of its flight and is copied nowhere -- no host image; done[i] = 1 once it is measured */
struct DsOut {
    const int16_t *const *orig;        /* [n] by job index: the original planes on the device the job is decoded on,
                                        * read in place; NULL: image[i]'s host planes, copied into the flight's arena */
    const fa_image *const *image;      /* [n] */
    unsigned long long *sse;           /* [n][3] on the host; either may be NULL */
    unsigned           *maxdiff;
    unsigned char      *done;          /* [n] */
};

/* the planes of one frame behind tab[0 .. n); k: the frame's number in the launch */
static void ds_describe(std::vector<DsPlane> &tab, unsigned k, const int16_t *orig, const int16_t *dec, unsigned width, unsigned height, unsigned bands)
{
    const size_t npix = (size_t) width * height;
    for (unsigned b = 0; b < bands; b++) {
        DsPlane p;
        p.a = orig + b * npix; p.b = dec + b * npix;
        p.width = width; p.height = height; p.cpr = (width + 15) / 16; p.slot = k * 3 + b;
        tab.push_back(p);
    }
}

/* one launch for the planes of the table at d_tab (device memory, a copy of tab) into the zeroed result array at d_res:
 * about eight workgroups of four waves per CU over all planes, fewer when the work is less */
static bool ds_launch(const DsPlane *d_tab, const std::vector<DsPlane> &tab, void *d_res, int ncu, hipStream_t stream)
{
    if (tab.empty()) return true;
    unsigned most = 0;
    for (const DsPlane &p : tab) if (p.cpr * p.height > most) most = p.cpr * p.height;
    unsigned gx = (most + 255) / 256, cap = (unsigned) (ft_groups(ncu) / tab.size());
    if (cap < 1) cap = 1;
    if (gx > cap) gx = cap;
    if (!gx) return true;
    ds_distortion_kernel<<<dim3(gx, (unsigned) tab.size()), dim3(256), 0, stream>>>(d_tab, (unsigned long long *) d_res,
                                                                                    (unsigned *) ((char *) d_res + DS_SLOTS * sizeof(unsigned long long)));
    return hipGetLastError() == hipSuccess;
}

/* ------------------------------------------------------------------ the entry points (include/libfiasco_amd_hip.h) */

/* the two measuring batch entries (this file's and the smoothed one, smooth.inc): the jobs of B (checked, oc_batch_jobs)
 * through the decoder, compared with their originals and, with targets, written */
static int ds_decode_batch(const char *who, const fiasco_amd_batch_t *b, OcBatch &B, unsigned long long *sse, unsigned *maxdiff,
                           const fiasco_amd_device_target *targets, void *stream)
{
    const unsigned n = b->n;
    std::vector<unsigned char> written(n, 0), measured(n, 0);
    std::vector<const int16_t *> orig(n, nullptr);
    std::vector<const fa_image *> image(n, nullptr);
    unsigned wanted = 0;
    for (unsigned i = 0; i < n; i++) {
        if (B.jobs[i].skip) continue;
        /* the original: where the input conversion left it when that is the device the frame is decoded on, else the
         * host planes (a PNM-fed frame has them, a frame on another device is fetched as the PSNR calls fetch it) */
        image[i] = b->jobs[i].image;
        if (image[i]->src_dev && image[i]->src_dev_id == B.device[i]) orig[i] = image[i]->src_dev;
        wanted++;
    }
    if (!wanted) { fa_set_error("%s: no frame with a finished intra automaton", who); return 0; }
    for (unsigned i = 0; i < n; i++)
        if (!B.jobs[i].skip && !orig[i] && !fa_image_host_planes(image[i])) return 0;
    OcOut out;
    out.target = B.target.data(); out.done = written.data(); out.caller = (hipStream_t) stream; out.ready = nullptr;
    if (targets) {
        out.ready = ic_mark_ready(stream);
        if (!out.ready) return 0;
    }
    if (sse) memset(sse, 0, (size_t) n * 3 * sizeof *sse);
    if (maxdiff) memset(maxdiff, 0, (size_t) n * 3 * sizeof *maxdiff);
    DsOut ds;
    ds.orig = orig.data(); ds.image = image.data(); ds.sse = sse; ds.maxdiff = maxdiff; ds.done = measured.data();
    const int good = decode_frames(n, B.jobs.data(), targets ? &out : nullptr, &ds);
    if (out.ready) (void) hipEventDestroy(out.ready);
    for (unsigned i = 0; i < n; i++)
        if (!B.jobs[i].skip && !measured[i]) fa_set_error("<frame %u>: %s", i, B.jobs[i].errmsg[0] ? B.jobs[i].errmsg : "decoder failed");
    return good;
}

extern "C" int fiasco_amd_batch_decode_distortion_device(const fiasco_amd_batch_t *b, unsigned long long *sse, unsigned *maxdiff,
                                                         const fiasco_amd_device_target *targets, void *stream)
{
    OcBatch B;
    const char *who = "fiasco_amd_batch_decode_distortion_device";
    if (!oc_batch_jobs(who, sse || maxdiff || targets ? nullptr : "no result arrays and no targets", b, targets, B)) return 0;
    return ds_decode_batch(who, b, B, sse, maxdiff, targets, stream);
}

extern "C" int fiasco_amd_planes_distortion_device(const int16_t *a, const int16_t *b, int bands, unsigned width, unsigned height,
                                                   unsigned long long sse[3], unsigned maxdiff[3], void *stream)
{
    if (!a || !b) { fa_set_error("fiasco_amd_planes_distortion_device: no planes"); return 0; }
    if (!sse && !maxdiff) { fa_set_error("fiasco_amd_planes_distortion_device: no result arrays"); return 0; }
    if (bands != 1 && bands != 3) { fa_set_error("fiasco_amd_planes_distortion_device: %d bands (1 or 3).", bands); return 0; }
    if (width < 1 || width > 8192 || height < 1 || height > 8192) {
        fa_set_error("fiasco_amd_planes_distortion_device: planes of %u x %u pixels (1 .. 8192 each).", width, height);
        return 0;
    }
    if (!ic_have_device()) return 0;
    const size_t bytes = (size_t) width * height * (unsigned) bands * 2;
    int adev = -1, bdev = -1, cur = -1;
    /* compared in place and only read, yet an allocation that cannot be told is refused here */
    const char *who = "fiasco_amd_planes_distortion_device";
    if (!ic_check_memory(who, "planes `a' are", "planes `a'", a, bytes, "planes `a'", &adev)
        || !ic_check_memory(who, "planes `b' are", "planes `b'", b, bytes, "planes `b'", &bdev)) return 0;
    if (adev != bdev) {
        fa_set_error("fiasco_amd_planes_distortion_device: the planes `a' live on device %d, the planes `b' on device %d (no peer copy on this path).", adev, bdev);
        return 0;
    }
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    if (cur != adev && hipSetDevice(adev) != hipSuccess) { fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError())); return 0; }
    /* on the caller's stream itself: behind what it holds.  Table and results share one small allocation; the table is
     * copied with a blocking call and the buffer freed once the results are back: this call waits on the host. */
    std::vector<DsPlane> tab;
    ds_describe(tab, 0, a, b, width, height, (unsigned) bands);
    const size_t tab_b = align_up(3 * sizeof(DsPlane), 256);
    char *buf = nullptr;
    union { unsigned long long sums[DS_SLOTS]; char bytes[DS_RES_BYTES]; } res;      /* sums, then maxima: 8-byte aligned */
    bool ok = hipMalloc((void **) &buf, tab_b + DS_RES_BYTES) == hipSuccess
              && hipMemcpy(buf, tab.data(), tab.size() * sizeof(DsPlane), hipMemcpyHostToDevice) == hipSuccess
              && hipMemsetAsync(buf + tab_b, 0, DS_RES_BYTES, (hipStream_t) stream) == hipSuccess
              && ds_launch((const DsPlane *) buf, tab, buf + tab_b, ft_cus(), (hipStream_t) stream)
              && hipStreamSynchronize((hipStream_t) stream) == hipSuccess
              && hipMemcpy(res.bytes, buf + tab_b, DS_RES_BYTES, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) fa_set_error("HIP error: %s", hipGetErrorString(hipGetLastError()));
    if (buf) (void) hipFree(buf);
    if (cur >= 0 && cur != adev) (void) hipSetDevice(cur);
    if (!ok) return 0;
    const unsigned *mx = (const unsigned *) (res.bytes + DS_SLOTS * sizeof(unsigned long long));
    for (unsigned k = 0; k < 3; k++) {
        if (sse) sse[k] = k < (unsigned) bands ? res.sums[k] : 0;
        if (maxdiff) maxdiff[k] = k < (unsigned) bands ? mx[k] : 0;
    }
    return 1;
}
