/*
 *  frame_decoder.inc -- the frame an automaton describes, decoded on the device (included by core_hip.cpp).
 *
 *  SURVEY 8(f) row F4: after every frame of a video the coder decodes what it has just written -- the next
 *  P/B frame is predicted from the RECONSTRUCTED frame (reference codec/coder.c:647-651: decode_image +
 *  restore_mc), and the decoded planes are what a PSNR is measured on.  The reference's decoder is integer
 *  arithmetic only (codec/decoder.c:1106-1498, restated for the host in oracle/oracle_decoder.c, whose header
 *  spells out the formulas); here the same values come from one kernel launch per level:
 *
 *    level 0   pixel(s)      = (int) (final_distribution[s] * 8 + .5) * 2                 (host, uploaded)
 *    level l   image(s, l)   = for each half: image(tree child, l - 1) + sum over the edges of
 *                                domain 0 : (int) (weight * final_distribution[0] * 8 + .5) * 2   (a constant)
 *                                domain d : ((int_weight * image(d, l - 1)) >> 10) << 1
 *                              in 16 bits with wrap-around; the float -> int conversions are done on the host
 *                              exactly as oracle_decoder.c does them, the device only sees integers
 *    frame     the images of the states of the largest level that carries a linear combination, copied to
 *              their place and cropped (decode_image, codec/decoder.c:411-536)
 *    P/B       + the motion compensated blocks of the reference frames, chroma clipped to [-128, 127] * 16
 *              (restore_mc, codec/motion.c:37-229; full-pixel vectors)
 *
 *  HBM layout per frame: nodes [S][2] of 32 bytes (tree child, edge list), images of level l at
 *  S * (2^l - 1) + s * 2^l (int16, raster with the level's own width), the planes [bands][H][W].  Every
 *  (state, level < max level) image is computed -- S * 2^max * 2 bytes, 7 MB for a 720p colour frame -- where the
 *  host decoder memoises the ones the frame needs: same values, no dependency tracking (nearly every state is some
 *  state's domain one level up: a reachability closure saves a few per cent); the images of the LARGEST level are
 *  those of the states the frame shows and go straight into the planes (dec_assemble_kernel).  The work is
 *  HBM-bound integer adds: one 2-byte read per (pixel, term), coalesced along the pixels of an image.
 *
 *  Magnification (dfiasco -m M, enlarge_image codec/decoder.c:776-840: 2 M added to the level of every state, the
 *  coordinates shifted by M): the recursion above never asks for the level of a state, so the frame at magnification M
 *  is the images of the SAME top states at level maxl + 2 M, placed at their coordinates << M (>> -M), cropped to the
 *  size of fiasco_amd_magnified_size().  For M = -k the level launches of a full-size decode have written those images on
 *  their way up: dec_thumb_kernel gathers them into reduced planes and one decode gives the frame and its thumbnail.
 *
 *  Smoothing (dfiasco -s N, smooth_image codec/decoder.c:674-768; fa_dec_job.smoothing): behind the kernels that write
 *  the planes of a flight and before every consumer, dec_flight_smooth blends the Y plane of the frames that ask for it
 *  along the borders of their partition, one launch per pass of the border list (smooth.inc).  What is written and what
 *  is measured is then the frame the reference's decoder displays.  Intra frames, at every magnification: the list of a
 *  magnified frame is fa_smoothing_borders_magnified()'s, and a thumbnail beside a frame is smoothed along the list at
 *  minus its reduction, behind dec_thumb_kernel.  Small planes take sm_frame_kernel, all passes in one launch.
 *
 *  4:2:0 (fa_dec_job.format_420; include/libfiasco_amd_420.h; enlarge_image with FORMAT_4_2_0, codec/decoder.c:792-838): the
 *  states behind the Y root get one more step of reduction, so the chroma planes have half the side length and are made of
 *  states two levels higher in the tree, shown at the same level as the Y tops.  fa_420_plan_of (fa_batch_decode.c) gives
 *  that level and the coded levels of the tops; the level launches are the ones above; dec_assemble420_kernel places the
 *  tops in planes Y [H][W], Cb, Cr [H >> 1][W >> 1]; the smoothing list is fa_smoothing_borders_420()'s.  Intra frames, to
 *  4:2:0 targets (output_convert_420.inc) or to the host; the frames of a call are of one format.
 *
 *  Frames of a stream that is walked (fa_dec_job.from_stream; csrc/host/fa_stream.c, stream_decode.inc): their reference
 *  frames live at the magnification and in the format shown, as get_next_frame keeps them, which lifts three refusals for
 *  P/B frames: magnification (the blocks as enlarge_image leaves them: dec_mc_scaled, dec_mc.h), 4:2:0 (dec_mc420_kernel,
 *  dec_clip_chroma420_kernel; a 4:2:0 frame may be kept) and smoothing (a frame that is smoothed and kept is smoothed in a
 *  copy, DecFrame::shown; the kept planes stay unsmoothed).  A residual frame may lack every linear combination, or those of
 *  a band: it gets no tops there and the prediction is added to the zeroed planes.
 *
 *  The decoded planes stay on the device (fa_image.dev): the next P/B frame of the sequence takes its
 *  reference frames with a device-to-device copy (upload_reference); the host copy serves every other caller.
 */
struct DecEdge { int16_t dom, val; };
struct DecNode { int32_t tree, n; DecEdge e[6]; };                    /* 32 bytes per (state, label) */
/* n > 6 (basis states of medium.fco / large.fco, whose edge lists run on into the next rows -- fa_wfa_append_edge):
 * the list lies behind the 2 S nodes, from DecEdge number *(int32_t *) e on */
struct DecTop  { int32_t state, x0, y0, band; };
#define DEC_MC_FN __host__ __device__ static inline
#include "dec_mc.h"                /* DecMc, the blocks of a magnified frame, the items of dec_mc420_kernel */

/* the frames of a flight side by side: blockIdx.y = frame */
struct DecDesc {
    const DecNode *nodes;
    int16_t       *img;
    const DecTop  *tops;
    int16_t       *planes;
    unsigned       S, maxl, ntops, W, H;
};

/* pixel p of the level-l image (l >= 1) of state s from the level l - 1 images */
__device__ __forceinline__ int16_t dec_pixel(const DecNode *__restrict__ nodes, const int16_t *__restrict__ img, unsigned S, unsigned s, unsigned l, unsigned p)
{
    const unsigned wl = l >> 1;                        /* log2 of the width of this level */
    const unsigned cwl = (l - 1) >> 1, chl = l >> 1;   /* log2 of the child's width / height */
    const unsigned y = p >> wl, x = p & ((1u << wl) - 1);
    unsigned label, cx, cy;
    if (l & 1) { label = y >> chl; cy = y & ((1u << chl) - 1); cx = x; }            /* halves above each other */
    else       { label = x >> cwl; cx = x & ((1u << cwl) - 1); cy = y; }            /* side by side */
    const unsigned pc = (cy << cwl) + cx;
    const int16_t *prev = img + (size_t) S * ((1u << (l - 1)) - 1);
    const DecNode nd = nodes[(size_t) s * 2 + label];
    unsigned v = 0;
    if (nd.tree >= 0) v = (uint16_t) prev[((size_t) nd.tree << (l - 1)) + pc];
    if (nd.n <= 6)
        for (int e = 0; e < nd.n; e++) {
            const int dom = nd.e[e].dom, val = nd.e[e].val;
            if (dom == 0) v += (unsigned) val;
            else v += (unsigned) ((((int) val * (int) prev[((size_t) dom << (l - 1)) + pc]) >> 10) * 2);
        }
    else {
        int32_t off;
        memcpy(&off, &nd.e[0], 4);
        const DecEdge *__restrict__ ed = (const DecEdge *) (nodes + (size_t) S * 2) + off;
        for (int e = 0; e < nd.n; e++) {
            const int dom = ed[e].dom, val = ed[e].val;
            if (dom == 0) v += (unsigned) val;
            else v += (unsigned) ((((int) val * (int) prev[((size_t) dom << (l - 1)) + pc]) >> 10) * 2);
        }
    }
    return (int16_t) (uint16_t) v;
}

/* level l < maxl: the image of EVERY state (the level above may read any of them) */
__global__ void __launch_bounds__(256) dec_level_kernel(const DecDesc *__restrict__ descs, unsigned l)
{
    const DecDesc d = descs[blockIdx.y];
    const unsigned S = d.S;
    const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (l >= d.maxl || idx >= ((size_t) S << l)) return;
    const unsigned s = (unsigned) (idx >> l), p = (unsigned) (idx & ((1u << l) - 1));
    d.img[(size_t) S * ((1u << l) - 1) + ((size_t) s << l) + p] = dec_pixel(d.nodes, d.img, S, s, l, p);
}

/* the largest level: only the images the frame is made of (the states of that level), computed straight into their
 * place in the planes, cropped (round 6: half the level images' memory and a third of the decoder's traffic were the
 * top-level images of states nobody shows) */
__global__ void __launch_bounds__(256) dec_assemble_kernel(const DecDesc *__restrict__ descs)
{
    const DecDesc d = descs[blockIdx.y];
    const unsigned l = d.maxl, S = d.S, W = d.W, H = d.H;
    const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (idx >= ((size_t) d.ntops << l)) return;
    const DecTop t = d.tops[idx >> l];
    const unsigned p = (unsigned) (idx & ((1u << l) - 1)), wl = l >> 1;
    const unsigned y = t.y0 + (p >> wl), x = t.x0 + (p & ((1u << wl) - 1));
    if (x >= W || y >= H) return;                                  /* the crop of decode_image */
    d.planes[(size_t) t.band * W * H + (size_t) y * W + x] = l ? dec_pixel(d.nodes, d.img, S, (unsigned) t.state, l, p) : d.img[t.state];
}

/* dec_assemble_kernel for a flight of 4:2:0 frames (include/libfiasco_amd_420.h): the planes are Y [H][W], then Cb and Cr
 * [H >> 1][W >> 1], and every top goes into the plane of its band with that band's base, pitch and crop -- the chroma
 * tops are states two levels higher in the tree, decoded at the same level maxl and placed at coordinates the host has
 * shifted one step further (alloc_state_images, codec/decoder.c:918-937; the crop :502-529) */
__global__ void __launch_bounds__(256) dec_assemble420_kernel(const DecDesc *__restrict__ descs)
{
    const DecDesc d = descs[blockIdx.y];
    const unsigned l = d.maxl, S = d.S;
    const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (idx >= ((size_t) d.ntops << l)) return;
    const DecTop t = d.tops[idx >> l];
    const unsigned W = t.band ? d.W >> 1 : d.W, H = t.band ? d.H >> 1 : d.H;
    const size_t base = t.band ? (size_t) d.W * d.H + (size_t) (t.band - 1) * W * H : 0;
    const unsigned p = (unsigned) (idx & ((1u << l) - 1)), wl = l >> 1;
    const unsigned y = t.y0 + (p >> wl), x = t.x0 + (p & ((1u << wl) - 1));
    if (x >= W || y >= H) return;
    d.planes[base + (size_t) y * W + x] = l ? dec_pixel(d.nodes, d.img, S, (unsigned) t.state, l, p) : d.img[t.state];
}

/* the thumbnails of a flight side by side: blockIdx.y = thumbnail.  img, tops: those of the frame's DecDesc; l: the level
 * shown, the frame's largest less twice the reduction; W, H: the reduced size */
struct DecThumb {
    const int16_t *img;
    const DecTop  *tops;
    int16_t       *planes;
    unsigned       S, l, ntops, W, H, shift;
};

/* the frame at 1 / 2^shift of its side length: the level-l images of the states the frame shows, which the level
 * launches have written (level 0: the pixel table), copied to their place >> shift and cropped.  A copy: one 16-bit
 * load and one 16-bit store per pixel, neighbouring lanes read neighbouring pixels of an image and write neighbouring
 * pixels of a row of its block */
__global__ void __launch_bounds__(256) dec_thumb_kernel(const DecThumb *__restrict__ thumbs)
{
    const DecThumb d = thumbs[blockIdx.y];
    const unsigned l = d.l, W = d.W, H = d.H;
    const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (idx >= ((size_t) d.ntops << l)) return;
    const DecTop t = d.tops[idx >> l];
    const unsigned p = (unsigned) (idx & ((1u << l) - 1)), wl = l >> 1;
    const unsigned y = ((unsigned) t.y0 >> d.shift) + (p >> wl), x = ((unsigned) t.x0 >> d.shift) + (p & ((1u << wl) - 1));
    if (x >= W || y >= H) return;                                  /* the crop of decode_image */
    d.planes[(size_t) t.band * W * H + (size_t) y * W + x] = d.img[(size_t) d.S * ((1u << l) - 1) + ((size_t) t.state << l) + p];
}

/* 16-bit add with wrap-around into a plane other blocks may be adding to (a block that leaves the frame on
 * the right continues in the next row, like the linear addressing of restore_mc) */
__device__ __forceinline__ void dec_add16(int16_t *plane, size_t i, unsigned add)
{
    unsigned *word = (unsigned *) ((uintptr_t) (plane + i) & ~(uintptr_t) 3);
    const unsigned sh = ((uintptr_t) (plane + i) & 2) ? 16 : 0;
    unsigned old = *word, seen;
    do {
        seen = old;
        const unsigned half = ((seen >> sh) + add) & 0xffffu;
        old = atomicCAS(word, seen, (seen & ~(0xffffu << sh)) | (half << sh));
    } while (old != seen);
}

__global__ void __launch_bounds__(256) dec_mc_kernel(const DecMc *__restrict__ mcs, unsigned nmc, unsigned maxl, int16_t *__restrict__ planes,
                                                     const int16_t *__restrict__ past, const int16_t *__restrict__ future,
                                                     unsigned W, unsigned H, unsigned bands)
{
    const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (idx >= ((size_t) nmc * bands << maxl)) return;
    const unsigned p = (unsigned) (idx & ((1u << maxl) - 1));
    const unsigned m = (unsigned) ((idx >> maxl) % nmc), b = (unsigned) ((idx >> maxl) / nmc);
    const DecMc mc = mcs[m];
    if (p >= (1u << mc.level)) return;
    const unsigned wl = (unsigned) mc.level >> 1;
    const long long y = p >> wl, x = p & ((1u << wl) - 1), npix = (long long) W * H;
    const long long di = ((long long) mc.y0 + y) * W + mc.x0 + x;
    const long long fi = ((long long) mc.y0 + mc.fy + y) * W + mc.x0 + mc.fx + x;
    const long long bi = ((long long) mc.y0 + mc.by + y) * W + mc.x0 + mc.bx + x;
    if (di < 0 || di >= npix) return;
    int add;
    if (mc.type == FA_MV_FORWARD) { if (fi < 0 || fi >= npix) return; add = past[(size_t) b * npix + fi]; }
    else if (mc.type == FA_MV_BACKWARD) { if (bi < 0 || bi >= npix) return; add = future[(size_t) b * npix + bi]; }
    else {
        if (fi < 0 || fi >= npix || bi < 0 || bi >= npix) return;
        add = ((int) past[(size_t) b * npix + fi] + (int) future[(size_t) b * npix + bi]) >> 1;
    }
    dec_add16(planes + (size_t) b * npix, (size_t) di, (unsigned) add & 0xffffu);
}

__global__ void __launch_bounds__(256) dec_clip_chroma_kernel(int16_t *__restrict__ planes, size_t npix)
{
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * npix) return;
    int v = planes[npix + i] >> 4;
    v = v < -128 ? -128 : v > 127 ? 127 : v;
    planes[npix + i] = (int16_t) (v * 16);
}

/* dec_mc_kernel for a 4:2:0 frame (fa_dec_job.from_stream; restore_mc with FORMAT_4_2_0, codec/motion.c:51): one work item
 * per pixel of (motion block, band).  Band 0 has dec_mc_kernel's geometry; in bands 1 and 2 the block's place, its sides,
 * the four vector components and the plane width are each halved toward zero (dec_mc420_item, dec_mc.h), the planes lie
 * where dec_assemble420_kernel puts them and the reference frames have the same layout.  Linear addressing, each band
 * checked against its own plane.  Plain 16-bit global accesses */
__global__ void __launch_bounds__(256) dec_mc420_kernel(const DecMc *__restrict__ mcs, unsigned nmc, unsigned maxl, int16_t *__restrict__ planes,
                                                        const int16_t *__restrict__ past, const int16_t *__restrict__ future,
                                                        unsigned W, unsigned H)
{
    const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (idx >= ((size_t) nmc * 3 << maxl)) return;
    const unsigned p = (unsigned) (idx & ((1u << maxl) - 1));
    const unsigned m = (unsigned) ((idx >> maxl) % nmc), b = (unsigned) ((idx >> maxl) / nmc);
    const DecMc mc = mcs[m];
    unsigned long long base;
    long long npix, di, fi, bi;
    if (!dec_mc420_item(&mc, b, p, W, H, &base, &npix, &di, &fi, &bi)) return;
    if (di < 0 || di >= npix) return;
    int add;
    if (mc.type == FA_MV_FORWARD) { if (fi < 0 || fi >= npix) return; add = past[base + fi]; }
    else if (mc.type == FA_MV_BACKWARD) { if (bi < 0 || bi >= npix) return; add = future[base + bi]; }
    else {
        if (fi < 0 || fi >= npix || bi < 0 || bi >= npix) return;
        add = ((int) past[base + fi] + (int) future[base + bi]) >> 1;
    }
    dec_add16(planes + base, (size_t) di, (unsigned) add & 0xffffu);
}

/* dec_clip_chroma_kernel for a 4:2:0 frame: the two planes of cpix = (W >> 1) * (H >> 1) values behind the npix of Y
 * (restore_mc shifts its count by 2, codec/motion.c:195-224) */
__global__ void __launch_bounds__(256) dec_clip_chroma420_kernel(int16_t *__restrict__ planes, size_t npix, size_t cpix)
{
    const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * cpix) return;
    int v = planes[npix + i] >> 4;
    v = v < -128 ? -128 : v > 127 ? 127 : v;
    planes[npix + i] = (int16_t) (v * 16);
}

static int16_t dec_fixed_of(float v) { return (int16_t) ((int) ((double) (v * 8) + .5) * 2); }

/* one plane that is smoothed: the checked border list against it (packed into the flight's block, never uploaded itself),
 * what sm_check() counted, where its sm_table_bytes() lie in the arena, and which kernel takes it.  np == 0: no launch */
struct SmPlan {
    std::vector<fiasco_amd_border> borders;
    unsigned np = 0;                  /* its passes */
    unsigned long long pairs = 0;     /* pixel pairs blended: 4 bytes read and 4 written each */
    size_t off = 0, b = 0;
    bool fused = false;               /* sm_frame_kernel, not the per-pass launches (sm_takes_fused) */
};

struct DecFrame {                     /* one frame in flight */
    char *base = nullptr;             /* nodes | tops | mcs | images */
    int16_t *planes = nullptr;        /* the result: stays on the device */
    size_t plane_bytes = 0;
    int16_t *past = nullptr, *future = nullptr;     /* uploaded copies (nullptr: the reference's own device planes) */
    std::vector<char> host;           /* sources of the asynchronous uploads: alive until the stream is drained */
    std::vector<int16_t> px0;
    /* dec_prepare -> dec_run */
    size_t nodes_b = 0, tops_b = 0, mcs_b = 0, img_b = 0, scratch_b = 0;
    unsigned S = 0, maxl = 0, mc_maxl = 0, ntops = 0, nmcs = 0;           /* maxl: the level shown (magnification included) */
    unsigned W = 0, H = 0;            /* the size shown: the coded one, or fiasco_amd_magnified_size() */
    bool c420 = false;                /* 4:2:0 (fa_dec_job.format_420): the planes are Y [H][W], Cb and Cr [H >> 1][W >> 1] */
    size_t vals = 0;                  /* the values of all its planes */
    int16_t *thumb = nullptr;         /* a thumbnail beside the frame (dec_flight_thumbs): its reduced planes in the arena */
    size_t thumb_off = 0, thumb_bytes = 0;
    unsigned tw = 0, th = 0;
    bool own_planes = false;          /* planes is an allocation of its own (kept on the device) */
    int16_t *shown = nullptr;         /* a frame that is smoothed AND kept (fa_dec_job.from_stream): the copy in the arena that is smoothed
                                       * and consumed, while `planes' stays as the next frame is predicted from it (get_next_frame
                                       * smooths a clone, codec/decoder.c:372-378); nullptr: the planes themselves */
    size_t shown_off = 0;             /* ... from the frame's scratch */
    bool shown_copy = false;
    unsigned long long bytes = 0;     /* algorithmic: 2 bytes per pixel written and per (pixel, term) read */
    size_t scratch_off = 0;           /* dec_flight_prepare: its scratch_b bytes of the flight's arena */
    unsigned slot = 0;                /* dec_flight_measure: its place in the result array of the measuring launch */
    bool measured = false;            /* ... which it has only if it has an original (DsOut) */
    /* smoothing (dec_smooth_prepare -> dec_flight_smooth, smooth.inc) */
    SmPlan sm, tsm;                   /* the frame's Y plane at the size shown; the Y plane of its thumbnail */
    int sm_is = 0, sm_inegs = 0;      /* the factors */
};

/* the planes the smoothing step and the consumers take */
static int16_t *dec_shown(const DecFrame &D) { return D.shown ? D.shown : D.planes; }

static void dec_fail(fa_dec_job *j, const char *msg) { snprintf(j->errmsg, sizeof j->errmsg, "%s", msg); j->out = nullptr; }

/* the edges of row r = (state, label) of the automaton; more than six run on into the next rows (fa_wfa_append_edge) */
static unsigned dec_edges(const fa_wfa *w, size_t r)
{
    unsigned e = 0;
    while (r * 6 + e < (size_t) w->cap * 12 && w->into[r * 6 + e] != FA_NO_EDGE) e++;
    return e;
}

/* what a node reads per pixel: its tree child and the edges into other domains than the constant one */
static unsigned dec_terms(const DecNode &n, const DecEdge *ext)
{
    int32_t off = 0;
    if (n.n > 6) memcpy(&off, &n.e[0], 4);
    const DecEdge *ed = n.n > 6 ? ext + off : n.e;
    unsigned terms = n.tree >= 0;
    for (int e = 0; e < n.n; e++) terms += ed[e].dom != 0;
    return terms;
}

/* host side of one frame: the integer automaton, the block lists, the sizes */
static bool dec_prepare(fa_dec_job *j, DecFrame &D)
{
    const fa_wfa *w = j->wfa;
    const unsigned S = w->states, bands = j->color ? 3 : 1;
    unsigned root[3] = { 0, 0, 0 }, maxl = 0, W = j->width, H = j->height;
    const int mag = j->magnify;
    const bool walked = j->from_stream != 0;        /* a frame of a stream that is walked: its references live at the size and in the format shown */
    if (mag && j->frame_type != FA_I_FRAME && !walked) { dec_fail(j, "device decoder: magnification of intra frames only (the vectors of a P/B frame are not scaled)"); return false; }
    if (j->format_420 && (j->frame_type != FA_I_FRAME || j->keep_dev) && !walked) { dec_fail(j, "device decoder: 4:2:0 for intra frames only (restore_mc scales the vectors per band)"); return false; }
    if (mag && !fiasco_amd_magnified_size(j->width, j->height, mag, &W, &H)) {
        snprintf(j->errmsg, sizeof j->errmsg, "device decoder: magnification %d is out of range for a frame of %u x %u pixels", mag, j->width, j->height);
        j->out = nullptr; return false;
    }
    if (j->color) {
        const unsigned r0 = (unsigned) FA_TREE(w, w->root_state, 0), r1 = (unsigned) FA_TREE(w, w->root_state, 1);
        root[FA_Y] = (unsigned) FA_TREE(w, r0, 0); root[FA_CB] = (unsigned) FA_TREE(w, r0, 1); root[FA_CR] = (unsigned) FA_TREE(w, r1, 0);
    } else root[0] = w->root_state;
    bool any_edge = false;
    for (unsigned s = w->basis_states; s < S; s++)
        if (FA_INTO(w, s, 0, 0) != FA_NO_EDGE || FA_INTO(w, s, 1, 0) != FA_NO_EDGE) {
            any_edge = true;
            if (w->level_of_state[s] > maxl) maxl = w->level_of_state[s];
        }
    /* A P/B frame of a walked stream is a residual: it may hold no linear combination at all, or none in a band.
     * decode_image leaves zeros there (no state at the level shown), and zeros are what the prediction is added to: such a
     * frame gets no tops for the band, where an intra frame of the batch entries is refused as degenerate */
    const bool residual = walked && j->frame_type != FA_I_FRAME;
    const unsigned NO_TOPS = 255;                   /* no state has that level */
    unsigned top_level[2] = { maxl, maxl };          /* the coded level of the states shown: Y (gray), chroma */
    if (residual && !any_edge) top_level[0] = top_level[1] = NO_TOPS;
    if (maxl > 24) { dec_fail(j, "device decoder: level of the linear combinations out of range"); return false; }
    /* the level shown (the header): the states of level `maxl' at level maxl + 2 mag.  Blocks smaller than the reduction
     * -- the reference clamps their level at 0 and several land on one pixel -- are refused, not reproduced */
    if (mag < 0 && maxl < 2u * (unsigned) -mag && !(residual && !any_edge)) { dec_fail(j, "device decoder: the blocks of the frame are smaller than the reduction (level of the linear combinations below twice the reduction)"); return false; }
    unsigned shown = residual && !any_edge ? 0u : (unsigned) ((int) maxl + 2 * mag);
    /* 4:2:0: the level shown and the coded levels of the states the planes are made of come from fa_420_plan_of, which
     * also refuses what is not reproduced (fa_batch_decode.c) */
    fa_420_plan plan = { 0, 0, 0 };
    if (j->format_420 && residual) {
        /* fa_420_plan_of without its refusals of what comes out zero: per band group the largest level with a linear
         * combination, shown at + 2 mag (Y) and + 2 mag - 2 (chroma); the largest of those is the level of every top */
        if (!j->color) { dec_fail(j, "device decoder: 4:2:0: a gray frame has no chroma bands"); return false; }
        int lc[2] = { -1, -1 }, top = -1;
        const int shift[2] = { 2 * mag, 2 * mag - 2 };
        for (unsigned s = w->basis_states; s < S; s++) {
            if (s == w->root_state || s == (unsigned) FA_TREE(w, w->root_state, 0) || s == (unsigned) FA_TREE(w, w->root_state, 1)) continue;
            if (FA_INTO(w, s, 0, 0) == FA_NO_EDGE && FA_INTO(w, s, 1, 0) == FA_NO_EDGE) continue;
            const int g = s > root[FA_Y];
            if ((int) w->level_of_state[s] > lc[g]) lc[g] = w->level_of_state[s];
        }
        for (int g = 0; g < 2; g++) {
            if (lc[g] < 0) continue;
            if (lc[g] + shift[g] < 0) { dec_fail(j, "device decoder: 4:2:0: the blocks of the frame are smaller than the reduction"); return false; }
            if (lc[g] + shift[g] > top) top = lc[g] + shift[g];
        }
        shown = top < 0 ? 0u : (unsigned) top;
        for (int g = 0; g < 2; g++) top_level[g] = top < 0 || top - shift[g] < 0 ? NO_TOPS : (unsigned) (top - shift[g]);
    } else if (j->format_420) {
        char why[160];
        if (!fa_420_plan_of(w, j->color, mag, &plan, why, sizeof why)) {
            snprintf(j->errmsg, sizeof j->errmsg, "device decoder: %.140s", why);
            j->out = nullptr; return false;
        }
        shown = plan.max_level;
        top_level[0] = plan.y_level; top_level[1] = plan.c_level;
    }
    if (shown > 24) { dec_fail(j, "device decoder: level of the magnified linear combinations out of range (above 24)"); return false; }
    /* host side of the arithmetic: nodes with integer weights, the lists of blocks */
    std::vector<DecTop> tops;
    std::vector<DecMc> mcs;
    for (unsigned s = w->basis_states; s < S; s++) {
        if (j->color && (s == w->root_state || s == (unsigned) FA_TREE(w, w->root_state, 0) || s == (unsigned) FA_TREE(w, w->root_state, 1)))
            continue;
        const int band = !j->color || s <= root[FA_Y] ? 0 : s > root[FA_CB] ? FA_CR : FA_CB;
        if (w->level_of_state[s] == top_level[j->format_420 && band ? 1 : 0]) {
            const int shift = j->format_420 && band ? mag - 1 : mag;       /* enlarge_image: one step more behind the Y root */
            DecTop t;
            t.state = (int) s; t.x0 = w->x[s * 2]; t.y0 = w->y[s * 2];
            if (shift > 0) { t.x0 <<= shift; t.y0 <<= shift; } else if (shift < 0) { t.x0 >>= -shift; t.y0 >>= -shift; }
            t.band = band;
            tops.push_back(t);
        }
    }
    unsigned mc_maxl = 0;
    if (j->frame_type != FA_I_FRAME) {
        const unsigned yroot = j->color ? root[FA_Y] : w->root_state;
        for (unsigned s = w->basis_states; s <= yroot; s++)
            for (unsigned l = 0; l < 2; l++) {
                const fa_mv *mv = &w->mv[s * 2 + l];
                const unsigned level = (unsigned) w->level_of_state[s] - 1;
                if (mv->type == FA_MV_NONE || level > j->p_max_level) continue;
                if ((mv->type != FA_MV_BACKWARD && !j->past) || (mv->type != FA_MV_FORWARD && !j->future)) {
                    dec_fail(j, "device decoder: motion vector without its reference frame"); return false;
                }
                DecMc m;
                if (!dec_mc_scaled(&m, w->x[s * 2 + l], w->y[s * 2 + l], (int) level, mv->type, mv->fx, mv->fy, mv->bx, mv->by, mag)) {
                    dec_fail(j, "device decoder: the motion blocks of the frame are smaller than the reduction (level of a block below twice the reduction)");
                    return false;
                }
                mcs.push_back(m);
                if ((unsigned) m.level > mc_maxl) mc_maxl = (unsigned) m.level;
            }
    }
    /* edge lists of more than six entries (long bases): behind the nodes */
    size_t next = 0;
    for (size_t r = 0; r < (size_t) S * 2; r++) { const unsigned e = dec_edges(w, r); if (e > 6) next += e; }
    const size_t nodes_b = align_up((size_t) S * 2 * sizeof(DecNode) + next * sizeof(DecEdge), 256), tops_b = align_up((tops.size() + 1) * sizeof(DecTop), 256),
                 mcs_b = align_up((mcs.size() + 1) * sizeof(DecMc), 256), img_b = align_up(((size_t) S << shown) * 2 + 256, 256);      /* levels 0 .. shown - 1 of every state */
    D.host.assign(nodes_b + tops_b + mcs_b, 0);
    DecNode *nodes = (DecNode *) D.host.data();
    DecEdge *ext = (DecEdge *) (nodes + (size_t) S * 2);
    int32_t ext_used = 0;
    for (unsigned s = 0; s < S; s++)
        for (unsigned l = 0; l < 2; l++) {
            DecNode &n = nodes[(size_t) s * 2 + l];
            n.tree = FA_TREE(w, s, l) != FA_RANGE ? (int) FA_TREE(w, s, l) : -1;
            const unsigned cnt = dec_edges(w, (size_t) s * 2 + l);
            DecEdge *dst = n.e;
            if (cnt > 6) { memcpy(&n.e[0], &ext_used, 4); dst = ext + ext_used; ext_used += (int32_t) cnt; }
            n.n = (int32_t) cnt;
            for (unsigned e = 0; e < cnt; e++) {
                const int dom = FA_INTO(w, s, l, e);
                dst[e].dom = (int16_t) dom;
                dst[e].val = dom == 0 ? (int16_t) ((int) ((double) (FA_WEIGHT(w, s, l, e) * w->final_distribution[0] * 8) + .5) * 2)
                                      : (int16_t) ((double) (FA_WEIGHT(w, s, l, e) * 512) + 0.5);
            }
        }
    if (!tops.empty()) memcpy(D.host.data() + nodes_b, tops.data(), tops.size() * sizeof(DecTop));
    if (!mcs.empty()) memcpy(D.host.data() + nodes_b + tops_b, mcs.data(), mcs.size() * sizeof(DecMc));
    D.px0.resize(S);
    for (unsigned s = 0; s < S; s++) D.px0[s] = dec_fixed_of(w->final_distribution[s]);

    const size_t npix = (size_t) W * H;
    D.c420 = j->format_420 != 0;
    D.vals = D.c420 ? npix + 2 * ((size_t) (W >> 1) * (H >> 1)) : npix * bands;
    D.plane_bytes = align_up(D.vals * 2, 256);
    D.nodes_b = nodes_b; D.tops_b = tops_b; D.mcs_b = mcs_b; D.img_b = img_b;
    D.S = S; D.maxl = shown; D.W = W; D.H = H; D.mc_maxl = mc_maxl; D.ntops = (unsigned) tops.size(); D.nmcs = (unsigned) mcs.size();
    D.own_planes = j->keep_dev != 0;
    D.scratch_b = nodes_b + tops_b + mcs_b + img_b + (D.own_planes ? 0 : D.plane_bytes);
    /* level l < maxl: S * 2^l pixels written, terms * 2^(l-1) read; the top level: the terms of the states shown,
     * straight into the frame: written once, read by nobody here */
    unsigned long long terms = 0, top_terms = 0;
    for (size_t k = 0; k < (size_t) S * 2; k++) terms += dec_terms(nodes[k], ext);
    for (size_t k = 0; k < tops.size(); k++)
        for (unsigned l = 0; l < 2; l++) top_terms += dec_terms(nodes[(size_t) tops[k].state * 2 + l], ext);
    const unsigned long long lower = shown ? (((unsigned long long) S << shown) - 2ull * S) : 0ull;
    const unsigned long long lower_reads = shown ? terms * ((1ull << (shown - 1)) - 1) : 0ull;
    D.bytes = 2ull * (lower + lower_reads + (shown ? top_terms << (shown - 1) : 0ull)) + 2ull * D.vals;
    return true;
}

/* device side of one frame, queued on `stream': its automaton, the level-0 images and the zeroed planes;
 * scratch: D.scratch_b bytes of the flight's arena */
static bool dec_run(fa_dec_job *j, DecFrame &D, char *scratch, hipStream_t stream)
{
    const size_t up_b = D.nodes_b + D.tops_b + D.mcs_b;
    D.base = scratch;
    if (D.own_planes) {
        if (hipMalloc((void **) &D.planes, D.plane_bytes) != hipSuccess) { (void) hipGetLastError(); D.planes = nullptr; dec_fail(j, "device decoder: out of device memory"); return false; }
    } else D.planes = (int16_t *) (scratch + up_b + D.img_b);
    bool ok = hipMemcpyAsync(D.base, D.host.data(), up_b, hipMemcpyHostToDevice, stream) == hipSuccess
              && hipMemcpyAsync(D.base + up_b, D.px0.data(), (size_t) D.S * 2, hipMemcpyHostToDevice, stream) == hipSuccess
              && hipMemsetAsync(D.planes, 0, D.plane_bytes, stream) == hipSuccess;
    if (!ok) { (void) hipGetLastError(); dec_fail(j, "device decoder: HIP error"); }
    return ok;
}

/* after the level and assembly launches of the flight: motion compensation of a P/B frame.  restore_mc is called for
 * every P/B frame: the clipping of the chroma planes too when no block moved */
static bool dec_run_mc(fa_dec_job *j, DecFrame &D, hipStream_t stream, int cur_dev)
{
    /* the size shown: the coded one but for a frame of a stream that is walked at a magnification */
    const unsigned bands = j->color ? 3 : 1, W = D.W, H = D.H;
    const size_t npix = (size_t) W * H;
    const int16_t *refs[2] = { nullptr, nullptr };
    const fa_image *src[2] = { j->past, j->future };
    bool ok = true;
    for (int r = 0; r < 2 && ok; r++) {
        if (!src[r]) continue;
        if (src[r]->width != W || src[r]->height != H || (src[r]->color != 0) != (j->color != 0)) {
            dec_fail(j, "device decoder: reference frame of another size"); ok = false; break;
        }
        if (src[r]->dev && src[r]->dev_id == cur_dev) { refs[r] = (const int16_t *) src[r]->dev; continue; }
        /* the frames of a walked stream stay on one share; their host planes, where they have any, may be 4:2:0 */
        if (D.c420 || !src[r]->pixels[0]) { dec_fail(j, "device decoder: the reference frame does not lie on the device the frame is decoded on"); ok = false; break; }
        int16_t *&up = r ? D.future : D.past;
        if (hipMalloc((void **) &up, D.plane_bytes) != hipSuccess) { (void) hipGetLastError(); dec_fail(j, "device decoder: out of device memory"); ok = false; break; }
        for (unsigned b = 0; b < bands && ok; b++)
            ok = hipMemcpyAsync(up + b * npix, src[r]->pixels[b], npix * 2, hipMemcpyHostToDevice, stream) == hipSuccess;
        refs[r] = up;
    }
    const size_t cpix = (size_t) (W >> 1) * (H >> 1);
    if (ok && D.nmcs) {
        const size_t n = ((size_t) D.nmcs * bands) << D.mc_maxl;
        const DecMc *mcs = (const DecMc *) (D.base + D.nodes_b + D.tops_b);
        if (D.c420) dec_mc420_kernel<<<dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream>>>(mcs, D.nmcs, D.mc_maxl, D.planes, refs[0], refs[1], W, H);
        else dec_mc_kernel<<<dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, stream>>>(mcs, D.nmcs, D.mc_maxl, D.planes, refs[0], refs[1], W, H, bands);
    }
    if (ok && j->color && D.c420) {
        if (cpix) dec_clip_chroma420_kernel<<<dim3((unsigned) ((2 * cpix + 255) / 256)), dim3(256), 0, stream>>>(D.planes, npix, cpix);
    } else if (ok && j->color)
        dec_clip_chroma_kernel<<<dim3((unsigned) ((2 * npix + 255) / 256)), dim3(256), 0, stream>>>(D.planes, npix);
    if (ok && hipGetLastError() != hipSuccess) ok = false;
    if (!ok && !j->errmsg[0]) dec_fail(j, "device decoder: HIP error");
    return ok;
}

extern "C" void fa_core_release_dev(void *dev, int dev_id)
{
    (void) dev_id;
    if (dev) (void) hipFree(dev);
}

/* ------------------------------------------------------------------ a share of a call, flight by flight */

/* One share of fa_core_decode_frames, on the device the calling thread is bound to (for_shares / bind_share,
 * shares.inc): what its flights have in common.  The two optional consumers of a flight's planes:
 * out != NULL (fiasco_amd_batch_decode_device, output_convert.inc): the frames are written as 8-bit pixels into
 * out->target[job]; such a frame gets no host image and no copy to the host (jobs[].out stays NULL, out->done[job] says
 * that it was written).  out->thumb != NULL (fiasco_amd_batch_decode_device_thumbnails): frame `job' is written a second
 * time, at 1 / 2^out->reduce of its side length, into out->thumb[job]; out->thumb_done[job] says so.  out->planes != NULL
 * (the images of a fiasco_decoder_t, decoder_outlet.inc): the shown planes themselves are copied into out->planes[job], a
 * buffer that was made before the call (the flight allocates nothing), instead of being converted; out->done[job] says
 * that they were.
 * ds != NULL (fiasco_amd_batch_decode_distortion_device, distortion.inc): the frames are compared with their originals
 * before the pixels are written, if they are (a frame whose target has no data is measured only).  Such a frame gets
 * no host image either; ds->done[job] says that it was measured. */
struct DecShare {
    fa_dec_job  *jobs;
    const OcOut *out; const DsOut *ds;          /* the optional consumers */
    bool         images = false;                /* ... beside the host images, not instead of them (the frames of a video: the
                                                 * sequence engine goes on with the image, fa_dec_job's consumer fields) */
    int          device = 0, ncu = 256;         /* the current one and its CUs, asked once per share */
    hipStream_t  stream = nullptr;
    hipEvent_t   ev0 = nullptr, ev1 = nullptr;  /* around the device work of a flight: decoder_us */
    char        *arena = nullptr; size_t arena_b = 0;       /* one per share, grown when a flight needs more */
    size_t       flight = DEC_FLIGHT;           /* halved when the level images of a flight do not fit (large blocks at a low quality) */
    int          good = 0;                      /* frames decoded */
};

/* The frames of one flight.  The level images of a frame (14 MB at 720p colour) live for one flight only, beside the
 * slabs of a staged batch.  The flight owns what its asynchronous uploads read -- the frames' host buffers, the tables
 * and the packed smoothing tables -- until dec_flight_wait has drained the stream, and the carve of the arena. */
struct DecFlight {
    std::vector<unsigned> job;                  /* [frame] index into the jobs */
    std::vector<DecFrame> fr;                   /* [frame] */
    std::vector<size_t>   alive;                /* the frames nothing has failed yet, in order */
    std::vector<DecDesc>  descs;                /* one per frame alive after the uploads: blockIdx.y of the level launches */
    std::vector<OcFrame>  octab; std::vector<DsPlane> dstab;    /* the frames written; the planes measured */
    std::vector<Y4Frame>  y4tab;                /* ... written as 4:2:0 buffers (OcOut::t420), in place of octab */
    std::vector<Rd4Frame> rd4tab;               /* ... or as display surfaces (OcOut::t420 and OcOut::render), in place of y4tab */
    std::vector<DecThumb> thtab; std::vector<OcFrame> thoctab;  /* the thumbnails gathered; written */
    std::vector<SmDesc>   smtab, tsmtab;        /* one per frame (thumbnail) alive and smoothed: first those of the per-pass
                                                 * launches (their blockIdx.y), then those of the fused launch (its blockIdx.x) */
    std::vector<char>     smhost;               /* the packed smoothing tables of the flight, laid out as in the arena from
                                                 * sm_first on: sized and filled by dec_flight_prepare, not touched after */
    union { unsigned long long sums[DS_SLOTS]; char bytes[DS_RES_BYTES]; } dsres;      /* sums, then maxima: 8-byte aligned */
    /* the arena: the scratch of every frame (DecFrame::scratch_off), then */
    size_t desc_off = 0, oc_off = 0;            /* the tables of DecDesc and OcFrame */
    size_t th_off = 0, thoc_off = 0;            /* thumbnails: the tables of DecThumb and OcFrame, */
    size_t thumb_first = 0, thumb_all = 0;      /* ... and the reduced planes of all frames, back to back: zeroed with one call */
    size_t smd_off = 0, tsmd_off = 0, sm_first = 0;     /* smoothing: the tables of SmDesc of the frames and of the thumbnails; the packed tables (SmPlan::off) */
    size_t ds_off = 0, res_off = 0, orig_off = 0;       /* measuring: the table of DsPlane, the result array, the originals that come from the host */
    size_t need = 0;                            /* all of it */

    size_t take(size_t bytes) { const size_t at = need; need += align_up(bytes, 256); return at; }
};

static_assert(DS_SLOTS == DEC_FLIGHT * 3, "the result array of a measuring launch has three slots per frame of a flight");

/* every frame of the flight that is still alive fails with msg */
static void dec_flight_fail(DecShare &S, DecFlight &F, const char *msg)
{
    (void) hipGetLastError();
    for (size_t k : F.alive) dec_fail(&S.jobs[F.job[k]], msg);
    F.alive.clear();
}

static void dec_account(unsigned long long us, unsigned frames, unsigned long long bytes)
{
    stats_update([&](fiasco_amd_stats &st) { st.decoder_us += us; st.decoder_frames += frames; st.decoder_bytes += bytes; });
}

/* a frame that gets a thumbnail beside it: the level shown is the frame's less twice the reduction, which the level
 * launches write only if it exists; the reduced planes are sized by the target (checked by the entry point) */
static bool dec_thumb_prepare(DecShare &S, unsigned job, DecFrame &D)
{
    const fiasco_amd_device_frame &t = S.out->thumb[job];
    if (!t.data) return true;
    if (D.maxl < 2 * S.out->reduce) {
        dec_fail(&S.jobs[job], "device decoder: the blocks of the frame are smaller than the reduction (level of the linear combinations below twice the reduction)");
        return false;
    }
    D.tw = t.width; D.th = t.height;
    D.thumb_bytes = align_up((size_t) D.tw * D.th * (S.jobs[job].color ? 3 : 1) * 2, 256);
    return true;
}

/* the borders of the job's partition at `magnify' (fa_smoothing_borders_magnified: the list `dfiasco -m magnify' smooths
 * along), checked against the plane of W x H they will be blended in.  A frame with a state that falls below level 1 at
 * that magnification, and a list that fails the check, fail with the message; an empty list is a plan without passes */
static bool dec_smooth_plan(fa_dec_job *j, int magnify, unsigned W, unsigned H, SmPlan &P, bool c420 = false)
{
    /* a 4:2:0 frame: the list of the automaton enlarge_image has shifted for that format (fa_smoothing_borders_420) */
    auto list = [&](fiasco_amd_border *out, unsigned cap) {
        if (c420 && j->from_stream && j->frame_type != FA_I_FRAME) return fa_smoothing_borders_420_residual(j->wfa, j->width, j->height, j->color, magnify, out, cap);
        return c420 ? fa_smoothing_borders_420(j->wfa, j->width, j->height, j->color, magnify, out, cap)
                    : fa_smoothing_borders_magnified(j->wfa, j->width, j->height, j->color, magnify, out, cap);
    };
    fa_set_error("%s", "");
    const unsigned n = list(nullptr, 0);
    if (!n) {
        const char *why = fiasco_get_error_message();
        if (!why[0]) return true;
        dec_fail(j, why);
        return false;
    }
    P.borders.resize(n);
    char msg[200];
    if (list(P.borders.data(), n) != n) { dec_fail(j, "device decoder: the smoothing borders changed while they were listed"); return false; }
    if (!sm_check(P.borders.data(), n, W, H, &P.np, &P.pairs, msg, sizeof msg)) { P.np = 0; dec_fail(j, msg); return false; }
    P.b = sm_table_bytes(n, P.np);
    P.fused = sm_takes_fused(P.pairs, P.np);
    return true;
}

/* a frame that is smoothed (fa_dec_job.smoothing): its factors, and the borders of its partition at the magnification it
 * is shown at -- and, where it gets a thumbnail, a second list at minus the reduction for the reduced plane --, checked
 * against their planes before anything of the flight is uploaded or launched.  A list that fails fails its frame alone,
 * thumbnail and all.  SmPlan::b is what dec_flight_prepare carves and packs.  A full-size plane nobody consumes (a
 * thumbnail only, of a batch entry) is not smoothed */
static bool dec_smooth_prepare(DecShare &S, unsigned job, DecFrame &D)
{
    fa_dec_job *j = &S.jobs[job];
    if (!j->smoothing) return true;
    if (j->smoothing < 0 || j->smoothing > 100) { dec_fail(j, "device decoder: smoothing out of range (1 .. 100 per cent; the header's value is the batch entries' to look up)"); return false; }
    /* a P/B frame of a walked stream is smoothed along the borders of its own automaton, as get_next_frame does it */
    if (j->frame_type != FA_I_FRAME && !j->from_stream) { dec_fail(j, "device decoder: smoothing of intra frames only"); return false; }
    if (!sm_factors(j->smoothing, &D.sm_is, &D.sm_inegs)) return true;       /* the reference smooths nothing */
    const bool consumed = !S.out || S.ds || S.images || S.out->target[job].data;
    if (consumed && !dec_smooth_plan(j, j->magnify, D.W, D.H, D.sm, D.c420)) return false;
    /* smoothed and kept: the copy that is smoothed and consumed, behind the frame's scratch */
    if (D.sm.np && D.own_planes && j->from_stream) { D.shown_copy = true; D.shown_off = D.scratch_b; D.scratch_b += D.plane_bytes; }
    if (D.thumb_bytes && !dec_smooth_plan(j, -(int) S.out->reduce, D.tw, D.th, D.tsm)) return false;
    return true;
}

/* host side of the n frames `idx': their automata as integers, and where everything lies in the arena.  The tables
 * are sized for a full flight whatever n is */
static void dec_flight_prepare(DecShare &S, DecFlight &F, const unsigned *idx, size_t n)
{
    F.job.assign(idx, idx + n);
    F.fr.resize(n);
    const bool thumbs = S.out && S.out->thumb;
    bool smooth = false, tsmooth = false;
    for (size_t k = 0; k < n; k++)
        if (dec_prepare(&S.jobs[F.job[k]], F.fr[k]) && (!thumbs || dec_thumb_prepare(S, F.job[k], F.fr[k])) && dec_smooth_prepare(S, F.job[k], F.fr[k])) {
            /* 4:2:0 planes have consumers of their own -- the 4:2:0 targets of the call, or the host -- and a flight has one
             * assembly launch: the frames of a call are of one format */
            const bool c420 = F.fr[k].c420;
            if ((c420 && (S.ds || S.images || thumbs || (S.out && !S.out->t420 && !S.out->planes))) || (!c420 && S.out && S.out->t420)
                || (!F.alive.empty() && F.fr[F.alive[0]].c420 != c420)) {
                dec_fail(&S.jobs[F.job[k]], "device decoder: 4:2:0 frames and 4:4:4 frames do not share a call, and 4:2:0 frames go to 4:2:0 targets or to the host");
                continue;
            }
            F.alive.push_back(k); F.fr[k].scratch_off = F.take(F.fr[k].scratch_b);
            smooth = smooth || F.fr[k].sm.np;
            tsmooth = tsmooth || F.fr[k].tsm.np;
        }
    F.desc_off = F.take(DEC_FLIGHT * sizeof(DecDesc));
    /* smoothing: the table of SmDesc of the frames and a second one of the thumbnails, then the packed tables of every
     * plane that has passes, back to back: filled on the host here, in a block of the size of the carve, and uploaded
     * with one copy (dec_flight_smooth) */
    F.smd_off = F.take(smooth ? DEC_FLIGHT * sizeof(SmDesc) : 0);
    F.tsmd_off = F.take(tsmooth ? DEC_FLIGHT * sizeof(SmDesc) : 0);
    F.sm_first = F.need;
    for (size_t k : F.alive)
        for (SmPlan *P : { &F.fr[k].sm, &F.fr[k].tsm }) if (P->np) P->off = F.take(P->b);
    F.smhost.assign(F.need - F.sm_first, 0);
    std::vector<size_t> run;
    for (size_t k : F.alive) {
        bool fits = true;
        for (SmPlan *P : { &F.fr[k].sm, &F.fr[k].tsm })
            fits = fits && (!P->np || sm_pack(P->borders.data(), (unsigned) P->borders.size(), P->np, F.smhost.data() + (P->off - F.sm_first), P->b));
        if (!fits) {
            dec_fail(&S.jobs[F.job[k]], "device decoder: the smoothing tables do not fit their carve");
            continue;
        }
        run.push_back(k);
    }
    F.alive.swap(run);
    F.oc_off = F.take(S.out ? DEC_FLIGHT * (S.out->t420 ? sizeof(Y4Frame) : sizeof(OcFrame)) : 0);
    F.th_off = F.take(thumbs ? DEC_FLIGHT * sizeof(DecThumb) : 0);
    F.thoc_off = F.take(thumbs ? DEC_FLIGHT * sizeof(OcFrame) : 0);
    F.thumb_first = F.need;
    if (thumbs) for (size_t k : F.alive) if (F.fr[k].thumb_bytes) F.fr[k].thumb_off = F.take(F.fr[k].thumb_bytes);
    F.thumb_all = F.need - F.thumb_first;
    F.ds_off = F.take(S.ds ? DS_SLOTS * sizeof(DsPlane) : 0);
    F.res_off = F.take(S.ds ? DS_RES_BYTES : 0);
    F.orig_off = F.need;
    if (S.ds) for (size_t k : F.alive) if (!S.ds->orig[F.job[k]] && S.ds->image[F.job[k]]) (void) F.take(F.fr[k].plane_bytes);
}

/* an arena that holds the flight.  false: it cannot be had, the flight size is halved and the caller tries the same
 * frames again in smaller flights; a single frame that does not fit fails */
static bool dec_flight_room(DecShare &S, DecFlight &F)
{
    if (F.need <= S.arena_b) return true;
    if (S.arena) (void) hipFree(S.arena);
    S.arena = nullptr; S.arena_b = 0;
    if (hipMalloc((void **) &S.arena, F.need) == hipSuccess) { S.arena_b = F.need; return true; }
    if (S.flight > 1) {
        (void) hipGetLastError();
        S.flight = S.flight / 2;
        for (unsigned i : F.job) { S.jobs[i].out = nullptr; S.jobs[i].errmsg[0] = 0; }
        return false;
    }
    dec_flight_fail(S, F, "device decoder: out of device memory");
    return true;
}

/* per frame the automaton, the level-0 images and the zeroed planes; then the descriptors of the frames that got there */
static void dec_flight_upload(DecShare &S, DecFlight &F)
{
    std::vector<size_t> run;
    for (size_t k : F.alive) {
        DecFrame &D = F.fr[k];
        fa_dec_job *j = &S.jobs[F.job[k]];
        if (!dec_run(j, D, S.arena + D.scratch_off, S.stream)) continue;
        DecDesc d;
        d.nodes = (const DecNode *) D.base; d.img = (int16_t *) (D.base + D.nodes_b + D.tops_b + D.mcs_b);
        d.tops = (const DecTop *) (D.base + D.nodes_b); d.planes = D.planes;
        d.S = D.S; d.maxl = D.maxl; d.ntops = D.ntops; d.W = D.W; d.H = D.H;
        F.descs.push_back(d);
        run.push_back(k);
    }
    F.alive.swap(run);
    if (!F.alive.empty() && hipMemcpyAsync(S.arena + F.desc_off, F.descs.data(), F.descs.size() * sizeof(DecDesc), hipMemcpyHostToDevice, S.stream) != hipSuccess)
        dec_flight_fail(S, F, "device decoder: HIP error");
}

/* one launch per level for the whole flight (blockIdx.y = frame), one for the assembly */
static void dec_flight_levels(DecShare &S, DecFlight &F)
{
    if (F.alive.empty()) return;
    unsigned lmax = 0;
    size_t nlev = 0, nasm = 0;                         /* the largest S and the most top-level pixels of the flight */
    for (const DecDesc &d : F.descs) {
        if (d.maxl > lmax) lmax = d.maxl;
        if (d.S > nlev) nlev = d.S;
        if (((size_t) d.ntops << d.maxl) > nasm) nasm = (size_t) d.ntops << d.maxl;
    }
    const DecDesc *dd = (const DecDesc *) (S.arena + F.desc_off);
    for (unsigned l = 1; l < lmax; l++) {              /* (the largest level of a frame: dec_assemble_kernel) */
        const size_t n = nlev << l;
        dec_level_kernel<<<dim3((unsigned) ((n + 255) / 256), (unsigned) F.descs.size()), dim3(256), 0, S.stream>>>(dd, l);
    }
    /* the frames of a call have one format, so a flight has (dec_flight_prepare) */
    const dim3 grid((unsigned) ((nasm + 255) / 256), (unsigned) F.descs.size());
    if (nasm && F.fr[F.alive[0]].c420) dec_assemble420_kernel<<<grid, dim3(256), 0, S.stream>>>(dd);
    else if (nasm) dec_assemble_kernel<<<grid, dim3(256), 0, S.stream>>>(dd);
}

/* the P/B frames of the flight; one that fails drops out alone */
static void dec_flight_mc(DecShare &S, DecFlight &F)
{
    std::vector<size_t> run;
    for (size_t k : F.alive)
        if (S.jobs[F.job[k]].frame_type == FA_I_FRAME || dec_run_mc(&S.jobs[F.job[k]], F.fr[k], S.stream, S.device)) run.push_back(k);
    F.alive.swap(run);
}

/* The planes of the flight that are smoothed -- those of the frames (thumbs false: behind the kernels that wrote them,
 * before every consumer) or the reduced ones of the thumbnails (thumbs true: behind dec_thumb_kernel, before they are
 * written).  The descriptors of the planes that got here, those of the per-pass launches first; the packed tables of
 * the whole flight with one copy (queued with the frames' step, which always runs first); then one launch of
 * sm_pass_kernel per pass index for the planes that take that path (blockIdx.y indexes THEIR part of the table) and ONE
 * launch of sm_frame_kernel for the fused ones (smooth.inc).  The copies read host memory the flight owns and no longer
 * changes (the table is complete before it is queued, F.smhost since dec_flight_prepare) */
static void dec_flight_smooth(DecShare &S, DecFlight &F, bool thumbs)
{
    std::vector<SmDesc> &tab = thumbs ? F.tsmtab : F.smtab;
    const size_t tab_off = thumbs ? F.tsmd_off : F.smd_off;
    bool ok = thumbs || F.smhost.empty() || F.alive.empty()
              || hipMemcpyAsync(S.arena + F.sm_first, F.smhost.data(), F.smhost.size(), hipMemcpyHostToDevice, S.stream) == hipSuccess;
    /* a frame that is smoothed and kept: from here on its copy, the kept planes stay as the kernels above left them */
    for (size_t k : F.alive) {
        DecFrame &D = F.fr[k];
        if (thumbs || !D.shown_copy || D.shown) continue;
        D.shown = (int16_t *) (S.arena + D.scratch_off + D.shown_off);
        ok = ok && hipMemcpyAsync(D.shown, D.planes, D.vals * 2, hipMemcpyDeviceToDevice, S.stream) == hipSuccess;
    }
    unsigned passes = 0;
    unsigned long long fused_most = 0;
    std::vector<const SmPlan *> per;                    /* the planes of the per-pass launches: the first per.size() descriptors */
    for (int fused = 0; fused < 2; fused++)
        for (size_t k : F.alive) {
            DecFrame &D = F.fr[k];
            const SmPlan &P = thumbs ? D.tsm : D.sm;
            if (!P.np || P.fused != (fused != 0)) continue;
            tab.emplace_back();
            sm_describe(tab.back(), thumbs ? D.thumb : dec_shown(D), thumbs ? D.tw : D.W, thumbs ? D.th : D.H, S.arena + P.off, (unsigned) P.borders.size(), P.np,
                        D.sm_is, D.sm_inegs);
            if (!fused) { per.push_back(&P); if (P.np > passes) passes = P.np; }
            else for (unsigned p = 0; p < P.np; p++)
                fused_most = std::max(fused_most, sm_pass_items(F.smhost.data() + (P.off - F.sm_first), (unsigned) P.borders.size(), P.np, p));
        }
    if (ok && tab.empty()) return;
    const SmDesc *d_tab = (const SmDesc *) (S.arena + tab_off);
    ok = ok && hipMemcpyAsync(S.arena + tab_off, tab.data(), tab.size() * sizeof(SmDesc), hipMemcpyHostToDevice, S.stream) == hipSuccess;
    for (unsigned p = 0; ok && p < passes; p++) {
        unsigned long long most = 0;
        for (const SmPlan *P : per)
            most = std::max(most, sm_pass_items(F.smhost.data() + (P->off - F.sm_first), (unsigned) P->borders.size(), P->np, p));
        ok = sm_launch(d_tab, (unsigned) per.size(), p, most, S.stream);
    }
    if (ok) ok = sm_launch_fused(d_tab + per.size(), (unsigned) (tab.size() - per.size()), fused_most, S.stream);
    if (!ok) dec_flight_fail(S, F, "device decoder: HIP error");
}

/* the thumbnails of the flight, behind its level launches: the reduced planes zeroed, ONE launch of dec_thumb_kernel
 * (blockIdx.y = thumbnail) gathers the images of the level shown */
static void dec_flight_thumbs(DecShare &S, DecFlight &F)
{
    size_t nmax = 0;
    for (size_t k : F.alive) {
        DecFrame &D = F.fr[k];
        if (!D.thumb_bytes) continue;
        D.thumb = (int16_t *) (S.arena + D.thumb_off);
        DecThumb t;
        t.img = (const int16_t *) (D.base + D.nodes_b + D.tops_b + D.mcs_b); t.tops = (const DecTop *) (D.base + D.nodes_b); t.planes = D.thumb;
        t.S = D.S; t.l = D.maxl - 2 * S.out->reduce; t.ntops = D.ntops; t.W = D.tw; t.H = D.th; t.shift = S.out->reduce;
        F.thtab.push_back(t);
        if (((size_t) t.ntops << t.l) > nmax) nmax = (size_t) t.ntops << t.l;
    }
    if (F.thtab.empty()) return;
    bool ok = hipMemsetAsync(S.arena + F.thumb_first, 0, F.thumb_all, S.stream) == hipSuccess
              && hipMemcpyAsync(S.arena + F.th_off, F.thtab.data(), F.thtab.size() * sizeof(DecThumb), hipMemcpyHostToDevice, S.stream) == hipSuccess;
    if (ok && nmax) {
        dec_thumb_kernel<<<dim3((unsigned) ((nmax + 255) / 256), (unsigned) F.thtab.size()), dim3(256), 0, S.stream>>>((const DecThumb *) (S.arena + F.th_off));
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ok) dec_flight_fail(S, F, "device decoder: HIP error");
}

/* the frames of the flight against their originals -- ds->orig[job] in place, else the host planes of ds->image[job],
 * copied into the arena --: the result array is zeroed and ONE launch of ds_distortion_kernel fills it.  The frames
 * alive now get the slots; from here on the flight lives or fails as a whole, so a slot stays its frame's */
static void dec_flight_measure(DecShare &S, DecFlight &F)
{
    if (F.alive.empty()) return;
    size_t at = F.orig_off;
    unsigned slot = 0; bool ok = true;
    for (size_t k : F.alive) {
        const fa_dec_job *j = &S.jobs[F.job[k]];
        DecFrame &D = F.fr[k];
        const unsigned bands = j->color ? 3 : 1;
        const size_t npix = (size_t) j->width * j->height;
        const int16_t *o = S.ds->orig[F.job[k]];
        if (!o && !S.ds->image[F.job[k]]) continue;             /* a frame nobody measures */
        if (!o) {
            const fa_image *im = S.ds->image[F.job[k]];
            for (unsigned b = 0; b < bands && ok; b++)
                ok = hipMemcpyAsync(S.arena + at + b * npix * 2, im->pixels[b], npix * 2, hipMemcpyHostToDevice, S.stream) == hipSuccess;
            o = (const int16_t *) (S.arena + at);
            at += D.plane_bytes;
        }
        if (!ok) break;
        D.slot = slot++; D.measured = true;
        ds_describe(F.dstab, D.slot, o, D.planes, j->width, j->height, bands);
    }
    if (ok && F.dstab.empty()) return;
    if (!ok || hipMemsetAsync(S.arena + F.res_off, 0, DS_RES_BYTES, S.stream) != hipSuccess
        || hipMemcpyAsync(S.arena + F.ds_off, F.dstab.data(), F.dstab.size() * sizeof(DsPlane), hipMemcpyHostToDevice, S.stream) != hipSuccess
        || !ds_launch((const DsPlane *) (S.arena + F.ds_off), F.dstab, S.arena + F.res_off, S.ncu, S.stream))
        dec_flight_fail(S, F, "device decoder: HIP error");
}

/* the frames of the flight that have a target into the caller's buffers, once the caller's stream has let go of them:
 * ONE launch of oc_convert_kernel -- or of rd_render_kernel, where the targets are display surfaces (OcOut::render); of
 * oc420_convert_kernel for a 4:2:0 flight, or of rd420_render_kernel where that flight's targets are display surfaces --;
 * one more for the thumbnails, if there are any */
static void dec_flight_write(DecShare &S, DecFlight &F)
{
    unsigned long long total = 0, thtotal = 0;
    if (S.out->planes) {
        /* the planes outlet: no layout forces a kernel -- the shown planes are packed as the image keeps them: one copy */
        std::vector<size_t> run;
        for (size_t k : F.alive) {
            const unsigned i = F.job[k];
            const DecFrame &D = F.fr[k];
            if (S.out->target[i].data) {
                int16_t *buf = S.out->planes[i];
                if (!buf || S.out->planes_dev[i] != S.device || D.vals * 2 != S.out->planes_bytes) {
                    dec_fail(&S.jobs[i], "device decoder: the buffer for the frame's planes does not fit the frame or its device");
                    continue;
                }
                if (hipMemcpyAsync(buf, dec_shown(D), D.vals * 2, hipMemcpyDeviceToDevice, S.stream) != hipSuccess) {
                    (void) hipGetLastError(); dec_fail(&S.jobs[i], "device decoder: HIP error"); continue;
                }
            }
            run.push_back(k);
        }
        F.alive.swap(run);
        return;
    }
    for (size_t k : F.alive) {
        if (F.fr[k].thumb) {
            F.thoctab.emplace_back();
            oc_describe(F.thoctab.back(), F.fr[k].thumb, S.out->thumb[F.job[k]], thtotal);
        }
        if (!S.out->target[F.job[k]].data) continue;            /* measured only, the thumbnail only, or not this frame */
        if (S.out->t420 && S.out->render) {
            F.rd4tab.emplace_back();
            rd4_describe_packed(F.rd4tab.back(), dec_shown(F.fr[k]), S.out->t420[F.job[k]], total);
            continue;
        }
        if (S.out->t420) {
            F.y4tab.emplace_back();
            y4_describe_packed(F.y4tab.back(), dec_shown(F.fr[k]), S.out->t420[F.job[k]], total);
            continue;
        }
        F.octab.emplace_back();
        oc_describe(F.octab.back(), dec_shown(F.fr[k]), S.out->target[F.job[k]], total);
    }
    if (F.octab.empty() && F.thoctab.empty() && F.y4tab.empty() && F.rd4tab.empty()) return;
    bool ok = hipStreamWaitEvent(S.stream, S.out->ready, 0) == hipSuccess;
    static_assert(sizeof(Rd4Frame) <= sizeof(Y4Frame), "the table of a 4:2:0 flight is carved for Y4Frame entries");
    if (ok && !F.rd4tab.empty())
        ok = hipMemcpyAsync(S.arena + F.oc_off, F.rd4tab.data(), F.rd4tab.size() * sizeof(Rd4Frame), hipMemcpyHostToDevice, S.stream) == hipSuccess
             && rd4_launch((const Rd4Frame *) (S.arena + F.oc_off), (unsigned) F.rd4tab.size(), total, S.out->render, S.ncu, S.stream);
    if (ok && !F.y4tab.empty())
        ok = hipMemcpyAsync(S.arena + F.oc_off, F.y4tab.data(), F.y4tab.size() * sizeof(Y4Frame), hipMemcpyHostToDevice, S.stream) == hipSuccess
             && y4_launch((const Y4Frame *) (S.arena + F.oc_off), (unsigned) F.y4tab.size(), total, S.ncu, S.stream);
    if (ok && !F.octab.empty())
        ok = hipMemcpyAsync(S.arena + F.oc_off, F.octab.data(), F.octab.size() * sizeof(OcFrame), hipMemcpyHostToDevice, S.stream) == hipSuccess
             && (S.out->render ? rd_launch((const OcFrame *) (S.arena + F.oc_off), (unsigned) F.octab.size(), total, S.out->render, S.ncu, S.stream)
                                : oc_launch((const OcFrame *) (S.arena + F.oc_off), (unsigned) F.octab.size(), total, S.ncu, S.stream));
    if (ok && !F.thoctab.empty())
        ok = hipMemcpyAsync(S.arena + F.thoc_off, F.thoctab.data(), F.thoctab.size() * sizeof(OcFrame), hipMemcpyHostToDevice, S.stream) == hipSuccess
             && oc_launch((const OcFrame *) (S.arena + F.thoc_off), (unsigned) F.thoctab.size(), thtotal, S.ncu, S.stream);
    if (!ok) dec_flight_fail(S, F, "device decoder: HIP error");
}

/* the end of the flight's device work; measuring: 12 bytes per band come back */
static void dec_flight_wait(DecShare &S, DecFlight &F)
{
    (void) hipEventRecord(S.ev1, S.stream);
    if (hipStreamSynchronize(S.stream) != hipSuccess) dec_flight_fail(S, F, "device decoder: kernel failed");
    if (S.ds && !F.alive.empty() && !F.dstab.empty() && hipMemcpy(F.dsres.bytes, S.arena + F.res_off, DS_RES_BYTES, hipMemcpyDeviceToHost) != hipSuccess)
        dec_flight_fail(S, F, "device decoder: download failed");
}

/* a frame nobody consumed on the device: its planes as a host image, which keeps the device planes of a keep_dev frame */
static bool dec_download(DecShare &S, fa_dec_job *j, DecFrame &D)
{
    fa_image *im = fa_image_alloc(D.W, D.H, j->color);
    const size_t npix = (size_t) D.W * D.H, cpix = D.c420 ? (size_t) (D.W >> 1) * (D.H >> 1) : npix;     /* 4:2:0: the chroma planes at the beginning of theirs */
    bool ok = im != nullptr;
    for (int b = 0; ok && b < (j->color ? 3 : 1); b++)
        ok = hipMemcpy(im->pixels[b], D.planes + (b ? npix + (size_t) (b - 1) * cpix : 0), (b ? cpix : npix) * 2, hipMemcpyDeviceToHost) == hipSuccess;
    if (ok) j->out_420 = D.c420;
    if (!ok) { fa_image_free(im); dec_fail(j, "device decoder: download failed"); return false; }
    if (D.own_planes) { im->dev = D.planes; im->dev_id = S.device; D.planes = nullptr; }
    j->out = im;
    return true;
}

/* what the frames alive at the end get: done[] and the sums, or a host image; and the statistics.  Pixels: 2 bytes
 * read per pixel and band, the 8-bit pixel written; measuring: 2 bytes read per side; smoothing: a pixel pair is read
 * and written, 8 bytes */
static void dec_flight_results(DecShare &S, DecFlight &F)
{
    float ms = 0;
    if (hipEventElapsedTime(&ms, S.ev0, S.ev1) != hipSuccess) { (void) hipGetLastError(); ms = 0; }
    unsigned frames = 0;
    unsigned long long bytes = 0;
    const unsigned *mx = (const unsigned *) (F.dsres.bytes + DS_SLOTS * sizeof(unsigned long long));
    for (size_t k : F.alive) {
        const unsigned i = F.job[k];
        fa_dec_job *j = &S.jobs[i];
        DecFrame &D = F.fr[k];
        const unsigned bands = j->color ? 3 : 1;
        const unsigned long long vals = D.vals;
        const bool written = S.out && S.out->target[i].data;
        if (written) S.out->done[i] = 1;
        const unsigned long long tvals = D.thumb ? (unsigned long long) D.tw * D.th * bands : 0ull;     /* gathered: 2 + 2 bytes; written: 2 + 1 */
        if (D.thumb) S.out->thumb_done[i] = 1;
        if (S.ds && D.measured) {
            for (unsigned b = 0; b < bands; b++) {
                if (S.ds->sse) S.ds->sse[(size_t) i * 3 + b] = F.dsres.sums[D.slot * 3 + b];
                if (S.ds->maxdiff) S.ds->maxdiff[(size_t) i * 3 + b] = mx[D.slot * 3 + b];
            }
            S.ds->done[i] = 1;
        }
        if ((S.images || (!S.out && !S.ds)) && !dec_download(S, j, D)) continue;
        if (j->from_stream && !j->out) {
            /* a frame of a walked stream whose consumers are on the device: an image without host planes says that it is
             * decoded, and holds the planes the next frame is predicted from */
            fa_image *im = (fa_image *) calloc(1, sizeof *im);
            if (!im) { dec_fail(j, "Out of memory!"); continue; }
            im->width = D.W; im->height = D.H; im->color = j->color;
            if (D.own_planes) { im->dev = D.planes; im->dev_id = S.device; D.planes = nullptr; }
            j->out = im; j->out_420 = D.c420;
        }
        frames++;
        bytes += D.bytes + (S.ds ? 4 * vals : 0) + (written ? 3 * vals : 0) + 7 * tvals + (D.sm.np ? 8 * D.sm.pairs : 0) + (D.thumb && D.tsm.np ? 8 * D.tsm.pairs : 0);
    }
    dec_account((unsigned long long) (ms * 1000.0f), frames, bytes);
    S.good += (int) frames;
}

/* what the frames allocated for themselves, failed or not; the planes a host image took over stay */
static void dec_flight_release(DecFlight &F)
{
    for (DecFrame &D : F.fr) {
        if (D.own_planes && D.planes) (void) hipFree(D.planes);
        if (D.past) (void) hipFree(D.past);
        if (D.future) (void) hipFree(D.future);
    }
}

/* originals read in place: the conversion that wrote them may still run on the upload stream of the share that owns
 * them (ic_fetch waits on the host for the same reason; here the stream waits), once per owner */
static void dec_share_wait_originals(DecShare &S, const std::vector<unsigned> &todo)
{
    std::vector<const Staged *> seen;
    for (unsigned i : todo) {
        const Staged *own = S.ds->orig[i] ? (const Staged *) S.ds->image[i]->src_owner : nullptr;
        if (!own || !own->ev_up || std::find(seen.begin(), seen.end(), own) != seen.end()) continue;
        seen.push_back(own);
        if (hipStreamWaitEvent(S.stream, own->ev_up, 0) != hipSuccess) (void) hipGetLastError();
    }
}

/* the caller's stream behind the conversions: it may read the pixels without a host synchronisation */
static void dec_share_release_caller(DecShare &S)
{
    hipEvent_t written = nullptr;
    if (hipEventCreateWithFlags(&written, hipEventDisableTiming) != hipSuccess || hipEventRecord(written, S.stream) != hipSuccess
        || hipStreamWaitEvent(S.out->caller, written, 0) != hipSuccess) (void) hipGetLastError();
    if (written) (void) hipEventDestroy(written);
}

/* What a share makes per call -- its stream, the two events and the arena -- kept between the calls of a caller that comes
 * again: a fiasco_decoder_t owns one (OcOut::keep, decoder_outlet.inc) for its lifetime, so a call for one display frame
 * costs its flight and no stream, event or arena.  The arena only grows.  A stream's jobs carry one share key, so one share
 * serves the decoder (decode_frames refuses a call with a DecKeep whose jobs are dealt to more); should the share's device change between calls, what is kept is released and made again there.
 * Between calls nothing of it is in use: every flight ends with a wait for its stream */
struct DecKeep {
    int         device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t  ev0 = nullptr, ev1 = nullptr;
    char       *arena = nullptr; size_t arena_b = 0;
};

static void dec_keep_release(DecKeep &K)
{
    int cur = -1;
    bool moved = false;
    if (K.device >= 0 && hipGetDevice(&cur) == hipSuccess && cur != K.device) moved = hipSetDevice(K.device) == hipSuccess;
    if (K.arena) (void) hipFree(K.arena);
    if (K.ev0) (void) hipEventDestroy(K.ev0);
    if (K.ev1) (void) hipEventDestroy(K.ev1);
    if (K.stream) (void) hipStreamDestroy(K.stream);
    (void) hipGetLastError();
    if (moved) (void) hipSetDevice(cur);
    K = DecKeep();
}

/* the jobs `mine' of a call on this thread's device, in flights.  Returns the number of frames decoded */
static int decode_share(fa_dec_job *jobs, const std::vector<unsigned> &mine, const OcOut *out, const DsOut *ds, bool images)
{
    DecShare S;
    S.jobs = jobs; S.out = out; S.ds = ds; S.images = images;
    DecKeep *K = out ? out->keep : nullptr;
    bool usable = hipGetDevice(&S.device) == hipSuccess;
    if (K && K->stream && (!usable || K->device != S.device)) dec_keep_release(*K);
    if (usable && K && K->stream) { S.stream = K->stream; S.ev0 = K->ev0; S.ev1 = K->ev1; S.arena = K->arena; S.arena_b = K->arena_b; }
    else {
        usable = usable && hipStreamCreate(&S.stream) == hipSuccess;
        if (usable && (hipEventCreate(&S.ev0) != hipSuccess || hipEventCreate(&S.ev1) != hipSuccess)) (void) hipGetLastError();
    }
    if (usable) S.ncu = ft_cus();
    if (!usable) (void) hipGetLastError();
    std::vector<unsigned> todo;
    for (unsigned i : mine) {
        fa_dec_job *j = &jobs[i];
        j->out = nullptr; j->errmsg[0] = 0;
        if (j->skip) continue;
        if (!usable) { dec_fail(j, "libfiasco_amd: no usable HIP device (the decoder runs on the device; there is no CPU path)"); continue; }
        todo.push_back(i);
    }
    if (ds && S.stream) dec_share_wait_originals(S, todo);
    for (size_t f0 = 0; f0 < todo.size(); ) {
        const size_t n = S.flight < todo.size() - f0 ? S.flight : todo.size() - f0;
        DecFlight F;
        dec_flight_prepare(S, F, &todo[f0], n);
        if (!dec_flight_room(S, F)) continue;
        (void) hipEventRecord(S.ev0, S.stream);
        dec_flight_upload(S, F);
        dec_flight_levels(S, F);
        dec_flight_mc(S, F);
        dec_flight_smooth(S, F, false);
        if (out && out->thumb) { dec_flight_thumbs(S, F); dec_flight_smooth(S, F, true); }
        if (ds) dec_flight_measure(S, F);
        if (out) dec_flight_write(S, F);
        dec_flight_wait(S, F);
        dec_flight_results(S, F);
        dec_flight_release(F);
        f0 += n;
    }
    if (out && !out->planes && S.stream) dec_share_release_caller(S);
    if (K && usable) {
        K->device = S.device; K->stream = S.stream; K->ev0 = S.ev0; K->ev1 = S.ev1; K->arena = S.arena; K->arena_b = S.arena_b;
        return S.good;
    }
    if (S.arena) (void) hipFree(S.arena);
    if (S.ev0) (void) hipEventDestroy(S.ev0);
    if (S.ev1) (void) hipEventDestroy(S.ev1);
    if (S.stream) (void) hipStreamDestroy(S.stream);
    return S.good;
}

/* decode n frames: dealt to the shares by the rule of dec_shares / dec_share_of (shares.inc), the shares decode side
 * by side, each on its own host thread (share 0 on the caller's; for_shares, shares.inc).  Returns the number of
 * frames decoded; a failed job has out == NULL and a message. */
static int decode_frames(unsigned n, fa_dec_job *jobs, const OcOut *out, const DsOut *ds, bool images)
{
    const size_t ND = dec_shares(n, jobs);
    std::vector<std::vector<unsigned> > deal(ND);
    for (unsigned i = 0; i < n; i++) deal[dec_share_of(jobs, i, ND)].push_back(i);
    std::vector<size_t> share;
    for (size_t k = 0; k < ND; k++) if (!deal[k].empty()) share.push_back(k);
    if (share.empty()) return 0;
    /* what a caller keeps between calls (OcOut::keep) is ONE stream and ONE arena: two shares must never adopt it at once */
    if (out && out->keep && share.size() > 1) {
        for (unsigned i = 0; i < n; i++) if (!jobs[i].skip) dec_fail(&jobs[i], "device decoder: jobs with a kept share context were dealt to more than one share (they must carry one share key)");
        return 0;
    }
    std::vector<int> goodv(share.size(), 0);
    for_shares(share, [&](size_t part) { goodv[part] = decode_share(jobs, deal[share[part]], out, ds, images); });
    int good = 0;
    for (size_t k = 0; k < goodv.size(); k++) good += goodv[k];
    return good;
}

/* The seam.  Jobs that name consumers (fa_host.h: target, sse, maxdiff -- the outputs of a sequence) get them attached to
 * the steps their flights have anyway: dec_flight_write and dec_flight_measure.  Such a frame is written, measured AND
 * handed back as an image: the sequence engine predicts the next frame from it.  Targets were checked when they were
 * set (fiasco_amd_seq_set_outputs_device).  The original is read in place where it lies on the device the job is decoded
 * on, else copied up from its host planes (a PNM-fed frame has them, a frame on another device fetches them). */
extern "C" int fa_core_decode_frames(unsigned n, fa_dec_job *jobs)
{
    bool pixels = false, sums = false;
    void *caller = nullptr;
    for (unsigned i = 0; i < n; i++) {
        jobs[i].delivered = 0;
        if (jobs[i].skip) continue;
        const fiasco_amd_device_target *t = (const fiasco_amd_device_target *) jobs[i].target;
        if (t && t->data) { pixels = true; caller = jobs[i].consumer_stream; }
        if ((jobs[i].sse || jobs[i].maxdiff) && jobs[i].orig) sums = true;
    }
    if (!pixels && !sums) return decode_frames(n, jobs, nullptr, nullptr, false);
    std::vector<fiasco_amd_device_frame> target(n, fiasco_amd_device_frame());
    std::vector<unsigned char> written(n, 0), measured(n, 0);
    std::vector<const int16_t *> orig(n, nullptr);
    std::vector<const fa_image *> image(n, nullptr);
    std::vector<unsigned long long> sse((size_t) n * 3, 0);
    std::vector<unsigned> maxdiff((size_t) n * 3, 0);
    const size_t shares = dec_shares(n, jobs);
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess) { (void) hipGetLastError(); cur = -1; }
    for (unsigned i = 0; i < n; i++) {
        fa_dec_job *j = &jobs[i];
        if (j->skip) continue;
        const fiasco_amd_device_target *t = (const fiasco_amd_device_target *) j->target;
        if (t && t->data) {
            fiasco_amd_device_frame &f = target[i];
            f.data = t->data; f.pitch = t->pitch; f.plane_stride = t->plane_stride; f.width = t->width; f.height = t->height; f.layout = t->layout;
            if (!f.pitch) f.pitch = ic_row_bytes(f);
            if (!f.plane_stride) f.plane_stride = f.pitch * f.height;
        }
        if ((j->sse || j->maxdiff) && j->orig) {
            image[i] = j->orig;
            if (j->orig->src_dev && j->orig->src_dev_id == dec_device_of(jobs, i, shares, cur)) orig[i] = j->orig->src_dev;
            else if (!fa_image_host_planes(j->orig)) image[i] = nullptr;       /* decoded, not measured: not delivered */
        }
    }
    OcOut out;
    out.target = target.data(); out.done = written.data(); out.caller = (hipStream_t) caller; out.ready = nullptr;
    if (pixels) {
        out.ready = ic_mark_ready(caller);
        if (!out.ready) {
            for (unsigned i = 0; i < n; i++) if (!jobs[i].skip) dec_fail(&jobs[i], fiasco_get_error_message());
            return 0;
        }
    }
    DsOut ds;
    ds.orig = orig.data(); ds.image = image.data(); ds.sse = sse.data(); ds.maxdiff = maxdiff.data(); ds.done = measured.data();
    const int good = decode_frames(n, jobs, pixels ? &out : nullptr, sums ? &ds : nullptr, true);
    if (out.ready) (void) hipEventDestroy(out.ready);
    for (unsigned i = 0; i < n; i++) {
        fa_dec_job *j = &jobs[i];
        if (j->skip || !j->out) continue;
        const bool wants_pixels = target[i].data != nullptr, wants_sums = image[i] != nullptr;
        if ((wants_pixels && !written[i]) || (wants_sums && !measured[i]) || (!wants_pixels && !wants_sums)) continue;
        for (unsigned b = 0; wants_sums && b < 3; b++) {
            if (j->sse) j->sse[b] = sse[(size_t) i * 3 + b];
            if (j->maxdiff) j->maxdiff[b] = maxdiff[(size_t) i * 3 + b];
        }
        j->delivered = 1;
    }
    return good;
}
