/*
 *  dec_mc.h -- the geometry of motion compensation in the device decoder (frame_decoder.inc), as plain functions that
 *  compile as C and as HIP: the block list of a frame that is shown magnified, and the addresses of one work item of
 *  dec_mc420_kernel.  tests/stream_check.c replays both on the host against a loop written from restore_mc's text.
 *
 *  restore_mc (codec/motion.c:37-229) works on the automaton as enlarge_image left it (codec/decoder.c:776-840): for a
 *  magnification M the coordinates of a block are shifted by M, its level is 2 M higher, and every vector component is
 *  doubled M times or halved -M times, one step at a time, with C's division toward zero.  In a 4:2:0 frame the blocks
 *  of the two chroma bands have half the coordinates, half the sides and half the vector components (FX, :51), again
 *  toward zero, in planes of half the width; the addressing is linear in every plane.
 */
#ifndef FA_DEC_MC_H
#define FA_DEC_MC_H
#include <stdint.h>

#ifndef DEC_MC_FN
#define DEC_MC_FN static inline
#endif

typedef struct DecMc { int32_t x0, y0, level, type, fx, fy, bx, by; } DecMc;

/* the block of a (state, label) whose range has the coded level `level', at (x, y), as it is compensated at
 * magnification mag.  0: its level falls below 0 (the caller refuses the frame, as the reduction rule for the blocks of an
 * intra frame does) */
DEC_MC_FN int dec_mc_scaled(DecMc *m, unsigned x, unsigned y, int level, int type, int fx, int fy, int bx, int by, int mag)
{
    int v[4], n, k;
    v[0] = fx; v[1] = fy; v[2] = bx; v[3] = by;
    for (n = mag; n > 0; n--) for (k = 0; k < 4; k++) v[k] = (int16_t) (v[k] * 2);       /* word_t, as the reference holds them */
    for (n = -mag; n > 0; n--) for (k = 0; k < 4; k++) v[k] /= 2;
    m->x0 = (int32_t) (mag > 0 ? x << mag : x >> -mag);
    m->y0 = (int32_t) (mag > 0 ? y << mag : y >> -mag);
    m->level = level + 2 * mag;
    m->type = type; m->fx = v[0]; m->fy = v[1]; m->bx = v[2]; m->by = v[3];
    return m->level >= 0;
}

/* Work item p of block mc in band b of a 4:2:0 frame of W x H pixels (planes Y [H][W], Cb, Cr [H >> 1][W >> 1] back to
 * back).  *base: where the band's plane begins, in values; *npix: its size; *di, *fi, *bi: the value added to, the value
 * of the past frame and the value of the future frame, from the plane's base (linear, as restore_mc addresses).  0: the
 * item lies outside the block of this band.  The caller checks di, fi, bi against 0 .. *npix - 1 */
DEC_MC_FN int dec_mc420_item(const DecMc *mc, unsigned b, unsigned p, unsigned W, unsigned H, unsigned long long *base,
                             long long *npix, long long *di, long long *fi, long long *bi)
{
    const unsigned wl = (unsigned) mc->level >> 1;
    const unsigned half = b ? 1u : 0u;
    const long long x = p & ((1u << wl) - 1), y = p >> wl;
    const long long bw = (1u << wl) >> half, bh = (1u << (((unsigned) mc->level + 1) >> 1)) >> half;
    const long long pw = W >> half;
    const long long x0 = mc->x0 / (half ? 2 : 1), y0 = mc->y0 / (half ? 2 : 1);
    const long long fx = mc->fx / (half ? 2 : 1), fy = mc->fy / (half ? 2 : 1);
    const long long bx = mc->bx / (half ? 2 : 1), by = mc->by / (half ? 2 : 1);
    if (p >= (1u << mc->level) || x >= bw || y >= bh) return 0;
    *npix = pw * (long long) (H >> half);
    *base = b ? (unsigned long long) W * H + (unsigned long long) (b - 1) * (unsigned long long) *npix : 0ull;
    *di = (y0 + y) * pw + x0 + x;
    *fi = (y0 + fy + y) * pw + x0 + fx + x;
    *bi = (y0 + by + y) * pw + x0 + bx + x;
    return 1;
}

#endif
