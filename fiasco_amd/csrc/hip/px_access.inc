/*
 *  px_access.inc -- what the pixel kernels (ic_convert_kernel, icy_convert_kernel, oc_convert_kernel, oc420_convert_kernel,
 *  rd_render_kernel, rd420_render_kernel; the smoothing and measuring kernels beside them) read and write at the ragged ends of their rows:
 *  the partial 16-byte accesses of a work item, and the one switch that turns them and the per-item functions built on
 *  them into plain C++ (included by core_hip.cpp ahead of those files, and by each of them under its replay switch).
 *
 *  The contract, which the step checks (the tests' step_check programs, built with the sanitizers, guard bytes around every
 *  plane and between its rows) enforce: a load reads exactly the `n' valid elements it is told about and hands back zero
 *  for the rest, a store writes exactly `nb' bytes (`n' values), at ANY alignment the caller may pass -- the element's own
 *  for the 16-bit accesses, none for the bytes.  An access never rounds its range up to a wider unit.
 *
 *  Two accesses come in two variants that differ only in the widths they try before they fall back to single elements:
 *    px_load_bytes_vec  / px_load_bytes_wide     the 16-byte vector or bytes / 16, 8, 4 bytes, then bytes
 *    px_store_bytes_vec / px_store_bytes_wide    the 16-byte vector or bytes / the widest the address allows
 *  Every kernel keeps the variant it was written with.  Giving a kernel the other one changes its code: that is a
 *  question of speed to be measured on its own, not a clean-up.
 *
 *  PX_HOST_REPLAY: everything here as plain C++ -- no address space, structs in place of the vector types.  A step check
 *  defines the switch of the file it replays (Y420_HOST_REPLAY, RENDER_HOST_REPLAY, RENDER420_HOST_REPLAY, YCBCR_IN_HOST_REPLAY,
 *  SMOOTH_HOST_REPLAY); that switch turns this one on and selects which part of its file is compiled.
 */
#ifndef PX_ACCESS_INC
#define PX_ACCESS_INC

#ifdef PX_HOST_REPLAY
#define PX_DEV static inline
#define PX_GLOBAL
#define PX_UNROLL           /* a pragma the host compilers of the step checks do not know, and warn about */
struct alignas(16) px_u4 { unsigned x, y, z, w; };
struct alignas(8) px_u2 { unsigned x, y; };
#else
#define PX_DEV static __device__ __forceinline__
/* sources and targets come out of descriptor tables: the compiler cannot see that they are global memory and would use
 * flat loads and stores */
#define PX_GLOBAL __attribute__((address_space(1)))
#define PX_UNROLL _Pragma("unroll")
typedef unsigned px_u4 __attribute__((ext_vector_type(4)));
typedef unsigned px_u2 __attribute__((ext_vector_type(2)));
#endif

typedef unsigned short px_h;

/* ------------------------------------------------------------------ bytes */

/* `n' bytes (at most 16) from p into w[0 .. 3], the rest reads as zero: one vector load, or byte loads */
PX_DEV void px_load_bytes_vec(const unsigned char *p, unsigned n, unsigned w[4])
{
    if (n == 16 && ((size_t) p & 15) == 0) {
        const px_u4 v = *(const PX_GLOBAL px_u4 *) p;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
    w[0] = w[1] = w[2] = w[3] = 0;
    PX_UNROLL
    for (unsigned k = 0; k < 16; k++)
        if (k < n) w[k >> 2] |= (unsigned) ((const PX_GLOBAL unsigned char *) p)[k] << (8 * (k & 3));
}

/* the same: 16-, 8- or 4-byte loads where the address and n allow them, byte loads otherwise */
PX_DEV void px_load_bytes_wide(const unsigned char *p, unsigned n, unsigned w[4])
{
    if (n == 16 && ((size_t) p & 15) == 0) {
        const px_u4 v = *(const PX_GLOBAL px_u4 *) p;
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if (n == 16 && ((size_t) p & 7) == 0) {
        const px_u2 a = ((const PX_GLOBAL px_u2 *) p)[0], b = ((const PX_GLOBAL px_u2 *) p)[1];
        w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y;
    } else if (!(n & 3) && ((size_t) p & 3) == 0) {
        PX_UNROLL
        for (unsigned k = 0; k < 4; k++) w[k] = 4 * k < n ? ((const PX_GLOBAL unsigned *) p)[k] : 0u;
    } else {
        w[0] = w[1] = w[2] = w[3] = 0;
        PX_UNROLL
        for (unsigned k = 0; k < 16; k++)
            if (k < n) w[k >> 2] |= (unsigned) ((const PX_GLOBAL unsigned char *) p)[k] << (8 * (k & 3));
    }
}

/* `n' bytes (at most 8) from p into w[0 .. 1], the rest reads as zero: 8- or 4-byte loads, or byte loads */
PX_DEV void px_load_bytes8(const unsigned char *p, unsigned n, unsigned w[2])
{
    if (n == 8 && ((size_t) p & 7) == 0) {
        const px_u2 a = *(const PX_GLOBAL px_u2 *) p;
        w[0] = a.x; w[1] = a.y;
    } else if (!(n & 3) && ((size_t) p & 3) == 0) {
        PX_UNROLL
        for (unsigned k = 0; k < 2; k++) w[k] = 4 * k < n ? ((const PX_GLOBAL unsigned *) p)[k] : 0u;
    } else {
        w[0] = w[1] = 0;
        PX_UNROLL
        for (unsigned k = 0; k < 8; k++)
            if (k < n) w[k >> 2] |= (unsigned) ((const PX_GLOBAL unsigned char *) p)[k] << (8 * (k & 3));
    }
}

/* `nb' bytes (at most 16) of w to q: one vector store, or byte stores */
PX_DEV void px_store_bytes_vec(unsigned char *q, unsigned nb, const unsigned w[4])
{
    if (nb == 16 && ((size_t) q & 15) == 0) { *(PX_GLOBAL px_u4 *) q = px_u4{ w[0], w[1], w[2], w[3] }; return; }
    PX_UNROLL
    for (unsigned k = 0; k < 16; k++)
        if (k < nb) ((PX_GLOBAL unsigned char *) q)[k] = (unsigned char) (w[k >> 2] >> (8 * (k & 3)));
}

/* the same: one 16-byte store, or 4-, 2- and 1-byte stores, the widest the address allows */
PX_DEV void px_store_bytes_wide(unsigned char *q, unsigned nb, const unsigned w[4])
{
    if (nb == 16 && ((size_t) q & 15) == 0) { *(PX_GLOBAL px_u4 *) q = px_u4{ w[0], w[1], w[2], w[3] }; return; }
    const unsigned unit = ((size_t) q & 3) == 0 ? 4 : ((size_t) q & 1) == 0 ? 2 : 1;
    PX_UNROLL
    for (unsigned k = 0; k < 4; k++) {
        if (unit == 4 && 4 * k + 4 <= nb) { ((PX_GLOBAL unsigned *) q)[k] = w[k]; continue; }
        PX_UNROLL
        for (unsigned h = 0; h < 2; h++) {
            const unsigned at = 4 * k + 2 * h, half = (w[k] >> (16 * h)) & 0xffffu;
            if (unit >= 2 && at + 2 <= nb) { ((PX_GLOBAL px_h *) q)[2 * k + h] = (px_h) half; continue; }
            if (at < nb) ((PX_GLOBAL unsigned char *) q)[at] = (unsigned char) half;
            if (at + 1 < nb) ((PX_GLOBAL unsigned char *) q)[at + 1] = (unsigned char) (half >> 8);
        }
    }
}

/* ------------------------------------------------------------------ 16 values of 16 bits as eight packed pairs */

/* `n' values (at most 16) from p, the rest reads as zero: 16-, 8- or 4-byte loads where the address and n allow them,
 * 2-byte loads otherwise */
PX_DEV void px_load_values(const int16_t *p, unsigned n, unsigned v[8])
{
    if (n == 16 && ((size_t) p & 15) == 0) {
        const px_u4 a = ((const PX_GLOBAL px_u4 *) p)[0], b = ((const PX_GLOBAL px_u4 *) p)[1];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else if (n == 16 && ((size_t) p & 7) == 0) {
        PX_UNROLL
        for (unsigned k = 0; k < 4; k++) { const px_u2 a = ((const PX_GLOBAL px_u2 *) p)[k]; v[2 * k] = a.x; v[2 * k + 1] = a.y; }
    } else if (!(n & 1) && ((size_t) p & 3) == 0) {
        PX_UNROLL
        for (unsigned k = 0; k < 8; k++) v[k] = 2 * k < n ? ((const PX_GLOBAL unsigned *) p)[k] : 0u;
    } else {
        PX_UNROLL
        for (unsigned k = 0; k < 8; k++) {
            const unsigned lo = 2 * k < n ? ((const PX_GLOBAL px_h *) p)[2 * k] : 0u, hi = 2 * k + 1 < n ? ((const PX_GLOBAL px_h *) p)[2 * k + 1] : 0u;
            v[k] = lo | (hi << 16);
        }
    }
}

/* `n' values (at most 16, n even) to q, which is 4-byte aligned: 16-, 8- or 4-byte stores */
PX_DEV void px_store_values(int16_t *q, unsigned n, const unsigned v[8])
{
    if (n == 16 && ((size_t) q & 15) == 0) {
        ((PX_GLOBAL px_u4 *) q)[0] = px_u4{ v[0], v[1], v[2], v[3] };
        ((PX_GLOBAL px_u4 *) q)[1] = px_u4{ v[4], v[5], v[6], v[7] };
    } else if (n == 16 && ((size_t) q & 7) == 0) {
        PX_UNROLL
        for (unsigned k = 0; k < 4; k++) ((PX_GLOBAL px_u2 *) q)[k] = px_u2{ v[2 * k], v[2 * k + 1] };
    } else {
        PX_UNROLL
        for (unsigned k = 0; k < 8; k++)
            if (2 * k < n) ((PX_GLOBAL unsigned *) q)[k] = v[k];
    }
}

/* value k of 16 packed ones, arithmetically shifted: the integer part of a 12.4 pixel */
PX_DEV int px_int(const unsigned *v, unsigned k) { return (int) (int16_t) (v[k >> 1] >> (16 * (k & 1))) >> 4; }
PX_DEV unsigned px_clip255(int v) { return (unsigned) (v < 0 ? 0 : v > 255 ? 255 : v); }

#endif      /* PX_ACCESS_INC */
