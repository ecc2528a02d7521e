"""Frames that are YCbCr already (include/libfiasco_amd_ycbcr.h): the library's definition of their planes in numpy, and what
tests/test_ycbcr_input_api.py (CPU) and tests/test_gpu_ycbcr_input.py (device) share -- frames, their layouts in memory, the
gray values on which the PNM reader and the definition agree.  No codec logic here.

    Y [y][x] = (Ybyte [y][x]            - 128) * 16
    Cb[y][x] = (Cbbyte[y >> s][x >> s]  - 128) * 16      s = 1 for 4:2:0, 0 for 4:4:4
    Cr[y][x] = (Crbyte[y >> s][x >> s]  - 128) * 16
"""
import numpy as np

import synth

SIZES = [(32, 32), (38, 34), (48, 70), (102, 66), (160, 120)]       # width x height
KINDS = ["nv12", "nv21", "i420", "444"]


def planes(y, cb, cr, s):
    """int16 [3][H][W]: the planes the coder sees for 8-bit Y [H][W] and Cb, Cr [H >> s][W >> s]"""
    h, w = y.shape
    assert s in (0, 1) and cb.shape == cr.shape == (h >> s, w >> s)
    up = (lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)) if s else (lambda c: c)
    return np.stack([(p.astype(np.int16) - 128) * 16 for p in (y, up(cb), up(cr))])


def bytes_of(p):
    """clip255((planes >> 4) + 128): the bytes the decoder writes for planes, and the distortion kernel compares"""
    return np.clip((p.astype(np.int32) >> 4) + 128, 0, 255).astype(np.uint8)


def every_value(w, h, s, seed=0):
    """(y, cb, cr): Y walks through every byte value, and so do Cb and -- permuted -- Cr: at 32 x 32 in 4:2:0 the 16 x 16
    chroma samples are exactly the 256 values"""
    cw, ch = w >> s, h >> s
    y = ((np.arange(w * h, dtype=np.int64) * 7 + seed) % 256).astype(np.uint8).reshape(h, w)
    cb = ((np.arange(cw * ch, dtype=np.int64) + seed) % 256).astype(np.uint8).reshape(ch, cw)
    cr = ((cb.astype(np.int64) * 167 + 13) % 256).astype(np.uint8)           # 167 is odd: a permutation of the byte values
    return y, cb, cr


def textured(w, h, s, seed=1234, shift=0):
    """(y, cb, cr) with content a coder has something to do with: the bytes of the PNM reader's planes of the synthetic colour
    frame synth.synth_color_k -- textured Y, chroma that varies smoothly and survives the coder --, the chroma sampled at
    (2 i, 2 j) for 4:2:0.  (Chroma as busy as Y makes the writer of a small frame give up with the reference's own "Can't
    write more than N weights.", through PNM as well.)"""
    p = bytes_of(pnm_planes(synth.synth_color_k(w, h, seed, shift)))
    step = 2 if s else 1
    return p[0].copy(), p[1][::step, ::step].copy(), p[2][::step, ::step].copy()


def layout(kind, y, cb, cr, pad=0, put=lambda a: a):
    """-> (frame, order): the frame as Batch.from_ycbcr / from_device_ycbcr take it -- (y, cbcr) for "nv12" and "nv21", (y, cb, cr)
    for "i420" (chroma of half the size) and "444" (of the full size).  pad: every row lies inside a row `pad' samples longer,
    so the pitches are larger than the rows.  put: where the arrays go before they are cut (identity: numpy on the host)."""
    def rows(a):
        if not pad:
            return put(np.ascontiguousarray(a))
        big = np.full((a.shape[0], a.shape[1] + pad) + a.shape[2:], 0x5a, dtype=np.uint8)
        big[:, :a.shape[1]] = a
        return put(big)[:, :a.shape[1]]
    assert kind in KINDS and cb.shape == (y.shape if kind == "444" else (y.shape[0] // 2, y.shape[1] // 2))
    if kind == "nv12":
        return (rows(y), rows(np.stack([cb, cr], axis=-1))), "nv12"
    if kind == "nv21":
        return (rows(y), rows(np.stack([cr, cb], axis=-1))), "nv21"
    return (rows(y), rows(cb), rows(cr)), "nv12"


def pnm_planes(rgb):
    """the PNM reader's planes of 8-bit R, G, B [..., 3] (host/fa_image.c convert_planes; numpy_planes of
    tests/test_gpu_device_input.py): float64, left to right, truncated"""
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    y = ((+0.2989 * r + 0.5866 * g + 0.1145 * b - 128) * 16).astype(np.int32).astype(np.int16)
    cb = ((-0.1687 * r - 0.3312 * g + 0.5000 * b) * 16).astype(np.int32).astype(np.int16)
    cr = ((+0.5000 * r - 0.4183 * g - 0.0816 * b) * 16).astype(np.int32).astype(np.int16)
    return np.stack([y, cb, cr])


# gray values v for which the PNM reader's arithmetic on r = g = b = v does NOT give ((v - 128) * 16, 0, 0)
EXCEPTIONS = [73, 85, 96, 100, 111, 115, 116, 119, 126, 164, 221, 240, 246, 254]


def agreeing_values():
    """the gray values on which the PNM reader and the definition agree, recomputed"""
    v = np.arange(256, dtype=np.uint8)
    p = pnm_planes(np.stack([v, v, v], axis=-1))
    good = (p[0] == (v.astype(np.int16) - 128) * 16) & (p[1] == 0) & (p[2] == 0)
    return [int(k) for k in v[good]]


def onto_agreeing(a):
    """the 8-bit image `a' with every exception moved to the next value that agrees"""
    good = agreeing_values()
    table = np.array([min(g for g in good if g >= v) for v in range(256)], dtype=np.uint8)
    return table[a]


def moving(n, w, h, s):
    """n frames (y, cb, cr) of w x h whose content moves from frame to frame"""
    return [textured(w, h, s, 1234, shift=k) for k in range(n)]
