"""What the tests of the renderer share (tests/test_render_api.py, tests/test_gpu_render.py, the generator
tests/golden/make_rendered.py): the twelve renderers of tests/golden/RENDERED.json, a numpy restatement of the reference's
renderer (lib/dither.c: fiasco_renderer_new and the display_* functions for 4:4:4 and gray) written from the reference and
independent of both C implementations, with the table ends as clamps, and the hand-made planes of the fixture.

  colour   yval = (Y >> 4) + 128; cr, cb = clamp(C >> 4, -128, 127); R = yval + T_rr[cr], G = yval + T_rg[cr] + T_bg[cb],
           B = yval + T_bb[cb]; T_x[v] = trunc(k v + 0.5) in double, k = 1.4022, -0.7145, -0.3456, 1.7710
  gray     R = G = B = (p >> 4) + 128
  16 / 32  pixel = ((c(R) >> (8 - n_r)) << s_r) | ((c(G) >> (8 - n_g)) << s_g) | (c(B) >> (8 - n_b)), little endian --
           blue is not shifted (lib/dither.c:205-208 shifts the table entry before it assigns it)
  24       c(R), c(G), c(B) in memory when red_mask > green_mask, else c(B), c(G), c(R)
  doubled  every pixel twice in a row, every row twice"""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (bpp, red mask, green mask, blue mask); each with and without double_resolution ("_x2")
BASE = {
    "rgb565": (16, 0xf800, 0x07e0, 0x001f),
    "rgb555": (16, 0x7c00, 0x03e0, 0x001f),
    "xrgb8888": (32, 0xff0000, 0x00ff00, 0x0000ff),
    "xbgr8888_blue_quirk": (32, 0x0000ff, 0x00ff00, 0xff0000),
    "rgb24": (24, 0xff0000, 0x00ff00, 0x0000ff),
    "bgr24": (24, 0x0000ff, 0x00ff00, 0xff0000),
}
RENDERERS = {}
for _n, _v in BASE.items():
    RENDERERS[_n] = _v + (False,)
    RENDERERS[_n + "_x2"] = _v + (True,)


def fixture():
    return json.load(open(os.path.join(GOLDEN, "RENDERED.json")))


def md5(data):
    return hashlib.md5(bytes(data)).hexdigest()


def refused(bpp, doubled, width, height, color):
    """the shapes where the reference's loops do not fill the surface"""
    if bpp == 24:
        return bool(width & 1) if doubled else bool(width * height & 3)
    return bpp == 16 and not doubled and not color and bool(width * height & 1)


def surface_size(bpp, doubled, width, height):
    k = 2 if doubled else 1
    return width * k, height * k, width * k * (bpp // 8)


def _mask(mask):
    below = 0
    while not (mask >> below) & 1:
        below += 1
    return bin(mask).count("1"), below


def rgb(planes):
    """int16 planes (H x W, or 3 x H x W for Y, Cb, Cr) -> R, G, B as int64 arrays, not yet clipped"""
    p = np.asarray(planes).astype(np.int64)
    if p.ndim == 2:
        y = (p >> 4) + 128
        return y, y, y
    y = (p[0] >> 4) + 128
    cb, cr = np.clip(p[1] >> 4, -128, 127).astype(np.float64), np.clip(p[2] >> 4, -128, 127).astype(np.float64)

    def t(k, v):
        return np.trunc(k * v + 0.5).astype(np.int64)
    return y + t(1.4022, cr), y + t(-0.7145, cr) + t(-0.3456, cb), y + t(1.7710, cb)


def render(planes, bpp, red, green, blue, doubled):
    """the surface as a uint8 array of shape (H', W', bpp // 8)"""
    r, g, b = (np.clip(v, 0, 255) for v in rgb(planes))
    if bpp == 24:
        out = np.stack([r, g, b] if red > green else [b, g, r], axis=-1).astype(np.uint8)
    else:
        (nr, sr), (ng, sg), (nb, _) = _mask(red), _mask(green), _mask(blue)
        word = ((r >> (8 - nr)) << sr) | ((g >> (8 - ng)) << sg) | (b >> (8 - nb))
        out = np.stack([(word >> (8 * k)) & 0xff for k in range(bpp // 8)], axis=-1).astype(np.uint8)
    if doubled:
        out = out.repeat(2, axis=0).repeat(2, axis=1)
    return np.ascontiguousarray(out)


def render_named(planes, name):
    return render(planes, *RENDERERS[name])


# ------------------------------------------------------------------ the hand-made planes of the fixture

FORMULA = ("N = w h values per plane, i = 0 .. N - 1, value = 16 v_i + (7 i mod 16).  gray: v_i = -384 + 767 i div (N - 1); "
           "colour: Y v_i = -157 + 315 i div (N - 1), Cb v_i = -1152 + 2303 ((37 i + 5) mod N) div (N - 1), "
           "Cr v_i = -1152 + 2303 ((53 i + 11) mod N) div (N - 1).  Then the specials from i = 2 on, every second value: "
           "v = -130, -129, -128, -127, 125, 126, 127, 128 in the gray / Y plane (the two clip bounds of R = G = B) with both "
           "chroma values 0, and after them the same eight values in Cb with Y = 0 and Cr = 0, then in Cr with Y = 0 and Cb = 0 "
           "(the two chroma clamps).  The first and the last value of every plane stay the ends of its sweep.")
SPECIALS = (-130, -129, -128, -127, 125, 126, 127, 128)


def handmade(width, height, color):
    """the planes of FORMULA: int16, H x W or 3 x H x W.  Gray sweeps -384 .. 383 (the clip table of 24 bpp less the 128 the
    reference adds to its pointer), Y of a colour frame -157 .. 158 (with the largest table entries R, G and B stay inside
    -256 .. 511), the chroma planes -1152 .. 1151 (the reference's chroma tables)"""
    n = width * height
    i = np.arange(n, dtype=np.int64)
    frac = (7 * i) % 16
    if not color:
        v = -384 + (767 * i) // (n - 1)
        for k, s in enumerate(SPECIALS):
            v[2 + 2 * k] = s
        return (16 * v + frac).astype(np.int16).reshape(height, width)
    y = -157 + (315 * i) // (n - 1)
    cb = -1152 + (2303 * ((37 * i + 5) % n)) // (n - 1)
    cr = -1152 + (2303 * ((53 * i + 11) % n)) // (n - 1)
    at = 2
    for plane in (y, cb, cr):
        for s in SPECIALS:
            y[at] = cb[at] = cr[at] = 0
            plane[at] = s
            at += 2
    cb[0], cb[n - 1], cr[0], cr[n - 1] = -1152, 1151, 1151, -1152
    return np.stack([16 * y + frac, 16 * cb + frac, 16 * cr + frac]).astype(np.int16).reshape(3, height, width)


def handmade_size(bpp, doubled, color):
    """33 x 3 where the renderer takes 99 pixels, else 34 x 2"""
    return (34, 2) if refused(bpp, doubled, 33, 3, color) else (33, 3)
