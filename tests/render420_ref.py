"""What the tests of the 4:2:0 renderer share (tests/test_render_420_api.py, tests/test_gpu_render_420.py, the generator
tests/golden/make_rendered_420.py): the fixture tests/golden/RENDERED_420.json, the numpy model -- the reference's 4:2:0
loops (lib/dither.c) write the bytes of its 4:4:4 renderer for the same Y plane with every chroma sample replicated over its
2 x 2 pixels, so the model is tests/render_ref.py on replicated planes --, the size rule, and hand-made planes from a closed
formula that meet the clip bounds and the chroma clamps in every plane and stay inside the reference's tables."""
import json
import os

import numpy as np

import render_ref

GOLDEN = render_ref.GOLDEN
RENDERERS = render_ref.RENDERERS
md5 = render_ref.md5
# the hand-made frames of the fixture: one every renderer takes, one with width % 4 == 2
HANDMADE_SIZES = ((36, 6), (34, 4))
# the renderers whose bytes at 36 x 6 the fixture holds: one of each depth
WITH_BYTES = ("rgb565", "rgb24", "xrgb8888")


def fixture():
    return json.load(open(os.path.join(GOLDEN, "RENDERED_420.json")))


def refused(bpp, doubled, width, height):
    """odd sides (the reference counts pixel pairs of row pairs); 24 bpp not doubled with a width that is no multiple of 4
    (the reference's rows fall out of step with its chroma planes)"""
    return bool((width | height) & 1) or (bpp == 24 and not doubled and bool(width & 3))


def refused_named(name, width, height):
    bpp, _, _, _, doubled = RENDERERS[name]
    return refused(bpp, doubled, width, height)


def surface_size(bpp, doubled, width, height):
    return render_ref.surface_size(bpp, doubled, width, height)


def replicated(y, cb, cr):
    """the 3 x H x W planes whose 4:4:4 rendering is the 4:2:0 rendering of y, cb, cr"""
    y = np.asarray(y)
    h, w = y.shape
    up = [np.repeat(np.repeat(np.asarray(c), 2, 0), 2, 1) for c in (cb, cr)]
    assert up[0].shape == (h, w) == up[1].shape, (y.shape, up[0].shape)
    return np.stack([y, up[0], up[1]]).astype(np.int16)


def render_named(y, cb, cr, name):
    """the surface as a uint8 array of shape (H', W', bpp // 8)"""
    return render_ref.render_named(replicated(y, cb, cr), name)


FORMULA = ("Y: N = w h values, i = 0 .. N - 1 in raster order, v_i = -157 + 315 i div (N - 1).  Cb, Cr: M = (w / 2) (h / 2) values, "
           "j = 0 .. M - 1, Cb v_j = -1152 + 2303 ((37 j + 5) mod M) div (M - 1), Cr v_j = -1152 + 2303 ((53 j + 11) mod M) div (M - 1); "
           "Cb v_0 = -1152, v_(M-1) = 1151, Cr v_0 = 1151, v_(M-1) = -1152.  Then the specials, one chroma sample each from j = 1 on: "
           "for s in -130, -129, -128, -127, 125, 126, 127, 128: Cb = Cr = 0 and the four Y values of the sample 0, -1, 1, s in raster "
           "order (the two clip bounds of R = G = B); then for the same eight s: Cb = s, Cr = 0 and the four Y values 0; then Cr = s, Cb = 0 "
           "likewise (the two chroma clamps).  value = 16 v + (7 index mod 16) with the index of the value in its own plane.")


def handmade(width, height):
    """the planes of FORMULA: int16 Y of h x w, Cb and Cr of h/2 x w/2"""
    w, h, cw, ch = width, height, width // 2, height // 2
    n, m = w * h, cw * ch
    assert m >= 1 + 3 * len(render_ref.SPECIALS) + 1
    i, j = np.arange(n, dtype=np.int64), np.arange(m, dtype=np.int64)
    y = (-157 + (315 * i) // (n - 1)).reshape(h, w)
    cb = -1152 + (2303 * ((37 * j + 5) % m)) // (m - 1)
    cr = -1152 + (2303 * ((53 * j + 11) % m)) // (m - 1)
    cb[0], cb[m - 1], cr[0], cr[m - 1] = -1152, 1151, 1151, -1152

    def block(at):
        r, c = divmod(at, cw)
        return y[2 * r:2 * r + 2, 2 * c:2 * c + 2]
    at = 1
    for plane in (None, cb, cr):
        for s in render_ref.SPECIALS:
            cb[at] = cr[at] = 0
            if plane is None:
                block(at)[:] = [[0, -1], [1, s]]
            else:
                block(at)[:] = 0
                plane[at] = s
            at += 1
    fy, fc = (7 * i) % 16, (7 * j) % 16
    return ((16 * y.reshape(-1) + fy).astype(np.int16).reshape(h, w), (16 * cb + fc).astype(np.int16).reshape(ch, cw),
            (16 * cr + fc).astype(np.int16).reshape(ch, cw))
