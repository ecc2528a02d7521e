#!/usr/bin/env python3
"""What the REAL reference's decoder interface (fiasco.h: fiasco_d_options_*, fiasco_decoder_*, fiasco_image_*,
fiasco_renderer_*) says and writes where the older fixtures do not record it: tests/golden/DECODER_API.json.  Build
container only (oracle/_ref from oracle/ref_build.sh).

The reference library oracle/_ref/libfiasco_ref.so is driven through ctypes as tests/golden/make_decoded_streams.py drives
it.  One child process per case: the reference ends the process on some inputs, and such a case is left out BY NAME with
how it ended ("left_out").  The fixture holds md5s, sizes and messages only:
  messages   the sentences of fiasco_d_options_set_smoothing out of range, of an options object whose private pointer is
             NULL or of another type, and of both magnification refusals of fiasco_decoder_new
  info       get_width / get_height / get_length / get_rate / is_color / title / comment per stream of stream_cases.NAMES at
             magnification -1, 0, 1 (or the refusal)
  written    md5 of the whole PNM file fiasco_decoder_write_frame writes per display frame: three videos, magnification
             -1, 0, 1, smoothing 0 and -1 (not set)
  rendered   md5 of the XImage fiasco_renderer_render writes per frame: st_color_ipbbp_64 in both formats and seq4_gray_ibbp,
             under rgb565, xrgb8888 and rgb565_x2 of tests/render_ref.py
  gray_420   what a gray stream gives with the 4:2:0 option set: size and planes md5 per frame
  images     g100x70.pgm and carry48_c.ppm through fiasco_image_new: get_width, get_height (the reference returns the
             WIDTH, lib/image.c:127-135), the height of image_t, colour, planes md5, and the XImage md5 under two renderers"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
import conftest  # noqa: E402
import render_ref  # noqa: E402
import stream_cases as sc  # noqa: E402
from make_decoded_420 import FiascoImage, Image, load  # noqa: E402

c = ctypes
ENV = dict(os.environ, FIASCO_DATA=conftest.GOLDEN + ":" + conftest.REF_SHARE, FIASCO_IMAGES=conftest.GOLDEN)
FIXTURE = os.path.join(HERE, "DECODER_API.json")
WRITTEN = ["seq4_gray_ibbp", sc.IPBBP, sc.IBBP_B0]
RENDERED = [(sc.IPBBP, "444"), (sc.IPBBP, "420"), ("seq4_gray_ibbp", "444")]
RENDERERS = ["rgb565", "xrgb8888", "rgb565_x2"]
IMAGES = ["g100x70.pgm", "carry48_c.ppm"]
IMAGE_RENDERERS = ["rgb565", "xrgb8888"]


class DOptions(c.Structure):
    """fiasco_d_options_t (fiasco.h:179-189)"""
    _fields_ = [("delete", c.c_void_p), ("set_smoothing", c.c_void_p), ("set_magnification", c.c_void_p), ("set_4_2_0_format", c.c_void_p),
                ("private", c.c_void_p)]


def lib():
    L = load()
    for name in ("get_length", "get_rate", "get_width", "get_height"):
        f = getattr(L, "fiasco_decoder_" + name)
        f.argtypes, f.restype = [c.c_void_p], c.c_uint
    L.fiasco_decoder_is_color.argtypes = [c.c_void_p]
    for name in ("get_title", "get_comment"):
        f = getattr(L, "fiasco_decoder_" + name)
        f.argtypes, f.restype = [c.c_void_p], c.c_char_p
    L.fiasco_decoder_write_frame.argtypes = [c.c_void_p, c.c_char_p]
    L.fiasco_image_new.argtypes, L.fiasco_image_new.restype = [c.c_char_p], c.POINTER(FiascoImage)
    for name in ("get_width", "get_height"):
        f = getattr(L, "fiasco_image_" + name)
        f.argtypes, f.restype = [c.POINTER(FiascoImage)], c.c_uint
    L.fiasco_image_is_color.argtypes = [c.POINTER(FiascoImage)]
    L.fiasco_renderer_new.argtypes, L.fiasco_renderer_new.restype = [c.c_ulong, c.c_ulong, c.c_ulong, c.c_uint, c.c_int], c.c_void_p
    L.fiasco_renderer_render.argtypes = [c.c_void_p, c.c_char_p, c.POINTER(FiascoImage)]
    return L


def message(L):
    return L.fiasco_get_error_message().decode("latin-1")


def options(L, magnify, smoothing, subsampled):
    o = L.fiasco_d_options_new()
    assert L.fiasco_d_options_set_magnification(o, magnify) == 1
    if smoothing >= 0:                      # -1: not set, the header's value
        assert L.fiasco_d_options_set_smoothing(o, smoothing) == 1
    assert L.fiasco_d_options_set_4_2_0_format(o, 1 if subsampled else 0) == 1
    return o


def planes_of(image, subsampled):
    im = c.cast(image.contents.private, c.POINTER(Image)).contents
    w, h = im.width, im.height
    cw, ch = (w >> 1, h >> 1) if subsampled and im.color else (w, h)
    planes = [np.ctypeslib.as_array(im.pixels[0], (h, w)).copy()]
    if im.color:
        planes += [np.ctypeslib.as_array(im.pixels[b], (ch, cw)).copy() for b in (1, 2)]
    return im, planes


def planes_md5(planes):
    return hashlib.md5(b"".join(np.ascontiguousarray(p, "<i2").tobytes() for p in planes)).hexdigest()


def ximage(L, image, im, subsampled, renderer):
    """md5 of the XImage, or None where the project refuses the shape (the reference leaves part of the surface unwritten)"""
    bpp, red, green, blue, doubled = render_ref.RENDERERS[renderer]
    if render_ref.refused(bpp, doubled, im.width, im.height, bool(im.color)) or (subsampled and ((im.width | im.height) & 1)):
        return None
    r = L.fiasco_renderer_new(red, green, blue, bpp, 1 if doubled else 0)
    assert r, message(L)
    sw, sh, row = render_ref.surface_size(bpp, doubled, im.width, im.height)
    buf = c.create_string_buffer(sh * row)
    assert L.fiasco_renderer_render(r, buf, image) == 1, message(L)
    return hashlib.md5(buf.raw).hexdigest()


def child(what, args):
    L = lib()
    if what == "messages":
        out = {}
        o = L.fiasco_d_options_new()
        for v in (-2, 101):
            assert L.fiasco_d_options_set_smoothing(o, v) == 0
            out["smoothing_%d" % v] = message(L)
        null = DOptions()
        assert L.fiasco_d_options_set_smoothing(c.byref(null), 10) == 0
        out["options_null"] = message(L)
        other = c.create_string_buffer(b"XXXXXXXX", 64)
        wrong = DOptions(private=c.cast(other, c.c_void_p))
        assert L.fiasco_d_options_set_magnification(c.byref(wrong), 0) == 0
        out["options_wrong_type"] = message(L)
        for key, name, m in (("too_small", "g32x32_q20", -1), ("too_small_2", "g100x70_q20", -3), ("too_large", "g256_rpf", 4), ("too_large_2", "g32x32_q20", 9)):
            assert not L.fiasco_decoder_new(sc.stream_path(name).encode(), options(L, m, 0, False))
            out[key] = {"stream": name, "magnify": m, "message": message(L)}
        print(json.dumps(out))
    elif what == "info":
        name, m = args[0], int(args[1])
        d = L.fiasco_decoder_new(sc.stream_path(name).encode(), options(L, m, 0, False))
        if not d:
            print(json.dumps({"refused": message(L)}))
            return
        print(json.dumps({"width": L.fiasco_decoder_get_width(d), "height": L.fiasco_decoder_get_height(d), "length": L.fiasco_decoder_get_length(d),
                          "rate": L.fiasco_decoder_get_rate(d), "color": int(L.fiasco_decoder_is_color(d)),
                          "title": (L.fiasco_decoder_get_title(d) or b"").decode("latin-1"), "comment": (L.fiasco_decoder_get_comment(d) or b"").decode("latin-1")}))
    elif what == "written":
        name, m, s, tmp = args[0], int(args[1]), int(args[2]), args[3]
        d = L.fiasco_decoder_new(sc.stream_path(name).encode(), options(L, m, s, False))
        if not d:
            print(json.dumps({"refused": message(L)}))
            return
        files = []
        for k in range(L.fiasco_decoder_get_length(d)):
            path = os.path.join(tmp, "f%d.pnm" % k)
            assert L.fiasco_decoder_write_frame(d, path.encode()) == 1, message(L)
            data = open(path, "rb").read()
            files.append({"md5": hashlib.md5(data).hexdigest(), "bytes": len(data)})
        print(json.dumps({"files": files}))
    elif what == "rendered":
        name, fmt, renderer = args
        d = L.fiasco_decoder_new(sc.stream_path(name).encode(), options(L, 0, -1, fmt == "420"))
        assert d, message(L)
        frames = []
        for k in range(L.fiasco_decoder_get_length(d)):
            image = L.fiasco_decoder_get_frame(d)
            assert image, message(L)
            im, _ = planes_of(image, fmt == "420")
            frames.append(ximage(L, image, im, fmt == "420", renderer))
        print(json.dumps({"frames": frames}))
    elif what == "gray_420":
        d = L.fiasco_decoder_new(sc.stream_path(args[0]).encode(), options(L, 0, -1, True))
        assert d, message(L)
        frames = []
        for k in range(L.fiasco_decoder_get_length(d)):
            image = L.fiasco_decoder_get_frame(d)
            assert image, message(L)
            im, planes = planes_of(image, True)
            frames.append({"width": im.width, "height": im.height, "color": int(im.color), "format": im.format, "planes_md5": planes_md5(planes)})
        print(json.dumps({"frames": frames}))
    elif what == "image":
        image = L.fiasco_image_new(os.path.join(conftest.GOLDEN, args[0]).encode())
        assert image, message(L)
        im, planes = planes_of(image, False)
        print(json.dumps({"get_width": L.fiasco_image_get_width(image), "get_height": L.fiasco_image_get_height(image), "height": im.height,
                          "color": int(L.fiasco_image_is_color(image)), "planes_md5": planes_md5(planes),
                          "ximage_md5": {r: ximage(L, image, im, False, r) for r in IMAGE_RENDERERS}}))


def one(left_out, what, *args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", what] + [str(a) for a in args], env=ENV, capture_output=True)
    if r.returncode != 0:
        how = "signal %d" % -r.returncode if r.returncode < 0 else "exit %d: %s" % (r.returncode, r.stderr.decode("latin-1").strip().split("\n")[-1][:120])
        left_out[" ".join([what] + [str(a) for a in args[:3]])] = how
        return None
    return json.loads(r.stdout.decode().strip().split("\n")[-1])


def main():
    tmp = tempfile.mkdtemp(prefix="fiasco_decoder_api_")
    left_out = {}
    out = {"generator": "tests/golden/make_decoder_api.py", "reference": "oracle/_ref/libfiasco_ref.so (oracle/ref_build.sh), driven through ctypes",
           "messages": one(left_out, "messages"), "info": {}, "written": {}, "rendered": {}, "gray_420": {}, "images": {}}
    for name in sc.NAMES:
        out["info"][name] = {str(m): one(left_out, "info", name, m) for m in sc.MAGNIFY}
    for name in WRITTEN:
        out["written"][name] = {"%d:%d" % (m, s): one(left_out, "written", name, m, s, tmp) for m in sc.MAGNIFY for s in (0, -1)}
    for name, fmt in RENDERED:
        out["rendered"]["%s:%s" % (name, fmt)] = {r: one(left_out, "rendered", name, fmt, r) for r in RENDERERS}
    out["gray_420"]["seq4_gray_ibbp"] = one(left_out, "gray_420", "seq4_gray_ibbp")
    for name in IMAGES:
        out["images"][name] = one(left_out, "image", name)
    out["left_out"] = left_out
    json.dump(out, open(FIXTURE, "w"), indent=1, sort_keys=True)
    print("DECODER_API.json: %d bytes; left out: %s" % (os.path.getsize(FIXTURE), left_out))


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--one":
        child(sys.argv[2], sys.argv[3:])
    else:
        main()
