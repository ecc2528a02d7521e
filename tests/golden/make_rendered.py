#!/usr/bin/env python3
"""Frames as the REAL reference's renderer puts them into an XImage: tests/golden/RENDERED.json.  The reference library
oracle/_ref/libfiasco_ref.so is driven through ctypes -- fiasco_d_options_new / _set_smoothing / _set_magnification,
fiasco_decoder_new, fiasco_decoder_get_frame, fiasco_renderer_new / _render / _delete, all plain exported functions --
for the twelve renderers of tests/render_ref.py (six formats, each with and without double_resolution).

(a) decoded frames: cases of tests/golden/DECODED_SHOWN.json, coded again with cfiasco_ref as make_decoded_shown.py codes
    them (the stream's md5 is asserted), decoded by the library at magnifications -1, 0, 1 and smoothing 0 and -1 (the value
    of the stream header) and rendered: per renderer the md5 of the XImage bytes and the surface size, or "refused" where
    this project refuses the shape because the reference's loops would leave the end of the surface unwritten.
(b) hand-made planes: a fiasco_image_t built around planes of render_ref.handmade() -- the layouts of fiasco_image_t
    (fiasco.h:101-108) and image_t (lib/image.h:26-38) are written down below as ctypes structures, with the id string
    cast_image checks --, 33 x 3 where the renderer takes 99 pixels and 34 x 2 where it does not, gray and colour.  Every
    index stays inside the reference's tables (asserted), so the recorded bytes are defined.  Per renderer the md5, and for
    33 x 3 the bytes themselves (zlib, base64) so that a mismatch can be read.
Build container only (oracle/_ref from oracle/ref_build.sh)."""
import base64
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
import render_ref  # noqa: E402
import shown_ref  # noqa: E402
from conftest import GOLDEN, REF_SHARE  # noqa: E402

CASES = ["g100x70", "g130x66", "carry74_a"]
MAGNIFY = [-1, 0, 1]
SMOOTHING = [0, -1]
REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_rendered"
GUARD = 64
c = ctypes


class FiascoImage(c.Structure):
    """fiasco_image_t (fiasco.h:101-108): four method pointers and the private pointer"""
    _fields_ = [("delete", c.c_void_p), ("get_width", c.c_void_p), ("get_height", c.c_void_p), ("is_color", c.c_void_p),
                ("private", c.c_void_p)]


class Image(c.Structure):
    """image_t (lib/image.h:26-38); color is the enum bool_t, format the enum format_e (0: 4:4:4)"""
    _fields_ = [("id", c.c_char * 8), ("reference_count", c.c_uint), ("width", c.c_uint), ("height", c.c_uint), ("color", c.c_int),
                ("format", c.c_int), ("pixels", c.POINTER(c.c_int16) * 3)]


def load():
    L = c.CDLL(os.path.join(REFDIR, "libfiasco_ref.so"))
    L.fiasco_get_error_message.restype = c.c_char_p
    L.fiasco_d_options_new.restype = c.c_void_p
    L.fiasco_d_options_set_smoothing.argtypes = [c.c_void_p, c.c_int]
    L.fiasco_d_options_set_magnification.argtypes = [c.c_void_p, c.c_int]
    L.fiasco_d_options_delete.argtypes = [c.c_void_p]
    L.fiasco_decoder_new.restype = c.c_void_p
    L.fiasco_decoder_new.argtypes = [c.c_char_p, c.c_void_p]
    L.fiasco_decoder_get_frame.restype = c.POINTER(FiascoImage)
    L.fiasco_decoder_get_frame.argtypes = [c.c_void_p]
    L.fiasco_decoder_delete.argtypes = [c.c_void_p]
    L.fiasco_renderer_new.restype = c.c_void_p
    L.fiasco_renderer_new.argtypes = [c.c_ulong, c.c_ulong, c.c_ulong, c.c_uint, c.c_int]
    L.fiasco_renderer_render.argtypes = [c.c_void_p, c.c_char_p, c.POINTER(FiascoImage)]
    L.fiasco_renderer_delete.argtypes = [c.c_void_p]
    return L


def render(L, name, image, width, height, color):
    """the XImage bytes of `image' (width x height) under renderer `name', or None where the shape is refused"""
    bpp, red, green, blue, doubled = render_ref.RENDERERS[name]
    if render_ref.refused(bpp, doubled, width, height, color):
        return None
    sw, sh, row = render_ref.surface_size(bpp, doubled, width, height)
    r = L.fiasco_renderer_new(red, green, blue, bpp, 1 if doubled else 0)
    assert r, L.fiasco_get_error_message()
    buf = c.create_string_buffer(b"\xa5" * (sh * row + GUARD), sh * row + GUARD)
    assert L.fiasco_renderer_render(r, buf, image) == 1, L.fiasco_get_error_message()
    L.fiasco_renderer_delete(r)
    assert buf.raw[sh * row:] == b"\xa5" * GUARD, (name, "the reference wrote behind the surface")
    return buf.raw[:sh * row]


def check_defined(planes):
    """every index the reference forms on these planes lies inside its tables (lib/dither.c:139-242, lib/misc.c: the clip
    table of 24 bpp spans -256 .. 511)"""
    p = np.asarray(planes).astype(np.int64) >> 4
    if p.ndim == 2:
        assert -384 <= p.min() and p.max() <= 383             # shift_clipping = gray_clip + 128; y_table spans -1152 .. 1151
        return
    assert -1152 <= p[1:].min() and p[1:].max() <= 1151       # the chroma tables
    for v in render_ref.rgb(planes):
        assert -256 <= v.min() and v.max() <= 511             # gray_clip; r_table etc. span -1024 .. 1279


def decoded(L, env):
    shown = shown_ref.fixture_cases()
    out = {}
    for name in CASES:
        ent = shown[name]
        data, ext = shown_ref.synth_input(ent["input"]) or make_golden.make_input(ent["input"])
        src, fco = os.path.join(TMP, name + "." + ext), os.path.join(TMP, name + ".fco")
        open(src, "wb").write(data)
        subprocess.check_call([os.path.join(REFDIR, "cfiasco_ref"), "--progress-meter", "0"] + ent["args"]
                              + ["--smooth", str(ent["smoothing"]), "-o", fco, src], env=env, stderr=subprocess.DEVNULL)
        assert hashlib.md5(open(fco, "rb").read()).hexdigest() == ent["stream_md5"], name
        recs = {}
        for m in MAGNIFY:
            assert "md5" in ent["shown"][str(m)], (name, m)
            per = {}
            for s in SMOOTHING:
                o = L.fiasco_d_options_new()
                assert L.fiasco_d_options_set_magnification(o, m) == 1
                assert L.fiasco_d_options_set_smoothing(o, ent["smoothing"] if s < 0 else s) == 1, L.fiasco_get_error_message()
                d = L.fiasco_decoder_new(fco.encode(), o)
                assert d, L.fiasco_get_error_message()
                image = L.fiasco_decoder_get_frame(d)
                assert image, L.fiasco_get_error_message()
                im = c.cast(image.contents.private, c.POINTER(Image)).contents
                assert im.id == b"IFIASCO" and im.format == 0 and bool(im.color) == ent["color"], name
                w, h = im.width, im.height
                assert (w, h) == (ent["shown"][str(m)]["width"], ent["shown"][str(m)]["height"]), (name, m)
                per[s] = {n: render(L, n, image, w, h, ent["color"]) for n in render_ref.RENDERERS}
                L.fiasco_decoder_delete(d)
                L.fiasco_d_options_delete(o)
            for s in SMOOTHING:
                got = {n: v for n, v in per[s].items() if v is not None}
                assert len(got) >= 10, (name, m, sorted(got))
                names = sorted(got)
                for a in names:
                    for b in names:
                        same_bytes_by_design = not ent["color"] and {a.replace("_x2", ""), b.replace("_x2", "")} == {"rgb24", "bgr24"} \
                            and a.endswith("_x2") == b.endswith("_x2")      # R = G = B: the two byte orders coincide
                        assert a >= b or same_bytes_by_design or got[a] != got[b], (name, m, s, a, b)
            for n in render_ref.RENDERERS:
                assert per[0][n] is None or per[0][n] != per[-1][n], "%s: smoothing changes nothing at -m %d under %s" % (name, m, n)
            recs[str(m)] = {"width": w, "height": h,
                            "md5": {str(s): {n: ("refused" if v is None else hashlib.md5(v).hexdigest()) for n, v in per[s].items()}
                                    for s in SMOOTHING}}
        out[name] = {"stream_md5": ent["stream_md5"], "color": ent["color"], "smoothing": ent["smoothing"], "rendered": recs}
        print("%-10s %s" % (name, " ".join("%s:%dx%d" % (m, r["width"], r["height"]) for m, r in recs.items())))
    return out


def handmade(L):
    out = {}
    for color in (False, True):
        recs = {}
        for n, (bpp, red, green, blue, doubled) in render_ref.RENDERERS.items():
            w, h = render_ref.handmade_size(bpp, doubled, color)
            planes = render_ref.handmade(w, h, color)
            check_defined(planes)
            flat = np.ascontiguousarray(planes).reshape(3 if color else 1, -1)
            v = flat >> 4
            for s in render_ref.SPECIALS:
                assert all((v[k] == s).any() for k in range(len(v))), (n, s)      # the clip bounds and the chroma clamps are met
            im = Image(id=b"IFIASCO", reference_count=1, width=w, height=h, color=1 if color else 0, format=0)
            for k in range(len(flat)):
                im.pixels[k] = flat[k].ctypes.data_as(c.POINTER(c.c_int16))
            fi = FiascoImage(private=c.cast(c.pointer(im), c.c_void_p))
            raw = render(L, n, c.pointer(fi), w, h, color)
            assert raw is not None, n
            assert raw == render_ref.render_named(planes, n).tobytes(), (n, "tests/render_ref.py disagrees with the reference")
            rec = {"width": w, "height": h, "planes_md5": hashlib.md5(planes.tobytes()).hexdigest(), "md5": hashlib.md5(raw).hexdigest()}
            if (w, h) == (33, 3):
                rec["bytes_zlib_b64"] = base64.b64encode(zlib.compress(raw, 9)).decode()
            recs[n] = rec
        assert any(r["width"] == 33 for r in recs.values()) and any(r["width"] == 34 for r in recs.values())
        out["color" if color else "gray"] = recs
    return out


def main():
    os.makedirs(TMP, exist_ok=True)
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    os.environ["FIASCO_DATA"] = env["FIASCO_DATA"]
    L = load()
    doc = {"generator": "tests/golden/make_rendered.py",
           "renderers": {n: {"bpp": v[0], "red_mask": "%x" % v[1], "green_mask": "%x" % v[2], "blue_mask": "%x" % v[3], "double_resolution": v[4]}
                         for n, v in render_ref.RENDERERS.items()},
           "handmade": {"formula": render_ref.FORMULA, "seed": "none: the formula is closed", "planes": handmade(L)},
           "decoded": decoded(L, env)}
    with open(os.path.join(HERE, "RENDERED.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("RENDERED.json: %d bytes" % os.path.getsize(os.path.join(HERE, "RENDERED.json")))


if __name__ == "__main__":
    main()
