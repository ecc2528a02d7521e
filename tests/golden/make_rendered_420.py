#!/usr/bin/env python3
"""Frames decoded in 4:2:0 as the REAL reference's renderer puts them into an XImage -- what its viewer shows on a screen
(bin/dwfa.c:161 with lib/dither.c): tests/golden/RENDERED_420.json.  The reference library oracle/_ref/libfiasco_ref.so is
driven through ctypes as make_rendered.py and make_decoded_420.py drive it -- fiasco_d_options_new / _set_4_2_0_format /
_set_magnification / _set_smoothing, fiasco_decoder_new, fiasco_decoder_get_frame, fiasco_renderer_new / _render / _delete --
for the twelve renderers of tests/render_ref.py.

(a) decoded frames: cases of tests/golden/DECODED_420.json, coded again with cfiasco_ref as make_decoded_420.py codes them (the
    stream's md5 is asserted), decoded with set_4_2_0_format(1) at the magnifications the case lists and smoothing 0 and -1
    (the value of the stream header); image_t.format == 1 is asserted.  Per renderer the md5 of the XImage bytes, or "refused"
    where this project refuses the shape.  The degenerate case, whose chroma the reference leaves zero and the library
    refuses, is recorded as refused throughout.
(b) hand-made planes: an image_t with format = 1 around the planes of render420_ref.handmade(), 36 x 6 for every renderer and
    34 x 4 for the renderers that accept it.  Every index stays inside the reference's tables (asserted).  Per renderer the
    md5, and for one renderer of each depth the bytes themselves (zlib, base64) at 36 x 6.

Asserted on every render: the guard bytes behind the surface are intact; wherever the shape is accepted the reference's bytes
ARE the numpy model (render_ref.render_named on the planes with every chroma sample replicated over its 2 x 2 pixels);
at 24 bpp not doubled with width % 4 == 2 they are NOT, which pins the refusal as a fact about the reference; smoothing
changes the bytes.
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
import make_rendered  # noqa: E402
import render420_ref  # noqa: E402
import render_ref  # noqa: E402
import yuv420_ref  # noqa: E402
from conftest import GOLDEN, REF_SHARE  # noqa: E402

CASES = ["carry48_a", "c34", "c102x66", "carry74_a", "flat64"]
SMOOTHING = [0, -1]
REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_rendered_420"
GUARD = 64
c = ctypes
FiascoImage, Image = make_rendered.FiascoImage, make_rendered.Image


def load():
    L = make_rendered.load()
    L.fiasco_d_options_set_4_2_0_format.argtypes = [c.c_void_p, c.c_int]
    return L


def render(L, name, image, width, height):
    """the XImage bytes of the 4:2:0 `image' (width x height) under renderer `name', refused shapes included: the buffer has
    the size of the surface and guard bytes behind it, which must stay"""
    bpp, red, green, blue, doubled = render_ref.RENDERERS[name]
    sw, sh, row = render_ref.surface_size(bpp, doubled, width, height)
    r = L.fiasco_renderer_new(red, green, blue, bpp, 1 if doubled else 0)
    assert r, L.fiasco_get_error_message()
    buf = c.create_string_buffer(b"\xa5" * (sh * row + GUARD), sh * row + GUARD)
    assert L.fiasco_renderer_render(r, buf, image) == 1, L.fiasco_get_error_message()
    L.fiasco_renderer_delete(r)
    assert buf.raw[sh * row:] == b"\xa5" * GUARD, (name, "the reference wrote behind the surface")
    return buf.raw[:sh * row]


def checked(L, image, planes, width, height, what):
    """{renderer: bytes, or None where refused}, with the assertions about the model"""
    out, out_of_step = {}, 0
    for n, (bpp, _, _, _, doubled) in render_ref.RENDERERS.items():
        raw = render(L, n, image, width, height)
        model = render420_ref.render_named(planes[0], planes[1], planes[2], n).tobytes()
        if render420_ref.refused(bpp, doubled, width, height):
            assert bpp == 24 and not doubled and width % 4 == 2, (what, n)
            assert raw != model, (what, n, "the reference's bytes are the model's where the shape is refused")
            out_of_step += 1
            out[n] = None
        else:
            assert raw == model, (what, n, "tests/render420_ref.py disagrees with the reference")
            out[n] = raw
    return out, out_of_step


def decoded(L, env):
    cases = yuv420_ref.fixture_cases()
    out, out_of_step = {}, 0
    for name in CASES:
        ent = cases[name]
        data, ext = yuv420_ref.synth_input(ent["input"]) or make_golden.make_input(ent["input"])
        src, fco = os.path.join(TMP, name + "." + ext), os.path.join(TMP, name + ".fco")
        open(src, "wb").write(data)
        subprocess.check_call([os.path.join(REFDIR, "cfiasco_ref"), "--progress-meter", "0"] + ent["args"]
                              + ["--smooth", str(ent["smoothing"]), "-o", fco, src], env=env, stderr=subprocess.DEVNULL)
        assert hashlib.md5(open(fco, "rb").read()).hexdigest() == ent["stream_md5"], name
        recs = {}
        for m, rec420 in yuv420_ref.accepted(ent):
            per = {}
            for s in SMOOTHING:
                o = L.fiasco_d_options_new()
                assert L.fiasco_d_options_set_magnification(o, m) == 1
                assert L.fiasco_d_options_set_smoothing(o, ent["smoothing"] if s < 0 else s) == 1, L.fiasco_get_error_message()
                assert L.fiasco_d_options_set_4_2_0_format(o, 1) == 1
                d = L.fiasco_decoder_new(fco.encode(), o)
                assert d, L.fiasco_get_error_message()
                image = L.fiasco_decoder_get_frame(d)
                assert image, L.fiasco_get_error_message()
                im = c.cast(image.contents.private, c.POINTER(Image)).contents
                assert im.id == b"IFIASCO" and im.format == 1 and im.color, name
                w, h = im.width, im.height
                assert (w, h) == (rec420["width"], rec420["height"]), (name, m)
                planes = [np.ctypeslib.as_array(im.pixels[0], (h, w)).copy()] + [np.ctypeslib.as_array(im.pixels[k], (h >> 1, w >> 1)).copy() for k in (1, 2)]
                if s == 0:
                    assert [yuv420_ref.md5(p.tobytes()) for p in planes] == rec420["planes_md5"], (name, m)
                assert rec420["md5"][str(s)]["i420"] == yuv420_ref.md5(yuv420_ref.i420(*planes)), (name, m, s)
                per[s], n = checked(L, image, planes, w, h, (name, m, s))
                out_of_step += n
                L.fiasco_decoder_delete(d)
                L.fiasco_d_options_delete(o)
            if ent["degenerate"]:
                per = {s: {n: None for n in render_ref.RENDERERS} for s in SMOOTHING}
            else:
                for n in render_ref.RENDERERS:
                    assert per[0][n] is None or per[0][n] != per[-1][n], "%s: smoothing changes nothing at -m %d under %s" % (name, m, n)
            recs[str(m)] = {"width": w, "height": h,
                            "md5": {str(s): {n: ("refused" if v is None else hashlib.md5(v).hexdigest()) for n, v in per[s].items()} for s in SMOOTHING}}
        out[name] = {"stream_md5": ent["stream_md5"], "smoothing": ent["smoothing"], "degenerate": ent["degenerate"], "rendered": recs}
        print("%-10s %s" % (name, " ".join("%s:%dx%d" % (m, r["width"], r["height"]) for m, r in recs.items())))
    assert out_of_step >= 6, out_of_step
    return out


def handmade(L):
    out = {}
    for w, h in render420_ref.HANDMADE_SIZES:
        planes = [np.ascontiguousarray(p) for p in render420_ref.handmade(w, h)]
        make_rendered.check_defined(render420_ref.replicated(*planes))
        for p in planes:
            for s in render_ref.SPECIALS:
                assert ((p >> 4) == s).any(), (w, h, s)      # the clip bounds and the chroma clamps are met in every plane
        im = Image(id=b"IFIASCO", reference_count=1, width=w, height=h, color=1, format=1)
        for k in range(3):
            im.pixels[k] = planes[k].ctypes.data_as(c.POINTER(c.c_int16))
        fi = FiascoImage(private=c.cast(c.pointer(im), c.c_void_p))
        got, out_of_step = checked(L, c.pointer(fi), planes, w, h, ("handmade", w, h))
        assert out_of_step == (2 if w % 4 else 0), (w, h)
        recs = {}
        for n, raw in got.items():
            if raw is None:
                continue
            rec = {"md5": hashlib.md5(raw).hexdigest()}
            if (w, h) == render420_ref.HANDMADE_SIZES[0] and n in render420_ref.WITH_BYTES:
                rec["bytes_zlib_b64"] = base64.b64encode(zlib.compress(raw, 9)).decode()
            recs[n] = rec
        out["%dx%d" % (w, h)] = {"width": w, "height": h, "planes_md5": [hashlib.md5(p.tobytes()).hexdigest() for p in planes], "renderers": recs}
    assert len(out["36x6"]["renderers"]) == 12 and len(out["34x4"]["renderers"]) == 10
    return out


def main():
    os.makedirs(TMP, exist_ok=True)
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    os.environ["FIASCO_DATA"] = env["FIASCO_DATA"]
    L = load()
    doc = {"generator": "tests/golden/make_rendered_420.py",
           "renderers": {n: {"bpp": v[0], "red_mask": "%x" % v[1], "green_mask": "%x" % v[2], "blue_mask": "%x" % v[3], "double_resolution": v[4]}
                         for n, v in render_ref.RENDERERS.items()},
           "handmade": {"formula": render420_ref.FORMULA, "seed": "none: the formula is closed", "planes": handmade(L)},
           "decoded": decoded(L, env)}
    with open(os.path.join(HERE, "RENDERED_420.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("RENDERED_420.json: %d bytes" % os.path.getsize(os.path.join(HERE, "RENDERED_420.json")))


if __name__ == "__main__":
    main()
