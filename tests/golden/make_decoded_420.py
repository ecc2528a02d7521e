#!/usr/bin/env python3
"""Frames as the REAL reference's decoder makes them in 4:2:0: tests/golden/DECODED_420.json.  For the colour stills below
`cfiasco_ref <args> --smooth 70' codes the input, and the reference library oracle/_ref/libfiasco_ref.so is driven through
ctypes -- fiasco_d_options_new / _set_4_2_0_format / _set_magnification / _set_smoothing, fiasco_decoder_new,
fiasco_decoder_get_frame -- and the planes are read out of image_t (lib/image.h:26-38; Cb and Cr hold (W >> 1) x (H >> 1)
values, alloc_image lib/image.c:209-211).  Per case and magnification M in -1, 0, 1 where the size rule allows it the fixture
records the size, the md5 of the unsmoothed int16 planes and, for smoothing 0, -1 (the header's value) and 35, the md5 of the
Y bytes and of the I420 and NV12 buffers computed in numpy from the reference's planes (tests/yuv420_ref.py: every plane
clip255((p >> 4) + 128)); for the smallest case the I420 bytes themselves.

Everything include/libfiasco_amd_420.h says about the reference is asserted here on every decode:
  the size is fiasco_amd_magnified_size()'s and even;
  the unsmoothed Y plane is the 4:4:4 Y plane at the same M;
  where the size rule gives M - 1 half the size, Cb and Cr are the 4:4:4 chroma planes at M - 1; where the halves were rounded up to even
  they are a crop of that thumbnail (102 x 66: 51 x 33 of 52 x 34; 74 x 138: 37 x 69 of 38 x 70); 48 x 70 and 34 x 34 decode at M = 0 although M - 1 is refused ("Minimum value is 0."), 74 x 138 likewise at -1;
  the flat image has all-zero chroma in 4:2:0 at every M while its 4:4:4 decode has colour, and the library's own plan
  (fiasco_amd_batch_smoothing_borders_420 on the CPU oracle, host code) refuses exactly that case and names the levels;
  every other case has chroma that is not all zero;
  the smoothed Y plane differs from the smoothed 4:4:4 Y plane, and it IS the unsmoothed Y plane smoothed sequentially
  (tests/smooth_ref.py) along the library's 4:2:0 border list: Y passes at shift M, Cb passes at shift M - 1.
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
import fiasco_amd  # noqa: E402
import make_golden  # noqa: E402
import smooth_ref  # noqa: E402
import yuv420_ref  # noqa: E402
from conftest import GOLDEN, ORACLE_LIB, REF_SHARE, options_from_args  # noqa: E402

# (name, input, MANIFEST case whose arguments are used, magnifications)
# carry48_a: 48 x 70, chroma 24 x 35, the thumbnail at -1 refused; carry74_a: half width 37; c102x66: chroma 51 x 33, a crop of
# the 52 x 34 thumbnail; c256sq, c320x200: all three magnifications; c34: the smallest size, -1 refused; flat64: the
# degenerate case, whose chroma the reference leaves zero and the library refuses
CASES = [
    ("carry48_a", "carry48_a", "seq3_color_carry48", [0, 1]),
    ("carry74_a", "carry74_a", "seq3_color_carry74", [-1, 0, 1]),
    ("c102x66", "colork:102:66:0", "c256_q20", [-1, 0, 1]),
    ("c256sq", "colork:256:256:0", "c256_q20", [-1, 0, 1]),
    ("c320x200", "colork:320:200:0", "c256_q20", [-1, 0, 1]),
    ("c34", "colork:34:34:0", "c256_q20", [0, 1]),
    ("flat64", "flat:64:64:200:80:40", "c256_q20", [-1, 0, 1]),
]
DEGENERATE = {"flat64"}
REFUSED_BELOW = {"carry48_a": 0, "c34": 0}         # cases that must decode at M = 0 although the size rule refuses M - 1
HEADER = 70
REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_420"
c = ctypes


class FiascoImage(c.Structure):
    """fiasco_image_t (fiasco.h:101-108): four method pointers and the private pointer"""
    _fields_ = [("delete", c.c_void_p), ("get_width", c.c_void_p), ("get_height", c.c_void_p), ("is_color", c.c_void_p),
                ("private", c.c_void_p)]


class Image(c.Structure):
    """image_t (lib/image.h:26-38); color is the enum bool_t, format the enum format_e (0: 4:4:4, 1: 4:2:0)"""
    _fields_ = [("id", c.c_char * 8), ("reference_count", c.c_uint), ("width", c.c_uint), ("height", c.c_uint), ("color", c.c_int),
                ("format", c.c_int), ("pixels", c.POINTER(c.c_int16) * 3)]


def load():
    L = c.CDLL(os.path.join(REFDIR, "libfiasco_ref.so"))
    L.fiasco_get_error_message.restype = c.c_char_p
    L.fiasco_d_options_new.restype = c.c_void_p
    L.fiasco_d_options_set_smoothing.argtypes = [c.c_void_p, c.c_int]
    L.fiasco_d_options_set_magnification.argtypes = [c.c_void_p, c.c_int]
    L.fiasco_d_options_set_4_2_0_format.argtypes = [c.c_void_p, c.c_int]
    L.fiasco_d_options_delete.argtypes = [c.c_void_p]
    L.fiasco_decoder_new.restype = c.c_void_p
    L.fiasco_decoder_new.argtypes = [c.c_char_p, c.c_void_p]
    L.fiasco_decoder_get_frame.restype = c.POINTER(FiascoImage)
    L.fiasco_decoder_get_frame.argtypes = [c.c_void_p]
    L.fiasco_decoder_delete.argtypes = [c.c_void_p]
    return L


def decode(L, fco, magnify, smoothing, subsampled):
    """(Y, Cb, Cr) as int16 arrays, or the message the reference refuses the stream at `magnify' with"""
    o = L.fiasco_d_options_new()
    assert L.fiasco_d_options_set_magnification(o, magnify) == 1
    assert L.fiasco_d_options_set_smoothing(o, smoothing) == 1, L.fiasco_get_error_message()
    assert L.fiasco_d_options_set_4_2_0_format(o, 1 if subsampled else 0) == 1
    d = L.fiasco_decoder_new(fco.encode(), o)
    if not d:
        L.fiasco_d_options_delete(o)
        return L.fiasco_get_error_message().decode("latin-1")
    image = L.fiasco_decoder_get_frame(d)
    assert image, L.fiasco_get_error_message()
    im = c.cast(image.contents.private, c.POINTER(Image)).contents
    assert im.id == b"IFIASCO" and im.color and im.format == (1 if subsampled else 0)
    w, h = im.width, im.height
    cw, ch = (w >> 1, h >> 1) if subsampled else (w, h)
    planes = [np.ctypeslib.as_array(im.pixels[0], (h, w)).copy()] + [np.ctypeslib.as_array(im.pixels[k], (ch, cw)).copy() for k in (1, 2)]
    L.fiasco_decoder_delete(d)
    L.fiasco_d_options_delete(o)
    return planes


def main():
    os.makedirs(TMP, exist_ok=True)
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    cases = {k["name"]: k for k in man["cases"]}
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    os.environ["FIASCO_DATA"] = env["FIASCO_DATA"]
    L = load()
    ora = fiasco_amd.Library(ORACLE_LIB)
    ora.set_verbosity(0)
    out, cropped = {}, set()
    smallest = min(CASES, key=lambda k: 0 if k[0] == "c34" else 1)[0]
    for name, inp, of, mags in CASES:
        args = cases[of]["args"]
        data, ext = yuv420_ref.synth_input(inp) or make_golden.make_input(inp)
        assert ext == "ppm", name
        src, fco = os.path.join(TMP, name + ".ppm"), os.path.join(TMP, name + ".fco")
        open(src, "wb").write(data)
        subprocess.check_call([os.path.join(REFDIR, "cfiasco_ref"), "--progress-meter", "0"] + args + ["--smooth", str(HEADER), "-o", fco, src],
                              env=env, stderr=subprocess.DEVNULL)
        stream = open(fco, "rb").read()
        cw, ch, _ = fiasco_amd._pnm_geometry(data)
        # the library's own view of the same automaton: host code, on the CPU oracle
        q, o = options_from_args(ora, args)
        o.set_smoothing(HEADER)
        b = fiasco_amd.Batch(ora, [data], q, o)
        assert b.encode()[0] == stream, name + ": the oracle's stream is not the reference's"
        recs = {}
        for m in mags:
            w, h = fiasco_amd.magnified_size(ora, cw, ch, m)
            full = decode(L, fco, m, 0, False)
            sub = decode(L, fco, m, 0, True)
            assert sub[0].shape == (h, w) == full[0].shape and w % 2 == 0 and h % 2 == 0, (name, m)
            assert np.array_equal(sub[0], full[0]), (name, m, "the unsmoothed Y plane is not the 4:4:4 one")
            below = decode(L, fco, m - 1, 0, False)
            if isinstance(below, str):          # 4:2:0 decodes where the thumbnail one step below is refused
                assert "Minimum value is %d." % m in below, (name, m, below)
            elif below[0].shape == (h // 2, w // 2):
                assert np.array_equal(sub[1], below[1]) and np.array_equal(sub[2], below[2]) or name in DEGENERATE, (name, m)
            else:                               # the halves were rounded up to even: the chroma planes are a crop
                assert below[0].shape == (h // 2 + (h // 2 & 1), w // 2 + (w // 2 & 1)), (name, m, below[0].shape)
                cropped.add(name)
                assert np.array_equal(sub[1], below[1][:h // 2, :w // 2]) and np.array_equal(sub[2], below[2][:h // 2, :w // 2]), (name, m)
            if name in DEGENERATE:
                assert not sub[1].any() and not sub[2].any() and full[1].any() and full[2].any(), (name, m)
                try:
                    b.smoothing_borders_420(0, magnify=m)
                    raise AssertionError((name, m, "the library accepts the degenerate case"))
                except fiasco_amd.FiascoError as e:
                    assert "max_level" in str(e) and "chroma root has level" in str(e), str(e)
            else:
                assert sub[1].any() and sub[2].any(), (name, m)
                borders = b.smoothing_borders_420(0, magnify=m)
            rec = {"width": w, "height": h, "planes_md5": [yuv420_ref.md5(p.tobytes()) for p in sub],
                   "chroma_nonzero": int(np.count_nonzero(sub[1]) + np.count_nonzero(sub[2])), "below_refused": isinstance(below, str), "md5": {}}
            for s in yuv420_ref.SMOOTHING:
                n = HEADER if s < 0 else s
                got = decode(L, fco, m, n, True)
                assert np.array_equal(got[1], sub[1]) and np.array_equal(got[2], sub[2]), (name, m, s)
                if s and name not in DEGENERATE:           # (the flat image may have no border at all)
                    other = decode(L, fco, m, n, False)
                    assert not np.array_equal(got[0], other[0]), (name, m, s, "the smoothed Y plane is the 4:4:4 one")
                    assert np.array_equal(smooth_ref.smooth(sub[0], borders, n), got[0]), (name, m, s, "the 4:2:0 border list")
                elif not s:
                    assert np.array_equal(got[0], sub[0]), (name, m)
                rec["md5"][str(s)] = {"y": yuv420_ref.md5(yuv420_ref.to_bytes(got[0]).tobytes()), "i420": yuv420_ref.md5(yuv420_ref.i420(*got)),
                                      "nv12": yuv420_ref.md5(yuv420_ref.nv12(*got))}
                if name == smallest and m == 0 and s == -1:
                    rec["i420_zlib_b64"] = base64.b64encode(zlib.compress(yuv420_ref.i420(*got), 9)).decode()
            assert name in DEGENERATE or len({v["y"] for v in rec["md5"].values()}) == 3, (name, m, "the smoothings do not differ")
            recs[str(m)] = rec
        b.free(); o.delete()
        assert name not in REFUSED_BELOW or recs[str(REFUSED_BELOW[name])]["below_refused"], name
        out[name] = {"input": inp, "args": args, "smoothing": HEADER, "stream_md5": hashlib.md5(stream).hexdigest(), "width": cw, "height": ch,
                     "degenerate": name in DEGENERATE, "refused_below": REFUSED_BELOW.get(name), "decoded": recs}
        print("%-10s %s" % (name, " ".join("%s:%dx%d:%s" % (m, r["width"], r["height"], r["md5"]["-1"]["nv12"][:6]) for m, r in recs.items())))
    assert {"c102x66", "carry74_a"} <= cropped, cropped
    assert "i420_zlib_b64" in out[smallest]["decoded"]["0"]
    with open(os.path.join(HERE, "DECODED_420.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_decoded_420.py", "smoothing": list(yuv420_ref.SMOOTHING),
                   "bytes": "every plane clip255((p >> 4) + 128); i420: Y | Cb | Cr packed; nv12: Y | rows of Cb, Cr pairs", "cases": out}, f, indent=1)
        f.write("\n")
    print("DECODED_420.json: %d bytes" % os.path.getsize(os.path.join(HERE, "DECODED_420.json")))


if __name__ == "__main__":
    main()
