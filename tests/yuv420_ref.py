"""What the tests of the 4:2:0 decode share (tests/test_420_api.py, tests/test_gpu_420.py, tests/test_420_step_host.py's
program through its own copy of the formula, the generator tests/golden/make_decoded_420.py): the fixture
tests/golden/DECODED_420.json, the inputs of its cases, the bytes of a plane, the buffers a target is compared with, and
hand-made planes that meet the clip bounds."""
import base64
import hashlib
import json
import os
import zlib

import numpy as np

import shown_ref
import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMOOTHING = (0, -1, 35)
# p >> 4 of these meets the two bounds of clip255((p >> 4) + 128) from both sides
SPECIALS = (-129, -128, 127, 128)


def fixture():
    return json.load(open(os.path.join(GOLDEN, "DECODED_420.json")))


def fixture_cases():
    return fixture()["cases"]


def synth_input(spec):
    """flat:W:H:R:G:B -> a PPM of one colour; colork:W:H:SHIFT -> a PPM of synth.synth_color_k(W, H, 1234, SHIFT), whose chroma
    survives the coder; else shown_ref.synth_input.  (bytes, extension) or None"""
    part = spec.split(":")
    if part[0] == "colork":
        w, h, shift = (int(v) for v in part[1:])
        return synth.ppm_bytes(synth.synth_color_k(w, h, 1234, shift)), "ppm"
    if part[0] == "flat":
        w, h, r, g, b = (int(v) for v in part[1:])
        return synth.ppm_bytes(np.broadcast_to(np.array([r, g, b], dtype=np.uint8), (h, w, 3)).copy()), "ppm"
    return shown_ref.synth_input(spec)


def case_input(inputs, ent):
    made = synth_input(ent["input"])
    return made[0] if made else inputs.data(ent["input"])


def staged(lib, inputs, ent):
    """a fixture case as a batch of one frame, not yet encoded -> (batch, options)"""
    import fiasco_amd
    from conftest import options_from_args
    q, o = options_from_args(lib, ent["args"])
    o.set_smoothing(ent["smoothing"])
    return fiasco_amd.Batch(lib, [case_input(inputs, ent)], q, o), o


def accepted(ent):
    """[(M, record)] of the magnifications recorded for the case"""
    return [(int(m), r) for m, r in sorted(ent["decoded"].items(), key=lambda kv: int(kv[0]))]


def to_bytes(plane):
    """clip255((p >> 4) + 128) of an int16 plane: the byte of Y, Cb and Cr alike"""
    return np.clip((np.asarray(plane).astype(np.int32) >> 4) + 128, 0, 255).astype(np.uint8)


def i420(y, cb, cr):
    """the packed I420 buffer of three int16 planes, as bytes"""
    return to_bytes(y).tobytes() + to_bytes(cb).tobytes() + to_bytes(cr).tobytes()


def nv12(y, cb, cr):
    """the packed NV12 buffer: the Y plane, then the rows of Cb, Cr pairs"""
    return to_bytes(y).tobytes() + np.stack([to_bytes(cb), to_bytes(cr)], -1).tobytes()


def nv21(y, cb, cr):
    return nv12(y, cr, cb)


def md5(data):
    return hashlib.md5(data).hexdigest()


def unpack(b64):
    return zlib.decompress(base64.b64decode(b64))


def handmade(w, h):
    """three int16 planes, Y h x w and two of h/2 x w/2, from a closed formula: full-range values with fraction bits, every
    plane meeting the clip bounds (SPECIALS) in its first positions wherever it has room for them"""
    out = []
    for k, (ph, pw) in enumerate(((h, w), (h // 2, w // 2), (h // 2, w // 2))):
        i = np.arange(ph * pw, dtype=np.int64)
        v = ((i * 7919 + k * 104729 + 12345) * 2654435761 % 65536 - 32768).astype(np.int16)
        for j, s in enumerate(SPECIALS):
            if j < v.size:
                v[j] = s * 16 + (j * 5) % 16
        out.append(v.reshape(ph, pw))
    return out


FORMULA = ("plane k (0: Y h x w, 1, 2: h/2 x w/2), value i in raster order: ((i * 7919 + k * 104729 + 12345) * 2654435761 mod 65536) "
           "- 32768 as int16; then value j < 4 = SPECIALS[j] * 16 + (5 j mod 16)")
