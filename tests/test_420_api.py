"""Decoding in 4:2:0 (include/libfiasco_amd_420.h), what can be checked without a GPU: the names in their header, the exports
map and their symbol table; the 4:2:0 border list (fiasco_amd_batch_smoothing_borders_420, host code: on the CPU oracle
library) applied sequentially to the oracle's 4:4:4 Y plane against the Y bytes the reference's decoder gives in 4:2:0
(tests/golden/DECODED_420.json) -- and that the 4:4:4 list does NOT give them; the refusals that need no device.  The kernel's
body replayed on the CPU is tests/test_420_step_host.py, the device side tests/test_gpu_420.py (-m gpu)."""
import ctypes
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fiasco_amd
import shown_ref
import smooth_ref
import yuv420_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["fiasco_amd_batch_decode_planes_420", "fiasco_amd_batch_smoothing_borders_420"]
DEVICE = ["fiasco_amd_batch_decode_device_420", "fiasco_amd_planes_to_420_device"]
NAMES = ["fiasco_amd_batch_decode_device_420", "fiasco_amd_batch_decode_planes_420", "fiasco_amd_batch_smoothing_borders_420",
         "fiasco_amd_planes_to_420_device"]


class FakeArray:
    def __init__(self, shape, typestr="|u1", ptr=0x10000, readonly=False, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, readonly), "version": 3, "strides": strides}


def _decls(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


def test_header_exports_map_and_symbol_table_hold_the_four_names(product, oracle):
    src = _decls("libfiasco_amd_420.h")
    older = "".join(_decls(h) for h in ("libfiasco_amd.h", "libfiasco_amd_hip.h", "libfiasco_amd_video.h", "libfiasco_amd_smooth.h",
                                        "libfiasco_amd_display.h", "libfiasco_amd_render.h"))
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert patterns
    assert set(re.findall(r"\b(fiasco_\w*)\s*\(", src)) == set(NAMES) and fiasco_amd.YUV420_SYMBOLS == NAMES
    assert NAMES == list(fiasco_amd._YUV420_SIGNATURES)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        assert params.count(",") + 1 == len(fiasco_amd._YUV420_SIGNATURES[name][1]), name
        assert not re.search(r"\b%s\s*\(" % name, older), name       # declared once
        assert name not in (fiasco_amd.EXPORTED_SYMBOLS + fiasco_amd.VIDEO_SYMBOLS + fiasco_amd.SMOOTH_SYMBOLS + fiasco_amd.DISPLAY_SYMBOLS
                            + fiasco_amd.RENDER_SYMBOLS), name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert hasattr(product.L, name), name
        assert getattr(product.L, name).argtypes == fiasco_amd._YUV420_SIGNATURES[name][1], name      # bound by Library.__init__
        assert hasattr(oracle.L, name) == (name in HOST), name      # the list and the host planes' entry are host code
    assert '#include "libfiasco_amd.h"' in src and '#include "libfiasco_amd_hip.h"' in src
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-x", "c", os.path.join(ROOT, "include", "libfiasco_amd_420.h")])
    assert [len(fiasco_amd._YUV420_SIGNATURES[n][1]) for n in NAMES] == [5, 4, 5, 7]
    # the structure as the header lays it out
    fields = re.search(r"typedef struct fiasco_amd_device_target_420 \{(.*?)\}", src, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[;,]", fields) == ["y", "y_pitch", "cb", "cr", "c_pitch", "c_step", "width", "height"]
    assert [f[0] for f in fiasco_amd.DeviceTarget420._fields_] == ["y", "y_pitch", "cb", "cr", "c_pitch", "c_step", "width", "height"]
    assert ctypes.sizeof(fiasco_amd.DeviceTarget420) == 56


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.decode_420; fiasco_amd.planes_to_420_device; "
            "assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_fixture_holds_what_the_tests_rely_on():
    doc = yuv420_ref.fixture()
    cases = doc["cases"]
    assert set(cases) == {"carry48_a", "carry74_a", "c102x66", "c256sq", "c320x200", "c34", "flat64"} and doc["smoothing"] == [0, -1, 35]
    size = {n: (e["width"], e["height"]) for n, e in cases.items()}
    assert size == {"carry48_a": (48, 70), "carry74_a": (74, 138), "c102x66": (102, 66), "c256sq": (256, 256), "c320x200": (320, 200),
                    "c34": (34, 34), "flat64": (64, 64)}
    assert [m for m, _ in yuv420_ref.accepted(cases["carry48_a"])] == [0, 1] == [m for m, _ in yuv420_ref.accepted(cases["c34"])]
    assert cases["carry48_a"]["decoded"]["0"]["below_refused"] and cases["c34"]["decoded"]["0"]["below_refused"]
    for n in ("c256sq", "c320x200", "c102x66", "flat64"):
        assert [m for m, _ in yuv420_ref.accepted(cases[n])] == [-1, 0, 1], n
    assert (cases["c102x66"]["decoded"]["0"]["width"] // 2, cases["c102x66"]["decoded"]["0"]["height"] // 2) == (51, 33)
    for n, e in cases.items():
        assert max(e["width"], e["height"]) <= 320 and e["degenerate"] == (n == "flat64"), n
        for m, r in yuv420_ref.accepted(e):
            assert r["width"] % 2 == 0 and r["height"] % 2 == 0 and set(r["md5"]) == {"0", "-1", "35"}, (n, m)
            assert (r["chroma_nonzero"] == 0) == e["degenerate"], (n, m)
            assert e["degenerate"] or len({v["y"] for v in r["md5"].values()}) == 3, (n, m)
    raw = yuv420_ref.unpack(cases["c34"]["decoded"]["0"]["i420_zlib_b64"])
    assert len(raw) == 34 * 34 + 2 * 17 * 17 and yuv420_ref.md5(raw) == cases["c34"]["decoded"]["0"]["md5"]["-1"]["i420"]


# ------------------------------------------------------------------ the list

LISTED = ("carry48_a", "carry74_a", "c102x66")


@pytest.fixture(scope="module")
def coded(oracle, inputs):
    """per case: the fixture's entry, the oracle's 4:4:4 planes at the coded size, the 4:2:0 list and the 4:4:4 list at
    M = 0 -- computed once on the oracle library and left alone"""
    out = {}
    for name in LISTED:
        ent = yuv420_ref.fixture_cases()[name]
        b, o = yuv420_ref.staged(oracle, inputs, ent)
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], name
        out[name] = (ent, b.decode_planes(0), b.smoothing_borders_420(0), b.smoothing_borders(0))
        b.free(); o.delete()
    return out


@pytest.mark.parametrize("name", LISTED)
def test_420_list_gives_the_reference_y_bytes_and_the_444_list_does_not(coded, name):
    ent, planes, list420, list444 = coded[name]
    rec = ent["decoded"]["0"]
    assert yuv420_ref.md5(planes[0].tobytes()) == rec["planes_md5"][0]          # unsmoothed, Y is the 4:4:4 plane
    assert yuv420_ref.md5(yuv420_ref.to_bytes(planes[0]).tobytes()) == rec["md5"]["0"]["y"]
    for key, n in (("35", 35), ("-1", ent["smoothing"])):
        want = rec["md5"][key]["y"]
        got = yuv420_ref.to_bytes(smooth_ref.smooth(planes[0], list420, n))
        assert yuv420_ref.md5(got.tobytes()) == want, (name, n)
        other = yuv420_ref.to_bytes(smooth_ref.smooth(planes[0], list444, n))
        differing = int(np.count_nonzero(other != got))
        print("%s -s %d: %d of %d Y bytes differ between the 4:2:0 and the 4:4:4 list" % (name, n, differing, got.size))
        assert differing > 0 and yuv420_ref.md5(other.tobytes()) != want, (name, n)


@pytest.mark.parametrize("name", LISTED)
def test_420_list_is_the_y_phase_then_the_cb_phase_one_step_down(coded, name):
    ent, planes, list420, list444 = coded[name]
    w, h = ent["width"], ent["height"]
    shown_ref.pixels_touched(list420, w, h)                     # asserts: the borders of one pass share no pixel
    passes = [b[4] for b in list420]
    assert passes == sorted(passes) and passes[0] == 0 and set(passes) == set(range(passes[-1] + 1))
    # the level falls exactly once in either list, where the Cb phase begins; the Y phase is the 4:4:4 one
    def phases(borders):
        levels = {}
        for b in borders:
            levels.setdefault(b[4], b[3])
        order = [levels[p] for p in sorted(levels)]
        drops = [k for k in range(1, len(order)) if order[k] <= order[k - 1]]
        assert len(drops) == 1, order
        first_cb = sorted(levels)[drops[0]]
        return [b for b in borders if b[4] < first_cb], [b for b in borders if b[4] >= first_cb]
    y420, cb420 = phases(list420)
    y444, cb444 = phases(list444)
    assert y420 == y444
    # the Cb phase: x, y >> 1, level - 2, the length that level's side clipped at the full-size plane; borders that land on
    # the first row or column have no pixel before them and drop out
    want = []
    for x, y, _, level, _ in cb444:
        x, y, level = x >> 1, y >> 1, level - 2
        assert level >= 1
        if (level & 1 and not y) or (not level & 1 and not x):
            continue
        want.append((x, y, min(shown_ref.side(level), w - x if level & 1 else h - y), level))
    got = [b[:4] for b in cb420]
    assert want and set(want) <= set(got) and [b for b in got if b in set(want)] == sorted(want, key=lambda b: (b[3], got.index(b)))
    # what the 4:2:0 list has beyond that are Cb states the 4:4:4 list leaves out because they begin outside the frame: at half
    # their coordinates they lie inside the Y plane, and the reference smooths along them
    extra = [b for b in got if b not in set(want)]
    assert all(2 * x + 1 >= w or 2 * y + 1 >= h for x, y, _, _ in extra), extra
    assert name != "carry48_a" or extra


# ------------------------------------------------------------------ refusals

def test_gray_frame_and_degenerate_frame_are_refused_by_host_code(oracle, inputs):
    o = oracle.cli_options()
    b = fiasco_amd.Batch(oracle, [inputs.data("g96x64")], 20.0, o)
    assert b.encode()[0] is not None
    for call in (lambda: b.decode_planes_420(0), lambda: b.smoothing_borders_420(0)):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            call()
        assert "4:2:0" in str(e.value) and "gray frame" in str(e.value), str(e.value)
    b.free(); o.delete()
    ent = yuv420_ref.fixture_cases()["flat64"]
    b, o = yuv420_ref.staged(oracle, inputs, ent)
    stream = b.encode()[0]
    assert hashlib.md5(stream).hexdigest() == ent["stream_md5"]
    assert b.decode_planes(0)[1:].any()                         # the 4:4:4 decode has colour
    for m in (-1, 0, 1):
        for call in (lambda: b.decode_planes_420(0, magnify=m), lambda: b.smoothing_borders_420(0, magnify=m)):
            with pytest.raises(fiasco_amd.FiascoError) as e:
                call()
            found = re.search(r"max_level (\d+) at magnification (-?\d+) takes chroma states of level (\d+), the chroma root has level (\d+)", str(e.value))
            assert found and "stay zero" in str(e.value), str(e.value)
            top, mag, want, root = (int(v) for v in found.groups())
            assert mag == m and want == top - 2 * m + 2 and root < want and root == 12, str(e.value)       # 64 x 64: level 12
    b.free(); o.delete()


def test_a_library_whose_decoder_has_no_420_says_so(coded, oracle, inputs):
    ent = coded["carry48_a"][0]
    b, o = yuv420_ref.staged(oracle, inputs, ent)
    b.encode()
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_planes_420(0)
    assert "oracle-cpu" in str(e.value) and "does not decode 4:2:0" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_planes_420(0, magnify=-1)                      # 48 x 70: the size rule comes first
    assert "Minimum value is 0." in str(e.value)
    b.free(); o.delete()


def _target(y=0x100000, y_pitch=0, cb=0x200000, cr=0x300000, c_pitch=0, c_step=1, width=96, height=64):
    t = (fiasco_amd.DeviceTarget420 * 1)()
    t[0].y, t[0].y_pitch, t[0].cb, t[0].cr, t[0].c_pitch, t[0].c_step, t[0].width, t[0].height = y, y_pitch, cb, cr, c_pitch, c_step, width, height
    return t


def test_target_refusals_that_come_before_the_device_is_looked_for(product, inputs):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [yuv420_ref.synth_input("colork:96:64:0")[0]], 20.0, o)
    L = product.L

    def refused(t, *words, magnify=0):
        assert L.fiasco_amd_batch_decode_device_420(b.handle, magnify, 0, t, None) == 0
        msg = product.error_message()
        assert all(w in msg for w in words), msg
        if not magnify:                                         # the kernel's own entry checks the same, before any device
            assert L.fiasco_amd_planes_to_420_device(0x1000, 0x2000, 0x3000, 96, 64, t, None) == 0
            assert all(w in product.error_message() for w in words), product.error_message()

    refused(_target(c_step=0), "c_step 0")
    refused(_target(c_step=3), "c_step 3")
    refused(_target(c_step=2, cb=0x200000, cr=0x200002), "not one byte apart")
    refused(_target(c_step=2, cb=0x200000, cr=0x200000), "not one byte apart")
    refused(_target(y_pitch=95), "Y pitch of 95 bytes is smaller than a row of 96")
    refused(_target(c_pitch=47), "chroma pitch of 47 bytes is smaller than a row of 48")
    refused(_target(c_step=2, cr=0x200001, c_pitch=95), "chroma pitch of 95 bytes is smaller than a row of 96")
    refused(_target(width=48, height=32), "48 x 32 pixels for a frame of 96 x 64")
    refused(_target(width=96, height=64), "96 x 64 pixels for a frame of 96 x 64 at magnification 1: 192 x 128", magnify=1)
    refused(_target(cb=0x100000 + 96 * 64 - 1), "the Y rows and the chroma rows overlap")
    refused(_target(y=0x200000 + 48 * 32 - 1, cb=0x200000), "the Y rows and the chroma rows overlap")
    refused(_target(c_step=2, cb=0x100000 + 96 * 63, cr=0x100000 + 96 * 63 + 1), "the Y rows and the chroma rows overlap")
    refused(_target(cb=0x200000, cr=0x200000 + 48 * 32 - 1), "the Cb rows and the Cr rows overlap")
    refused(_target(cb=0x200000, cr=0x200000 + 40, c_pitch=96), "the Cb rows and the Cr rows overlap")
    # what is no refusal gets as far as the device or the missing pass: packed planes back to back, chroma side by side in one surface
    for t in (_target(cb=0x100000 + 96 * 64, cr=0x100000 + 96 * 64 + 48 * 32), _target(cb=0x200000, cr=0x200000 + 48, c_pitch=96),
              _target(c_step=2, cb=0x200001, cr=0x200000)):
        assert L.fiasco_amd_batch_decode_device_420(b.handle, 0, 0, t, None) == 0
        msg = product.error_message()
        assert "no HIP device available" in msg or "no finished pass" in msg, msg
    assert L.fiasco_amd_batch_decode_device_420(None, 0, 0, None, None) == 0 and "empty batch" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_420(b.handle, 0, 0, None, None) == 0 and "no targets" in product.error_message()
    for bad in (-2, 101):
        assert L.fiasco_amd_batch_decode_device_420(b.handle, 0, bad, _target(), None) == 0 and "smoothing out of range" in product.error_message()
    assert L.fiasco_amd_planes_to_420_device(None, None, None, 96, 64, _target(), None) == 0 and "no planes" in product.error_message()
    for w, h in ((97, 64), (96, 0), (8194, 64)):
        assert L.fiasco_amd_planes_to_420_device(0x1000, 0x2000, 0x3000, w, h, _target(width=w, height=h), None) == 0
        assert "even, 2 .. 8192" in product.error_message()
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.smoothing_borders_420(0)
    assert "no finished automaton" in str(e.value)
    b.free(); o.delete()


def test_python_targets_are_checked_before_anything_is_called():
    b = fiasco_amd.Batch.__new__(fiasco_amd.Batch)
    b.lib, b.handle, b.n, b._keep, b._geom = None, 0x10, 1, None, [(96, 64, 3)]
    y, c, cc = FakeArray((64, 96)), FakeArray((32, 48), ptr=0x20000), FakeArray((32, 48, 2), ptr=0x20000)
    for targets, word in (([(FakeArray((64, 96), readonly=True), c, c)], "read-only"),
                          ([(y, FakeArray((32, 48), readonly=True), c)], "read-only"),
                          ([(y, FakeArray((32, 48, 2), readonly=True))], "read-only"),
                          ([(FakeArray((64, 96), typestr="<i2"), c, c)], "not bytes"),
                          ([(y, c, FakeArray((32, 48), typestr="<f4"))], "not bytes"),
                          ([(y, c, FakeArray((32, 47)))], "chroma planes of"),
                          ([(y, FakeArray((32, 47, 2)))], "interleaved chroma plane"),
                          ([(y, FakeArray((32, 48)))], "dimensions expected"),
                          ([(y, c, FakeArray((32, 48), strides=(64, 1)))], "one pitch expected"),
                          ([(y, FakeArray((32, 48, 2), strides=(96, 1, 48)))], "cannot be described by a pitch"),
                          ([(y,)], "(y, cb, cr) or (y, cbcr)"), ([object()], ""), ([], "0 targets for a batch of 1")):
        with pytest.raises((fiasco_amd.FiascoError, TypeError)) as e:
            b.decode_420(targets)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_420([(y, cc)], order="yv12")
    assert "nv12" in str(e.value)
    # what the wrapper hands over
    t = fiasco_amd._device_targets_420([(y, c, FakeArray((32, 48), ptr=0x30000)), (y, cc), None])
    assert (t[0].y, t[0].cb, t[0].cr, t[0].c_step, t[0].y_pitch, t[0].c_pitch, t[0].width, t[0].height) == (0x10000, 0x20000, 0x30000, 1, 96, 48, 96, 64)
    assert (t[1].cb, t[1].cr, t[1].c_step, t[1].c_pitch) == (0x20000, 0x20001, 2, 96) and not t[2].y
    t = fiasco_amd._device_targets_420([(y, cc)], "nv21")
    assert (t[0].cb, t[0].cr, t[0].c_step) == (0x20001, 0x20000, 2)


class Recorder:
    """stands in for Library: every C function called is written down and answers 1"""

    def __init__(self):
        self.calls = []
        self.L = self

    def __getattr__(self, name):
        if not name.startswith("fiasco_amd_"):
            raise AttributeError(name)
        return lambda *args: self.calls.append((name, args)) or 1

    def error_message(self):
        return ""


def test_python_defaults_call_the_entries_they_name():
    lib = Recorder()
    b = fiasco_amd.Batch.__new__(fiasco_amd.Batch)
    b.lib, b.handle, b.n, b._keep, b._geom = lib, 0x10, 1, None, [(96, 64, 3)]
    t = [(FakeArray((64, 96)), FakeArray((32, 48, 2), ptr=0x20000))]
    assert b.decode_420(t) == 1 and b.decode_420(t, magnify=-1, smoothing=35, order="nv21") == 1
    (n0, a0), (n1, a1) = lib.calls
    assert n0 == n1 == "fiasco_amd_batch_decode_device_420" and a0[:3] == (0x10, 0, -1) and a1[:3] == (0x10, -1, 35)
    assert a0[3][0].cr == a0[3][0].cb + 1 and a1[3][0].cb == a1[3][0].cr + 1
    del lib.calls[:]
    b.smoothing_borders_420(0, magnify=1)
    assert [k[0] for k in lib.calls] == ["fiasco_amd_batch_smoothing_borders_420"] * 2 and lib.calls[0][1][:3] == (0x10, 0, 1)
    del lib.calls[:]
    planes = [FakeArray((64, 96), typestr="<i2", ptr=0x1000), FakeArray((32, 48), typestr="<i2", ptr=0x2000), FakeArray((32, 48), typestr="<i2", ptr=0x3000)]
    fiasco_amd.planes_to_420_device(lib, planes[0], planes[1], planes[2], t[0])
    name, a = lib.calls[0]
    assert name == "fiasco_amd_planes_to_420_device" and a[:5] == (0x1000, 0x2000, 0x3000, 96, 64)
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.planes_to_420_device(lib, planes[0], planes[1], FakeArray((32, 47), typestr="<i2"), t[0])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_the_calls_fail_loudly_without_gpu(product, inputs):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [yuv420_ref.synth_input("colork:96:64:0")[0]], 20.0, o)
    assert b.encode() == [None]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_420([(FakeArray((64, 96)), FakeArray((32, 48, 2), ptr=0x20000))])
    assert "no HIP device available" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.planes_to_420_device(product, FakeArray((64, 96), typestr="<i2", ptr=0x1000), FakeArray((32, 48), typestr="<i2", ptr=0x2000),
                                        FakeArray((32, 48), typestr="<i2", ptr=0x3000), (FakeArray((64, 96)), FakeArray((32, 48, 2), ptr=0x20000)))
    assert "no HIP device available" in str(e.value)
    b.free(); o.delete()
