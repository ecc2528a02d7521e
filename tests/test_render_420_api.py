"""Frames decoded in 4:2:0 in the pixel formats of a display (include/libfiasco_amd_render_420.h), what can be checked without a
GPU: the names in their header, the exports map and the symbol table; the host loop fiasco_amd_renderer_render_planes_420
against the REAL reference's renderer (tests/golden/RENDERED_420.json, tests/golden/make_rendered_420.py) on the hand-made
planes; against the numpy model tests/render420_ref.py on full-range planes, where the reference reads past its tables and
this code clamps; the size rule with every refusal, its message and an untouched buffer; the wrapper's refusals.  The
fixture's decoded frames are compared on the device (tests/test_gpu_render_420.py, -m gpu): the CPU oracle decodes neither
4:2:0 nor at a magnification, so it cannot supply the chroma planes of any recorded frame (the 4:4:4 chroma at M - 1).  The
kernel's per-item functions replayed on the CPU are tests/test_render_420_step_host.py."""
import ctypes
import os
import re
import subprocess
import sys
import zlib
import base64

import numpy as np
import pytest

import fiasco_amd
import render420_ref
import render_ref
import yuv420_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["fiasco_amd_renderer_surface_size_420", "fiasco_amd_renderer_render_planes_420"]
DEVICE = ["fiasco_amd_planes_render_device_420", "fiasco_amd_batch_decode_device_rendered_420"]
NAMES = HOST + DEVICE
OLDER = ("libfiasco_amd.h", "libfiasco_amd_hip.h", "libfiasco_amd_video.h", "libfiasco_amd_smooth.h", "libfiasco_amd_display.h",
         "libfiasco_amd_render.h", "libfiasco_amd_420.h", "libfiasco_amd_ycbcr.h")
SIZES = [(4, 2), (18, 4), (36, 6), (5, 4), (4, 3)]


class FakeArray:
    def __init__(self, shape, typestr="|u1", ptr=0x1000, strides=None, readonly=False):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, readonly), "version": 3, "strides": strides}


def _decls(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


@pytest.fixture(scope="module")
def renderers(product):
    made = {n: fiasco_amd.Renderer(product, red, green, blue, bpp, doubled) for n, (bpp, red, green, blue, doubled) in render_ref.RENDERERS.items()}
    yield made
    for r in made.values():
        r.delete()


def test_header_symbol_list_and_library_hold_the_four_names(product, oracle):
    src = _decls("libfiasco_amd_render_420.h")
    older = "".join(_decls(h) for h in OLDER)
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert set(re.findall(r"\b(fiasco_\w*)\s*\(", src)) == set(NAMES) and fiasco_amd.RENDER420_SYMBOLS == NAMES
    assert NAMES == list(fiasco_amd._RENDER420_SIGNATURES)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    every_older_list = (fiasco_amd.EXPORTED_SYMBOLS + fiasco_amd.VIDEO_SYMBOLS + fiasco_amd.SMOOTH_SYMBOLS + fiasco_amd.DISPLAY_SYMBOLS
                        + fiasco_amd.RENDER_SYMBOLS + fiasco_amd.YUV420_SYMBOLS + fiasco_amd.YCBCR_SYMBOLS)
    for name in NAMES:
        assert len(re.findall(r"\b%s\s*\(" % name, src)) == 1, name                     # declared once
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        assert params.count(",") + 1 == len(fiasco_amd._RENDER420_SIGNATURES[name][1]), name
        assert not re.search(r"\b%s\b" % name, older), name
        assert name not in every_older_list, name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert getattr(product.L, name).argtypes == fiasco_amd._RENDER420_SIGNATURES[name][1], name     # bound by Library.__init__
        assert not hasattr(oracle.L, name), name                                        # the oracle library has no renderer
    assert '#include "libfiasco_amd_render.h"' in src
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-x", "c", os.path.join(ROOT, "include", "libfiasco_amd_render_420.h")])
    assert [len(fiasco_amd._RENDER420_SIGNATURES[n][1]) for n in NAMES] == [6, 7, 8, 6]


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.decode_rendered_420; fiasco_amd.render_planes_device_420; "
            "assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_fixture_holds_what_the_tests_rely_on():
    fx = render420_ref.fixture()
    assert fx["generator"] == "tests/golden/make_rendered_420.py" and fx["handmade"]["formula"] == render420_ref.FORMULA
    assert fx["renderers"] == render_ref.fixture()["renderers"] and len(fx["renderers"]) == 12
    cases420 = yuv420_ref.fixture_cases()
    assert set(fx["decoded"]) == {"carry48_a", "c34", "c102x66", "carry74_a", "flat64"}
    seen_refused = 0
    for name, e in fx["decoded"].items():
        assert e["stream_md5"] == cases420[name]["stream_md5"] and set(e["rendered"]) == set(cases420[name]["decoded"]), name
        assert e["degenerate"] == (name == "flat64")
        for m, rec in e["rendered"].items():
            assert (rec["width"], rec["height"]) == (cases420[name]["decoded"][m]["width"], cases420[name]["decoded"][m]["height"])
            assert set(rec["md5"]) == {"0", "-1"}
            for n in render_ref.RENDERERS:
                no = e["degenerate"] or render420_ref.refused_named(n, rec["width"], rec["height"])
                seen_refused += no and not e["degenerate"]
                assert (rec["md5"]["0"][n] == "refused") == no == (rec["md5"]["-1"][n] == "refused"), (name, m, n)
                assert no or rec["md5"]["0"][n] != rec["md5"]["-1"][n], (name, m, n)          # smoothing changes the bytes
    assert seen_refused >= 6
    hm = fx["handmade"]["planes"]
    assert set(hm) == {"36x6", "34x4"} and len(hm["36x6"]["renderers"]) == 12
    assert set(render_ref.RENDERERS) - set(hm["34x4"]["renderers"]) == {"rgb24", "bgr24"}
    assert {n for n, r in hm["36x6"]["renderers"].items() if "bytes_zlib_b64" in r} == set(render420_ref.WITH_BYTES)
    assert {render_ref.RENDERERS[n][0] for n in render420_ref.WITH_BYTES} == {16, 24, 32}
    assert os.path.getsize(os.path.join(render_ref.GOLDEN, "RENDERED_420.json")) < 64 * 1024


def test_host_loop_gives_the_references_bytes_on_the_handmade_planes(renderers):
    for key, e in render420_ref.fixture()["handmade"]["planes"].items():
        w, h = e["width"], e["height"]
        planes = render420_ref.handmade(w, h)
        assert [render_ref.md5(p.tobytes()) for p in planes] == e["planes_md5"], key
        for n, r in renderers.items():
            if n not in e["renderers"]:
                assert render420_ref.refused_named(n, w, h), (key, n)
                with pytest.raises(fiasco_amd.FiascoError):
                    r.render_planes_420(*planes)
                continue
            rec = e["renderers"][n]
            got = r.render_planes_420(*planes)
            if "bytes_zlib_b64" in rec:         # a mismatch can be read: the first byte that differs
                want = zlib.decompress(base64.b64decode(rec["bytes_zlib_b64"]))
                diff = [k for k in range(min(len(got), len(want))) if got[k] != want[k]][:1]
                assert got == want, (key, n, len(got), len(want), diff, got[diff[0]:diff[0] + 8].hex() if diff else None)
            assert render_ref.md5(got) == rec["md5"], (key, n)
            assert got == render420_ref.render_named(*planes, n).tobytes(), (key, n)


def test_host_loop_clamps_where_numpy_clamps_on_full_range_planes(renderers):
    """values outside the reference's tables: the clamp is pinned by numpy, not by the reference"""
    rng = np.random.RandomState(420)
    y = rng.randint(-32768, 32768, size=(4, 64)).astype(np.int16)
    cb, cr = (rng.randint(-32768, 32768, size=(2, 32)).astype(np.int16) for _ in range(2))
    for p in (y, cb, cr):
        p.reshape(-1)[:8] = [-32768, 32767, -2049, 2047, -2064, 2048, -1, 0]
    hit = render_ref.rgb(render420_ref.replicated(y, cb, cr))
    assert any(v.min() < -1024 for v in hit) and any(v.max() > 1279 for v in hit)             # beyond the reference's widest table
    for n, r in renderers.items():
        assert r.render_planes_420(y, cb, cr) == render420_ref.render_named(y, cb, cr, n).tobytes(), n


def test_every_chroma_sample_serves_its_four_pixels(renderers):
    """one chroma sample that differs from the rest: exactly its 2 x 2 pixels change, in the undoubled 32 bpp surface"""
    y = np.zeros((4, 8), dtype=np.int16)
    cb, cr = np.zeros((2, 4), dtype=np.int16), np.zeros((2, 4), dtype=np.int16)
    base = np.frombuffer(renderers["xrgb8888"].render_planes_420(y, cb, cr), dtype=np.uint32).reshape(4, 8)
    cb[1, 2] = 100 * 16
    got = np.frombuffer(renderers["xrgb8888"].render_planes_420(y, cb, cr), dtype=np.uint32).reshape(4, 8)
    changed = got != base
    assert changed[2:4, 4:6].all() and changed.sum() == 4


def test_surface_size_420_for_all_twelve_renderers(product, renderers):
    for n, r in renderers.items():
        bpp, _, _, _, doubled = render_ref.RENDERERS[n]
        for w, h in SIZES:
            if render420_ref.refused(bpp, doubled, w, h):
                with pytest.raises(fiasco_amd.FiascoError) as e:
                    r.surface_size_420(w, h)
                msg = str(e.value)
                assert "fiasco_amd_renderer: 4:2:0" in msg, (n, w, h, msg)
                assert ("is odd" in msg) == bool((w | h) & 1) and ("not a multiple of 4" in msg) == (not (w | h) & 1), (n, w, h, msg)
            else:
                assert r.surface_size_420(w, h) == render420_ref.surface_size(bpp, doubled, w, h), (n, w, h)
    # which of them are refused: the odd sides for everyone, 18 x 4 at 24 bpp not doubled
    assert [render420_ref.refused(32, d, w, h) for d in (False, True) for w, h in SIZES] == [False, False, False, True, True] * 2
    assert [render420_ref.refused(16, False, w, h) for w, h in SIZES] == [False, False, False, True, True]
    assert [render420_ref.refused(24, False, w, h) for w, h in SIZES] == [False, True, False, True, True]
    assert [render420_ref.refused(24, True, w, h) for w, h in SIZES] == [False, False, False, True, True]
    # NULL outputs are allowed; an empty or oversized frame and a missing renderer are not
    r = renderers["rgb565"]
    L = product.L
    assert L.fiasco_amd_renderer_surface_size_420(r.handle, 36, 6, None, None, None) == 1
    for w, h in ((0, 4), (4, 0), (16386, 2)):
        assert L.fiasco_amd_renderer_surface_size_420(r.handle, w, h, None, None, None) == 0
        assert "1 .. 16384" in product.error_message()
    assert L.fiasco_amd_renderer_surface_size_420(None, 4, 4, None, None, None) == 0 and "renderer" in product.error_message()


def test_refused_renders_write_nothing(product, renderers):
    L = product.L
    y, cb, cr = np.zeros((6, 36), dtype=np.int16), np.zeros((3, 18), dtype=np.int16), np.zeros((3, 18), dtype=np.int16)
    buf = ctypes.create_string_buffer(b"\x5a" * 4096, 4096)
    cases = [("rgb24", 18, 4, "not a multiple of 4"), ("bgr24", 34, 4, "not a multiple of 4"), ("rgb24_x2", 5, 4, "is odd"), ("rgb565", 4, 3, "is odd"),
             ("xrgb8888", 35, 6, "is odd"), ("xrgb8888_x2", 0, 2, "1 .. 16384")]
    for n, w, h, word in cases:
        assert L.fiasco_amd_renderer_render_planes_420(renderers[n].handle, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, w, h, buf) == 0, n
        assert word in product.error_message(), (n, product.error_message())
        assert buf.raw == b"\x5a" * 4096, n
    r = renderers["xrgb8888"].handle
    for args in ((None, cb.ctypes.data, cr.ctypes.data), (y.ctypes.data, None, cr.ctypes.data), (y.ctypes.data, cb.ctypes.data, None)):
        assert L.fiasco_amd_renderer_render_planes_420(r, args[0], args[1], args[2], 36, 6, buf) == 0 and "no planes" in product.error_message()
    assert L.fiasco_amd_renderer_render_planes_420(r, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, 36, 6, None) == 0 and "no surface" in product.error_message()
    assert L.fiasco_amd_renderer_render_planes_420(None, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, 36, 6, buf) == 0 and "renderer" in product.error_message()
    assert buf.raw == b"\x5a" * 4096
    # an accepted one fills exactly its surface
    assert L.fiasco_amd_renderer_render_planes_420(r, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, 36, 6, buf) == 1
    assert buf.raw[36 * 6 * 4:] == b"\x5a" * (4096 - 36 * 6 * 4) and b"\x5a" not in buf.raw[:36 * 6 * 4]
    for bad in ((y, cb, cr[:2]), (y, cb[:, :17], cr), (y[0], cb, cr)):
        with pytest.raises(fiasco_amd.FiascoError):
            renderers["xrgb8888"].render_planes_420(*bad)


def test_python_side_refusals(product, inputs, renderers):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    r32, r16, r24 = renderers["xrgb8888"], renderers["rgb565"], renderers["rgb24"]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered_420(r32, [])                                                  # one surface per frame
    assert "decode_rendered_420: 0 surfaces for a batch of 1" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered_420(r32, [FakeArray((64, 96, 4)), FakeArray((64, 96, 4))])
    assert "2 surfaces for a batch of 1" in str(e.value)
    planes = (FakeArray((64, 96), typestr="<i2"), FakeArray((32, 48), typestr="<i2", ptr=0x8000), FakeArray((32, 48), typestr="<i2", ptr=0xc000))
    bad = [(r32, FakeArray((64, 96)), "is not H x W x 4"), (r16, FakeArray((64, 96, 4)), "is not H x W x 2"), (r24, FakeArray((64, 96, 3, 1)), "is not H x W x 3"),
           (r32, FakeArray((64, 96, 4), typestr="<u4"), "uint8"), (r32, FakeArray((64, 96, 4), strides=(96 * 8, 8, 1)), "strides"),
           (r32, FakeArray((64, 96, 4), readonly=True), "read-only"), (r32, object(), "not in device memory")]
    for r, s, word in bad:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_rendered_420(r, [s])
        assert word in str(e.value), (word, str(e.value))
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.render_planes_device_420(product, r, planes[0], planes[1], planes[2], s)
        assert word in str(e.value), (word, str(e.value))
    good = FakeArray((64, 96, 4))
    for y, cb, cr, word in ((planes[0], planes[1], FakeArray((32, 47), typestr="<i2"), "chroma planes of"), (planes[0], planes[0], planes[2], "chroma planes of"),
                            (FakeArray((3, 64, 96), typestr="<i2"), planes[1], planes[2], "two dimensions"),
                            (FakeArray((64, 96), typestr="<f4"), planes[1], planes[2], "int16"), (planes[0], object(), planes[2], "not in device memory")):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.render_planes_device_420(product, r32, y, cb, cr, good)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.render_planes_device_420(product, r32, planes[0], planes[1], planes[2], None)
    assert "no surface" in str(e.value)
    # the C entries before a device is looked for
    L = product.L
    s = fiasco_amd._device_surfaces([good], 32)
    name = "fiasco_amd_batch_decode_device_rendered_420"
    assert L.fiasco_amd_batch_decode_device_rendered_420(None, r32.handle, 0, -1, s, None) == 0 and "empty batch" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_rendered_420(b.handle, None, 0, -1, s, None) == 0 and "no renderer" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_rendered_420(b.handle, r32.handle, 0, -1, None, None) == 0 and "no surfaces" in product.error_message()
    for smoothing in (-2, 101):
        assert L.fiasco_amd_batch_decode_device_rendered_420(b.handle, r32.handle, 0, smoothing, s, None) == 0
        assert "smoothing out of range" in product.error_message() and name in product.error_message()
    assert L.fiasco_amd_planes_render_device_420(None, 0x8000, 0xc000, 96, 64, r32.handle, s, None) == 0 and "no planes" in product.error_message()
    assert L.fiasco_amd_planes_render_device_420(0x4000, 0x8000, 0xc000, 96, 64, None, s, None) == 0 and "no renderer" in product.error_message()
    b.free(); o.delete()


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
    b.lib, b.handle, b.n, b._keep, b._geom = lib, 0x10, 1, None, [(96, 64, 1)]
    r = fiasco_amd.Renderer(lib, 0xf800, 0x7e0, 0x1f, 16, True)
    del lib.calls[:]
    s = [FakeArray((128, 192, 2))]
    assert b.decode_rendered_420(r, s) == 1 and b.decode_rendered_420(r, s, magnify=-1, smoothing=0) == 1
    (n0, a0), (n1, a1) = lib.calls
    assert n0 == n1 == "fiasco_amd_batch_decode_device_rendered_420" and a0[:4] == (0x10, 1, 0, -1) and a1[:4] == (0x10, 1, -1, 0)
    assert (a0[4][0].width, a0[4][0].height, a0[4][0].pitch) == (192, 128, 384)
    del lib.calls[:]
    fiasco_amd.render_planes_device_420(lib, r, FakeArray((64, 96), typestr="<i2", ptr=0x2000), FakeArray((32, 48), typestr="<i2", ptr=0x6000),
                                        FakeArray((32, 48), typestr="<i2", ptr=0x7000), s[0])
    name, a = lib.calls[0]
    assert name == "fiasco_amd_planes_render_device_420" and a[:6] == (0x2000, 0x6000, 0x7000, 96, 64, 1)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_the_device_calls_fail_loudly_without_gpu(product, inputs, renderers):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    assert b.encode() == [None]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered_420(renderers["xrgb8888"], [FakeArray((64, 96, 4))])
    assert "no HIP device available" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.render_planes_device_420(product, renderers["rgb565"], FakeArray((64, 96), typestr="<i2"), FakeArray((32, 48), typestr="<i2"),
                                            FakeArray((32, 48), typestr="<i2"), FakeArray((64, 96, 2)))
    assert "no HIP device available" in str(e.value)
    b.free(); o.delete()
