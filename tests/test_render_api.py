"""Decoded frames in the pixel formats of a display (include/libfiasco_amd_render.h), what can be checked without a GPU: the
names in their header, the exports map and the symbol table; the host loop fiasco_amd_renderer_render_planes against the
REAL reference's renderer (tests/golden/RENDERED.json, tests/golden/make_rendered.py) on the hand-made planes and on the
planes the CPU oracle decodes for the coded cases; against the numpy restatement
tests/render_ref.py on full-range planes, where the reference reads past its tables and this code clamps; every refusal with
its message and an untouched buffer; the surface sizes; the wrapper's refusals.  The kernel's per-item function replayed on
the CPU is tests/test_render_step_host.py, the device side tests/test_gpu_render.py (-m gpu)."""
import base64
import ctypes
import hashlib
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

import fiasco_amd
import render_ref
import shown_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["fiasco_amd_renderer_new", "fiasco_amd_renderer_delete", "fiasco_amd_renderer_surface_size", "fiasco_amd_renderer_render_planes"]
DEVICE = ["fiasco_amd_planes_render_device", "fiasco_amd_batch_decode_device_rendered"]
NAMES = HOST + DEVICE
OLDER = ("libfiasco_amd.h", "libfiasco_amd_hip.h", "libfiasco_amd_video.h", "libfiasco_amd_smooth.h", "libfiasco_amd_display.h")


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


def test_header_exports_map_and_symbol_table_hold_the_six_names(product, oracle):
    src = _decls("libfiasco_amd_render.h")
    older = "".join(_decls(h) for h in OLDER)
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert patterns
    assert set(re.findall(r"\b(fiasco_\w*)\s*\(", src)) == set(NAMES) and fiasco_amd.RENDER_SYMBOLS == NAMES
    assert list(fiasco_amd._RENDER_SIGNATURES) == NAMES
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    for name in NAMES:
        assert len(re.findall(r"\b%s\s*\(" % name, src)) == 1, name                     # declared once
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        assert params.count(",") + 1 == len(fiasco_amd._RENDER_SIGNATURES[name][1]), name
        assert not re.search(r"\b%s\b" % name, older), name
        assert name not in fiasco_amd.EXPORTED_SYMBOLS + fiasco_amd.VIDEO_SYMBOLS + fiasco_amd.SMOOTH_SYMBOLS + fiasco_amd.DISPLAY_SYMBOLS, name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert getattr(product.L, name).argtypes == fiasco_amd._RENDER_SIGNATURES[name][1], name       # bound by Library.__init__
        assert not hasattr(oracle.L, name), name                                        # the oracle library has none of them
    assert not re.search(r"\bfiasco_renderer_\w+\s*\(", src)                            # the reference's names stay the reference's
    assert '#include "libfiasco_amd.h"' in src and '#include "libfiasco_amd_hip.h"' in src
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-x", "c", os.path.join(ROOT, "include", "libfiasco_amd_render.h")])
    assert [len(fiasco_amd._RENDER_SIGNATURES[n][1]) for n in NAMES] == [5, 1, 7, 6, 7, 6]
    assert [f[0] for f in fiasco_amd.DeviceSurface._fields_] == ["data", "pitch", "width", "height"]
    assert re.search(r"typedef struct fiasco_amd_device_surface\s*\{\s*void\s*\*data;\s*size_t\s+pitch;\s*unsigned width, height;\s*\}", src)


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.decode_rendered; fiasco_amd.Renderer; "
            "assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_fixture_holds_what_the_tests_rely_on():
    fx = render_ref.fixture()
    assert set(fx["renderers"]) == set(render_ref.RENDERERS) and len(fx["renderers"]) == 12
    for n, (bpp, red, green, blue, doubled) in render_ref.RENDERERS.items():
        r = fx["renderers"][n]
        assert (r["bpp"], int(r["red_mask"], 16), int(r["green_mask"], 16), int(r["blue_mask"], 16), r["double_resolution"]) == (bpp, red, green, blue, doubled)
    dec = fx["decoded"]
    assert {"carry74_a"} <= set(dec) and set(dec) & {"g130x66", "g100x70"}
    assert any(e["color"] for e in dec.values()) and any(not e["color"] for e in dec.values())
    shown = shown_ref.fixture_cases()
    for name, e in dec.items():
        assert e["stream_md5"] == shown[name]["stream_md5"] and set(e["rendered"]) == {"-1", "0", "1"}, name
        for m, rec in e["rendered"].items():
            assert set(rec["md5"]) == {"0", "-1"} and all(set(v) == set(render_ref.RENDERERS) for v in rec["md5"].values()), (name, m)
            for n, (bpp, _, _, _, doubled) in render_ref.RENDERERS.items():
                no = render_ref.refused(bpp, doubled, rec["width"], rec["height"], e["color"])
                assert (rec["md5"]["0"][n] == "refused") == no and (rec["md5"]["-1"][n] == "refused") == no, (name, m, n)
                assert no or rec["md5"]["0"][n] != rec["md5"]["-1"][n], (name, m, n)
    for kind, recs in fx["handmade"]["planes"].items():
        sizes = {(r["width"], r["height"]) for r in recs.values()}
        assert sizes == {(33, 3), (34, 2)}, kind
        for n, r in recs.items():
            bpp, _, _, _, doubled = render_ref.RENDERERS[n]
            assert (r["width"], r["height"]) == render_ref.handmade_size(bpp, doubled, kind == "color"), (kind, n)
            assert ("bytes_zlib_b64" in r) == (r["width"] == 33), (kind, n)
    assert fx["handmade"]["formula"] == render_ref.FORMULA
    assert os.path.getsize(os.path.join(render_ref.GOLDEN, "RENDERED.json")) < 64 * 1024


def test_host_loop_gives_the_references_bytes_on_the_handmade_planes(renderers):
    fx = render_ref.fixture()["handmade"]["planes"]
    for kind in ("gray", "color"):
        for n, r in renderers.items():
            rec = fx[kind][n]
            planes = render_ref.handmade(rec["width"], rec["height"], kind == "color")
            assert hashlib.md5(planes.tobytes()).hexdigest() == rec["planes_md5"], (kind, n)
            got = r.render_planes(planes)
            if "bytes_zlib_b64" in rec:         # a mismatch can be read: the first byte that differs
                want = zlib.decompress(base64.b64decode(rec["bytes_zlib_b64"]))
                diff = [k for k in range(min(len(got), len(want))) if got[k] != want[k]][:1]
                assert got == want, (kind, n, len(got), len(want), diff, got[diff[0]:diff[0] + 8].hex() if diff else None)
            assert render_ref.md5(got) == rec["md5"], (kind, n)
            assert got == render_ref.render_named(planes, n).tobytes(), (kind, n)


@pytest.fixture(scope="module")
def oracle_planes(oracle, inputs):
    """per coded fixture case: the planes the CPU oracle decodes at smoothing 0, computed once and left alone.  The oracle's
    decoder does not magnify (fiasco_amd_batch_decode_planes_magnified refuses on it): magnification 0 here, the other
    recorded magnifications through the same host loop on the device decoder's planes in tests/test_gpu_render.py"""
    out = {}
    shown = shown_ref.fixture_cases()
    for name, e in render_ref.fixture()["decoded"].items():
        b, o = shown_ref.staged(oracle, inputs, shown[name])
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == e["stream_md5"], name
        with pytest.raises(fiasco_amd.FiascoError) as refusal:
            b.decode_planes(0, magnify=-1)
        assert "does not magnify" in str(refusal.value)
        p = b.decode_planes(0)
        p.setflags(write=False)
        out[name, 0] = p
        b.free(); o.delete()
    return out


def test_host_loop_gives_the_references_bytes_on_decoded_frames(renderers, oracle_planes):
    seen = 0
    for name, e in render_ref.fixture()["decoded"].items():
        for m, rec in e["rendered"].items():
            if (name, int(m)) not in oracle_planes:
                continue
            p = oracle_planes[name, int(m)]
            assert p.shape[-2:] == (rec["height"], rec["width"]) and (p.shape[0] == 3) == e["color"], (name, m)
            planes = p if e["color"] else p[0]
            for n, r in renderers.items():
                want = rec["md5"]["0"][n]
                if want == "refused":
                    with pytest.raises(fiasco_amd.FiascoError):
                        r.render_planes(planes)
                    continue
                assert render_ref.md5(r.render_planes(planes)) == want, (name, m, n)
                seen += 1
    assert seen >= 30


def test_host_loop_clamps_where_numpy_clamps_on_full_range_planes(renderers):
    """values outside the reference's tables: the clamp is pinned by numpy, not by the reference"""
    rng = np.random.RandomState(20)
    for color in (False, True):
        planes = rng.randint(-32768, 32768, size=(3, 4, 64) if color else (4, 64)).astype(np.int16)
        flat = planes.reshape(-1)
        flat[:8] = [-32768, 32767, -2049, 2047, -2064, 2048, -1, 0]
        hit = render_ref.rgb(planes)
        assert any(v.min() < -1024 for v in hit) and any(v.max() > 1279 for v in hit)         # beyond the reference's widest table
        for n, r in renderers.items():
            assert r.render_planes(planes) == render_ref.render_named(planes, n).tobytes(), (color, n)


def test_blue_is_not_shifted(renderers):
    """one pixel, B = 255 only: XRGB8888 has it in the low byte; with the blue mask high the reference still writes it there"""
    planes = np.zeros((3, 2, 2), dtype=np.int16)
    planes[0] = -128 * 16                 # yval = 0
    planes[1] = 127 * 16                  # T_bb[127] = 225, T_bg[127] = -43 -> G clips to 0
    for n in ("xrgb8888", "xbgr8888_blue_quirk"):
        px = renderers[n].render_planes(planes)[:4]
        assert px == bytes([225, 0, 0, 0]), (n, px.hex())


SIZES = [(1, 1), (33, 3), (100, 70)]


def test_surface_size_for_all_twelve_renderers(product, renderers):
    for n, r in renderers.items():
        bpp, _, _, _, doubled = render_ref.RENDERERS[n]
        for w, h in SIZES:
            for color in (False, True):
                if render_ref.refused(bpp, doubled, w, h, color):
                    with pytest.raises(fiasco_amd.FiascoError) as e:
                        r.surface_size(w, h, color)
                    assert "fiasco_amd_renderer" in str(e.value) and ("unwritten" in str(e.value)), (n, w, h, str(e.value))
                else:
                    assert r.surface_size(w, h, color) == render_ref.surface_size(bpp, doubled, w, h), (n, w, h)
    # which of them are refused is the reference's loop counts
    assert [render_ref.refused(24, False, w, h, True) for w, h in SIZES] == [True, True, False]
    assert [render_ref.refused(24, True, w, h, True) for w, h in SIZES] == [True, True, False]
    assert [render_ref.refused(16, False, w, h, False) for w, h in SIZES] == [True, True, False]
    assert not any(render_ref.refused(16, False, w, h, True) or render_ref.refused(16, True, w, h, False) or render_ref.refused(32, d, w, h, c)
                   for w, h in SIZES for d in (False, True) for c in (False, True))
    # NULL outputs are allowed; an empty or oversized frame is not
    r = renderers["rgb565"]
    assert product.L.fiasco_amd_renderer_surface_size(r.handle, 100, 70, 0, None, None, None) == 1
    for w, h in ((0, 4), (4, 0), (16385, 2)):
        assert product.L.fiasco_amd_renderer_surface_size(r.handle, w, h, 1, None, None, None) == 0
        assert "1 .. 16384" in product.error_message()
    assert product.L.fiasco_amd_renderer_surface_size(None, 4, 4, 1, None, None, None) == 0 and "renderer" in product.error_message()


def test_renderer_new_refuses_with_a_message(product):
    for bpp in (0, 8, 15, 17, 31, 33, 64):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.Renderer(product, 0xf800, 0x7e0, 0x1f, bpp)
        assert str(e.value) == "Rendering depth of XImage must be 16, 24, or 32 bpp.", bpp       # the reference's own sentence
    bad = [(0, 0x7e0, 0x1f, 16), (0xf800, 0, 0x1f, 16), (0xf800, 0x7e0, 0, 16),          # zero
           (0xd800, 0x7e0, 0x1f, 16), (0xf800, 0x7e0, 0x15, 16),                         # not contiguous
           (0x1ff0000, 0xff00, 0xff, 32), (0xff0000, 0xff80, 0x7f, 32),                   # wider than 8 bits
           (0x1f0000, 0x7e0, 0x1f, 16), (0xff000000, 0xff00, 0xff, 24), (0x1f00000000, 0xff00, 0xff, 32)]      # outside bpp bits
    for red, green, blue, bpp in bad:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.Renderer(product, red, green, blue, bpp)
        assert "fiasco_amd_renderer_new" in str(e.value) and "one run of 1 .. 8 bits inside the %d bits" % bpp in str(e.value), (red, green, blue, bpp)
    for ok in ((0xff000000, 0xff0000, 0xff00, 32), (0x8000, 0x4000, 0x1, 16), (0xf800, 0x7e0, 0x1f, 24)):
        fiasco_amd.Renderer(product, *ok).delete()
    product.L.fiasco_amd_renderer_delete(None)


def test_refused_renders_write_nothing(product, renderers):
    L = product.L
    planes = np.zeros((3, 3, 33), dtype=np.int16)
    buf = ctypes.create_string_buffer(b"\x5a" * 4096, 4096)
    cases = [("rgb24", 1, 33, 3, "not a multiple of 4"), ("bgr24", 0, 33, 3, "not a multiple of 4"), ("rgb24_x2", 1, 33, 3, "is odd"),
             ("bgr24_x2", 0, 33, 2, "is odd"), ("rgb565", 0, 33, 3, "odd number"), ("rgb555", 0, 1, 1, "odd number"), ("xrgb8888", 1, 0, 3, "1 .. 16384")]
    for n, color, w, h, word in cases:
        assert L.fiasco_amd_renderer_render_planes(renderers[n].handle, planes.ctypes.data, color, w, h, buf) == 0, n
        assert word in product.error_message(), (n, product.error_message())
        assert buf.raw == b"\x5a" * 4096, n
    r = renderers["xrgb8888"].handle
    assert L.fiasco_amd_renderer_render_planes(r, None, 1, 33, 3, buf) == 0 and "no planes" in product.error_message()
    assert L.fiasco_amd_renderer_render_planes(r, planes.ctypes.data, 1, 33, 3, None) == 0 and "no surface" in product.error_message()
    assert L.fiasco_amd_renderer_render_planes(None, planes.ctypes.data, 1, 33, 3, buf) == 0 and "renderer" in product.error_message()
    assert buf.raw == b"\x5a" * 4096
    # an accepted one fills exactly its surface
    assert L.fiasco_amd_renderer_render_planes(r, planes.ctypes.data, 1, 33, 3, buf) == 1
    assert buf.raw[33 * 3 * 4:] == b"\x5a" * (4096 - 33 * 3 * 4) and b"\x5a" not in buf.raw[:33 * 3 * 4]
    with pytest.raises(fiasco_amd.FiascoError):
        renderers["xrgb8888"].render_planes(np.zeros((2, 4, 4), dtype=np.int16))


def test_python_side_refusals(product, inputs, renderers):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    r32, r16, r24 = renderers["xrgb8888"], renderers["rgb565"], renderers["rgb24"]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered(r32, [])                                                      # one surface per frame
    assert "0 surfaces for a batch of 1" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered(r32, [FakeArray((64, 96, 4)), FakeArray((64, 96, 4))])
    assert "2 surfaces for a batch of 1" in str(e.value)
    bad = [(r32, FakeArray((64, 96)), "is not H x W x 4"), (r32, FakeArray((64, 96, 3)), "is not H x W x 4"), (r16, FakeArray((64, 96, 4)), "is not H x W x 2"),
           (r24, FakeArray((64, 96, 3, 1)), "is not H x W x 3"), (r32, FakeArray((64, 96, 4), typestr="<u4"), "uint8"),
           (r32, FakeArray((64, 96, 4), strides=(96 * 8, 8, 1)), "strides"), (r32, FakeArray((64, 96, 4), strides=(96 * 4, 4, 2)), "strides"),
           (r32, FakeArray((64, 96, 4), strides=(-96 * 4, 4, 1)), "strides"), (r16, FakeArray((64, 96, 2), strides=(2, 128, 1)), "strides"),
           (r32, FakeArray((64, 96, 4), readonly=True), "read-only"), (r32, object(), "not in device memory")]
    for r, s, word in bad:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_rendered(r, [s])
        assert word in str(e.value), (word, str(e.value))
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.render_planes_device(product, r, FakeArray((64, 96), typestr="<i2"), s)
        assert word in str(e.value), (word, str(e.value))
    # a pitch above the row is taken from the first stride
    arr = fiasco_amd._device_surfaces([FakeArray((64, 96, 2), strides=(200, 2, 1)), None], 16)
    assert (arr[0].pitch, arr[0].width, arr[0].height, arr[0].data) == (200, 96, 64, 0x1000) and not arr[1].data
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.render_planes_device(product, r32, FakeArray((64, 96), typestr="<f4"), FakeArray((64, 96, 4)))
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.render_planes_device(product, r32, FakeArray((64, 96), typestr="<i2"), None)
    # the C entries before a device is looked for
    L = product.L
    s = fiasco_amd._device_surfaces([FakeArray((64, 96, 4))], 32)
    assert L.fiasco_amd_batch_decode_device_rendered(None, r32.handle, 0, -1, s, None) == 0 and "empty batch" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_rendered(b.handle, None, 0, -1, s, None) == 0 and "no renderer" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_rendered(b.handle, r32.handle, 0, -1, None, None) == 0 and "no surfaces" in product.error_message()
    for smoothing in (-2, 101):
        assert L.fiasco_amd_batch_decode_device_rendered(b.handle, r32.handle, 0, smoothing, s, None) == 0
        assert "smoothing out of range" in product.error_message() and "fiasco_amd_batch_decode_device_rendered" in product.error_message()
    assert L.fiasco_amd_planes_render_device(None, 0, 96, 64, r32.handle, s, None) == 0 and "no planes" in product.error_message()
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
    assert lib.calls.pop() == ("fiasco_amd_renderer_new", (0xf800, 0x7e0, 0x1f, 16, 1)) and r.handle == 1
    s = [FakeArray((128, 192, 2))]
    assert b.decode_rendered(r, s) == 1 and b.decode_rendered(r, s, magnify=-1, smoothing=0) == 1
    (n0, a0), (n1, a1) = lib.calls
    assert n0 == n1 == "fiasco_amd_batch_decode_device_rendered" and a0[:4] == (0x10, 1, 0, -1) and a1[:4] == (0x10, 1, -1, 0)
    assert (a0[4][0].width, a0[4][0].height, a0[4][0].pitch) == (192, 128, 384)
    del lib.calls[:]
    fiasco_amd.render_planes_device(lib, r, FakeArray((3, 64, 96), typestr="<i2", ptr=0x2000), s[0])
    name, a = lib.calls[0]
    assert name == "fiasco_amd_planes_render_device" and a[:5] == (0x2000, 1, 96, 64, 1)
    r.delete()
    assert lib.calls[-1] == ("fiasco_amd_renderer_delete", (1,)) and r.handle is None


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_the_device_calls_fail_loudly_without_gpu(product, inputs, renderers):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    assert b.encode() == [None]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered(renderers["xrgb8888"], [FakeArray((64, 96, 4))])
    assert "no HIP device available" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.render_planes_device(product, renderers["rgb565"], FakeArray((64, 96), typestr="<i2"), FakeArray((64, 96, 2)))
    assert "no HIP device available" in str(e.value)
    b.free(); o.delete()
