"""Magnified decodes (`dfiasco -m M'; include/libfiasco_amd_hip.h: fiasco_amd_magnified_size,
fiasco_amd_batch_decode_device_magnified, fiasco_amd_batch_decode_planes_magnified,
fiasco_amd_batch_decode_device_thumbnails), what can be checked without a GPU: the size rule against what the real
reference did (tests/golden/DECODED_MAGNIFIED.json), the symbol lists, the refusals of the host route on the CPU oracle
library -- whose decoder does not magnify and says so --, the refusals of the wrappers.  The device side is
tests/test_gpu_magnify.py (-m gpu)."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

import fiasco_amd
import magnify_ref
from conftest import options_from_args

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_NAMES = ["fiasco_amd_magnified_size", "fiasco_amd_batch_decode_planes_magnified"]
DEVICE_NAMES = ["fiasco_amd_batch_decode_device_magnified", "fiasco_amd_batch_decode_device_thumbnails"]


def limit_of(message):
    m = re.search(r"(Minimum|Maximum) value is (-?\d+)\.$", message)
    assert m, message
    return m.group(1).lower(), int(m.group(2))


def test_fixture_holds_what_the_tests_rely_on():
    cases = magnify_ref.fixture_cases()
    assert {"g64x32", "g100x70", "g130x66", "c256", "c100x70", "c192x144", "c256sq", "g64x64_a", "g64x64_b"} <= set(cases)
    for name, e in cases.items():
        assert set(e["magnified"]) == {str(m) for m in magnify_ref.MAGS}, name
        zero = e["magnified"]["0"]
        assert (zero["width"], zero["height"]) == (e["width"], e["height"]), name
        assert all(r["md5"] != zero["md5"] for m, r in magnify_ref.accepted(e) if m), name
        assert magnify_ref.refused(e) or "md5" in e["magnified"]["3"], name
    assert not [m for m, _ in magnify_ref.accepted(cases["g64x32"]) if m < 0]                  # no reduction allowed
    assert (cases["g100x70"]["magnified"]["-1"]["width"], cases["g100x70"]["magnified"]["-1"]["height"]) == (50, 36)
    assert (cases["g130x66"]["magnified"]["-1"]["width"], cases["g130x66"]["magnified"]["-1"]["height"]) == (66, 34)
    assert "md5" in cases["c192x144"]["magnified"]["-2"] and "refused" in cases["c192x144"]["magnified"]["-3"]
    assert len(magnify_ref.accepted(cases["c256sq"])) == 7
    assert cases["g64x64_a"]["stream_md5"] != cases["g64x64_b"]["stream_md5"]


@pytest.mark.parametrize("which", ["product", "oracle"])
def test_size_rule_gives_every_size_and_refusal_of_the_reference(which, request):
    lib = request.getfixturevalue(which)                       # host code: the same in both libraries
    for name, e in magnify_ref.fixture_cases().items():
        for m, r in magnify_ref.accepted(e):
            assert fiasco_amd.magnified_size(lib, e["width"], e["height"], m) == (r["width"], r["height"]), (name, m)
        for m, r in magnify_ref.refused(e):
            with pytest.raises(fiasco_amd.FiascoError) as err:
                fiasco_amd.magnified_size(lib, e["width"], e["height"], m)
            assert limit_of(str(err.value)) == (r["refused"], r["limit"]), (name, m)
            assert "%d x %d" % (e["width"], e["height"]) in str(err.value)


def test_size_rule_at_its_edges(oracle):
    size = lambda w, h, m: fiasco_amd.magnified_size(oracle, w, h, m)
    # 2048 x 2048 pixels is allowed, one more step is not (codec/dfiasco.c:111: >)
    assert size(1024, 1024, 1) == (2048, 2048)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        size(1024, 1024, 2)
    assert limit_of(str(e.value)) == ("maximum", 1)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        size(1026, 1024, 1)
    assert limit_of(str(e.value)) == ("maximum", 0)
    # a side of exactly 32 is allowed, 31 is not: 64 -> 32, 62 -> 31
    assert size(64, 64, -1) == (32, 32) and size(66, 64, -1) == (34, 32)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        size(64, 62, -1)
    assert limit_of(str(e.value)) == ("minimum", 0)
    # a frame smaller than 32 fails the reference's n = 0 step for every reduction, and is shown as it is
    with pytest.raises(fiasco_amd.FiascoError):
        size(30, 64, -1)
    assert size(30, 64, 0) == (30, 64) and size(30, 64, 1) == (60, 128)
    # far out of range in both directions, and no frame
    for m in (-2147483648, -31, 31, 2147483647):
        with pytest.raises(fiasco_amd.FiascoError):
            size(256, 256, m)
    with pytest.raises(fiasco_amd.FiascoError):
        size(0, 64, 0)
    # NULL outputs: the verdict alone
    f = oracle.L.fiasco_amd_magnified_size
    f.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint)]
    assert f(256, 256, -3, None, None) == 1 and f(256, 256, -4, None, None) == 0


def test_headers_symbol_list_exports_map_and_libraries_agree(product, oracle):
    hip = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libfiasco_amd_hip.h")).read(), flags=re.S)
    ref = open(os.path.join(ROOT, "include", "libfiasco_amd.h")).read()
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert patterns
    for name in HOST_NAMES + DEVICE_NAMES:
        assert re.search(r"\b%s\s*\(" % name, hip), name
        assert name not in ref, name                               # libfiasco_amd.h stays the reference's interface
        assert name in fiasco_amd.EXPORTED_SYMBOLS, name
        assert hasattr(product.L, name), name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
    for name in HOST_NAMES:
        assert hasattr(oracle.L, name), name                       # host code: in both libraries
    for name in DEVICE_NAMES:
        assert not hasattr(oracle.L, name), name                   # the device outlets are the HIP core's
    for doc in ("INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in HOST_NAMES + DEVICE_NAMES:
            assert name in text, (doc, name)


def staged(lib, inputs, ent):
    q, o = options_from_args(lib, ent["args"])
    return fiasco_amd.Batch(lib, [magnify_ref.case_input(inputs, ent)], q, o), o


def test_host_route_on_the_oracle(oracle, inputs):
    """The oracle's decoder does not know fa_dec_job.magnify: magnify = 0 is fiasco_amd_batch_decode_planes(), every
    other value the size rule accepts is refused with the backend message, and what the rule refuses is refused by it."""
    ent = magnify_ref.fixture_cases()["g100x70"]
    b, o = staged(oracle, inputs, ent)
    f = oracle.L.fiasco_amd_batch_decode_planes_magnified
    f.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_int, ctypes.c_void_p]
    f.restype = ctypes.c_int
    pattern = np.full((1, 140, 200), 0x5a5a, dtype=np.int16)
    buf = pattern.copy()
    # no batch, no finished pass
    assert f(None, 0, 0, buf.ctypes.data) == 0 and "no finished automaton" in oracle.error_message()
    assert f(b.handle, 0, 0, buf.ctypes.data) == 0 and "no finished automaton" in oracle.error_message()
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_planes(0, magnify=1)
    stream = b.encode()[0]
    assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"]
    # index out of range, no room
    assert f(b.handle, 1, 0, buf.ctypes.data) == 0 and "frame 1" in oracle.error_message()
    assert f(b.handle, 0, 0, None) == 0
    # magnify = 0: the old call's planes
    plain = b.decode_planes(0)
    assert plain.shape == (1, 70, 100) and np.array_equal(b.decode_planes(0, magnify=0), plain)
    small = np.zeros((1, 70, 100), dtype=np.int16)
    assert f(b.handle, 0, 0, small.ctypes.data) == 1 and np.array_equal(small, plain)
    # accepted by the rule, not by this backend: refused, nothing written
    for m in (1, -1, 3):
        assert f(b.handle, 0, m, buf.ctypes.data) == 0
        msg = oracle.error_message()
        assert "does not magnify" in msg and "oracle-cpu" in msg, msg
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_planes(0, magnify=m)
        assert "does not magnify" in str(e.value)
    # refused by the rule
    assert f(b.handle, 0, -2, buf.ctypes.data) == 0 and "Minimum value is -1." in oracle.error_message()
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_planes(0, magnify=-2)
    assert "Minimum value is -1." in str(e.value)
    assert np.array_equal(buf, pattern)
    b.free(); o.delete()


class FakeArray:
    def __init__(self, shape, ptr=0x1000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": None}


def test_device_entries_refuse_before_they_need_a_device(product, inputs):
    """What the product's device entries hold against their own arguments comes before any HIP call."""
    L = product.L
    fm, ft = L.fiasco_amd_batch_decode_device_magnified, L.fiasco_amd_batch_decode_device_thumbnails
    fm.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(fiasco_amd.DeviceTarget), ctypes.c_void_p]
    ft.argtypes = [ctypes.c_void_p, ctypes.POINTER(fiasco_amd.DeviceTarget), ctypes.c_uint, ctypes.POINTER(fiasco_amd.DeviceTarget), ctypes.c_void_p]
    one = fiasco_amd._device_targets([FakeArray((32, 64))])
    assert fm(None, 1, one, None) == 0 and "fiasco_amd_batch_decode_device_magnified: empty batch" in product.error_message()
    assert ft(None, None, 1, one, None) == 0 and "fiasco_amd_batch_decode_device_thumbnails: empty batch" in product.error_message()
    ent = magnify_ref.fixture_cases()["g64x64_a"]
    b, o = staged(product, inputs, ent)
    assert fm(b.handle, 1, None, None) == 0 and "no targets" in product.error_message()
    assert ft(b.handle, one, 1, None, None) == 0 and "no thumbnails" in product.error_message()
    assert ft(b.handle, one, 0, one, None) == 0 and "reduction of at least 1" in product.error_message()
    # the wrappers: one target and one thumb per frame, reduce >= 1
    t = FakeArray((64, 64))
    for bad in (lambda: b.decode_device([], magnify=1), lambda: b.decode_device([t, t], magnify=-1),
                lambda: b.decode_thumbnails([t], 1, []), lambda: b.decode_thumbnails([t], 1, [t, t]),
                lambda: b.decode_thumbnails([t, t], 1, [t]), lambda: b.decode_thumbnails([], 1, [t]),
                lambda: b.decode_thumbnails([t], 0, [t]), lambda: b.decode_thumbnails(None, 0, [t]),
                lambda: b.decode_thumbnails(None, -1, [t])):
        with pytest.raises(fiasco_amd.FiascoError):
            bad()
    b.free(); o.delete()
