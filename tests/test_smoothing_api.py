"""The reference's border smoothing (smooth_image, codec/decoder.c:674-768; `dfiasco -s N'), what can be checked without
a GPU: the border list of fiasco_amd_batch_smoothing_borders() and the numpy restatement of the pair update
(tests/smooth_ref.py), applied to the oracle's decoded planes, give the bytes the real reference wrote
(tests/golden/DECODED_SMOOTH.json); the list is well formed; its order matters where that was measured; the refusals;
the symbol lists.  Everything here is host code: it runs on the CPU oracle library."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

import fiasco_amd
import smooth_ref
from conftest import GOLDEN, options_from_args
from pixels_ref import pixels_of_planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_NAMES = ["fiasco_amd_batch_smoothing_borders", "fiasco_amd_batch_decode_planes"]
LEVELS = (1, 35, 70, 100)


def fixture_cases():
    return json.load(open(os.path.join(GOLDEN, "DECODED_SMOOTH.json")))["cases"]


def staged(lib, inputs, ent):
    """a fixture case as a finished batch of one frame -> (batch, options, stream)"""
    q, o = options_from_args(lib, ent["args"])
    o.set_smoothing(ent["smoothing"])
    b = fiasco_amd.Batch(lib, [smooth_ref.case_input(inputs, ent)], q, o)
    return b, o, b.encode()[0]


@pytest.fixture(scope="module")
def decoded(oracle, inputs):
    """per fixture case: the oracle's unsmoothed planes and the border list, computed once and left alone"""
    out = {}
    for name, ent in fixture_cases().items():
        b, o, stream = staged(oracle, inputs, ent)
        assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], name
        planes, borders = b.decode_planes(0), b.smoothing_borders(0)
        b.free(); o.delete()
        planes.setflags(write=False)
        out[name] = (ent, planes, borders)
    return out


def pixel_md5(planes):
    return hashlib.md5(pixels_of_planes(planes[0] if planes.shape[0] == 1 else planes).tobytes()).hexdigest()


def test_fixture_holds_what_the_tests_rely_on():
    cases = fixture_cases()
    assert {"carry48_a", "carry74_a", "g100x70", "g64x32", "c256"} <= set(cases)
    assert any(e["smoothing"] != 70 and not e["color"] for e in cases.values())
    for name, e in cases.items():
        m = e["decoded_md5"]
        assert set(m) == {"-1", "0", "1", "35", "70", "100"}, name
        assert all(m[str(n)] != m["0"] for n in LEVELS), name
        assert m["-1"] == m[str(e["smoothing"])], name
        if e["smoothing"] != 70:
            assert m["-1"] != m["70"], name


def test_factors_are_the_references():
    assert smooth_ref.factors(1) == (509, 3) and smooth_ref.factors(70) == (333, 179) and smooth_ref.factors(100) == (256, 256)
    assert smooth_ref.factors(0) is None


def test_list_and_restatement_give_the_references_bytes(decoded):
    for name, (ent, planes, borders) in decoded.items():
        assert planes.shape == ((3 if ent["color"] else 1), ent["height"], ent["width"]), name
        assert pixel_md5(planes) == ent["decoded_md5"]["0"], name
        for n in LEVELS:
            assert pixel_md5(smooth_ref.smooth_planes(planes, borders, n)) == ent["decoded_md5"][str(n)], (name, n)


def test_list_is_well_formed(decoded):
    for name, (ent, planes, borders) in decoded.items():
        w, h = ent["width"], ent["height"]
        passes = [b[4] for b in borders]
        assert passes == sorted(passes) and passes[0] == 0 and set(passes) == set(range(passes[-1] + 1)), name
        level_of = {}
        for x, y, n, level, p in borders:
            assert level_of.setdefault(p, level) == level, (name, p)
            assert n >= 1 and n <= (1 << (level >> 1) if level & 1 else 1 << ((level + 1) >> 1)), (name, x, y, n, level)
            if level & 1:
                assert 1 <= y < h and x + n <= w, (name, x, y, n, level)
            else:
                assert 1 <= x < w and y + n <= h, (name, x, y, n, level)
        for p in set(passes):
            seen = np.zeros((h, w), dtype=bool)
            for x, y, n, level, _ in (b for b in borders if b[4] == p):
                region = seen[y - 1:y + 1, x:x + n] if level & 1 else seen[y:y + n, x - 1:x + 1]
                assert region.shape == ((2, n) if level & 1 else (n, 2)) and not region.any(), (name, p, x, y)
                region[:] = True
        levels = [level_of[p] for p in sorted(level_of)]
        drops = [k for k in range(1, len(levels)) if levels[k] <= levels[k - 1]]
        if ent["color"]:
            assert len(drops) == 1, (name, levels)               # Y by ascending level, then Cb from a low level again
        else:
            assert not drops, (name, levels)
        if (w & (w - 1)) or (h & (h - 1)):                       # a ragged frame clips a border
            assert any(n < (1 << (level >> 1) if level & 1 else 1 << ((level + 1) >> 1)) for _, _, n, level, _ in borders), name


def test_order_matters_where_it_was_measured(decoded):
    """Y and Cb borders of one level in one pass (sorted by level alone, stable) give other bytes than the reference."""
    for name, n in (("carry48_a", 70), ("carry48_a", 100), ("carry74_a", 70)):
        ent, planes, borders = decoded[name]
        merged = sorted(borders, key=lambda b: b[3])
        assert merged != borders
        assert pixel_md5(smooth_ref.smooth_planes(planes, merged, n)) != ent["decoded_md5"][str(n)], (name, n)


def test_refusals_of_the_host_calls(oracle, inputs):
    ent = fixture_cases()["g64x32"]
    q, o = options_from_args(oracle, ent["args"])
    b = fiasco_amd.Batch(oracle, [inputs.data(ent["input"])], q, o)
    L = oracle.L
    fb, fp = L.fiasco_amd_batch_smoothing_borders, L.fiasco_amd_batch_decode_planes
    fb.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.POINTER(fiasco_amd.Border), ctypes.c_uint]
    fp.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]
    buf = np.zeros((32, 64), dtype=np.int16)
    some = (fiasco_amd.Border * 4096)()
    # no batch, no finished pass
    assert fb(None, 0, some, 4096) == 0 and "no finished automaton" in oracle.error_message()
    assert fp(None, 0, buf.ctypes.data) == 0 and "no finished automaton" in oracle.error_message()
    assert fb(b.handle, 0, some, 4096) == 0 and "no finished automaton" in oracle.error_message()
    assert fp(b.handle, 0, buf.ctypes.data) == 0 and "no finished automaton" in oracle.error_message()
    with pytest.raises(fiasco_amd.FiascoError):
        b.smoothing_borders(0)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_planes(0)
    assert b.encode()[0] is not None
    # index out of range, no room
    assert fb(b.handle, 1, some, 4096) == 0 and "frame 1" in oracle.error_message()
    assert fp(b.handle, 1, buf.ctypes.data) == 0 and "frame 1" in oracle.error_message()
    assert fp(b.handle, 0, None) == 0
    n = fb(b.handle, 0, None, 0)
    assert n > 1 and fb(b.handle, 0, some, n) == n
    assert fb(b.handle, 0, some, n - 1) == 0 and "more than %d borders" % (n - 1) in oracle.error_message()
    assert len(b.smoothing_borders(0)) == n
    assert not buf.any() and fp(b.handle, 0, buf.ctypes.data) == 1 and buf.any()
    b.free(); o.delete()


def test_headers_symbol_list_and_exports_map_agree(product, oracle):
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libfiasco_amd.h")).read(), flags=re.S)
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert patterns
    for name in HOST_NAMES:
        assert re.search(r"\b%s\s*\(" % name, host), name
        assert name in fiasco_amd.EXPORTED_SYMBOLS
        assert hasattr(product.L, name) and hasattr(oracle.L, name), name           # host code: in both libraries
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
    m = re.search(r"typedef struct fiasco_amd_border \{(.*?)\} fiasco_amd_border;", host, flags=re.S)
    assert m and re.findall(r"(\w+)\s*(?:,|;)", m.group(1)) == ["x", "y", "len", "level", "pass"]
    assert ctypes.sizeof(fiasco_amd.Border) == 8
    assert [(n, getattr(fiasco_amd.Border, n).offset) for n, _ in fiasco_amd.Border._fields_] == \
        [("x", 0), ("y", 2), ("len", 4), ("level", 6), ("pass_", 7)]

