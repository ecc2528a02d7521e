"""Magnified frames and thumbnails smoothed as `dfiasco' shows them (include/libfiasco_amd_display.h), what can be checked
without a GPU: the names in their header, the exports map and their symbol table; the border list of a magnified frame
(fiasco_amd_batch_smoothing_borders_magnified, host code: on the CPU oracle library) against a numpy derivation from the
coded list for every case of tests/golden/DECODED_SHOWN.json at every magnification the reference accepts; that it lies
inside the plane shown, that its passes ascend from 0 with one level each and that the borders of a pass share no pixel;
the refusal of a frame with a state that falls below level 1, on a coded frame and on a synthetic automaton
(tests/shown_wfa_check.c); the size rule's refusals; the wrapper's refusals; the policy fiasco_amd_smooth_fused().  The
fused kernel's body replayed on the CPU is tests/test_shown_step_host.py, the device side tests/test_gpu_shown.py
(-m gpu)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

import fiasco_amd
import shown_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["fiasco_amd_batch_smoothing_borders_magnified"]
DEVICE = ["fiasco_amd_batch_decode_device_shown", "fiasco_amd_batch_decode_device_thumbnails_shown",
          "fiasco_amd_smooth_planes_device_fused", "fiasco_amd_smooth_fused"]
NAMES = HOST + DEVICE


class FakeArray:
    def __init__(self, shape, typestr="|u1", ptr=0x1000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": None}


def _decls(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


def test_header_exports_map_and_symbol_table_hold_the_five_names(product, oracle):
    src = _decls("libfiasco_amd_display.h")
    older = "".join(_decls(h) for h in ("libfiasco_amd.h", "libfiasco_amd_hip.h", "libfiasco_amd_video.h", "libfiasco_amd_smooth.h"))
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert patterns
    assert set(re.findall(r"\b(fiasco_\w*)\s*\(", src)) == set(NAMES) and fiasco_amd.DISPLAY_SYMBOLS == NAMES
    assert list(fiasco_amd._DISPLAY_SIGNATURES) == NAMES
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        assert params.count(",") + 1 == len(fiasco_amd._DISPLAY_SIGNATURES[name][1]), name
        assert not re.search(r"\b%s\s*\(" % name, older), name       # declared once
        assert name not in fiasco_amd.EXPORTED_SYMBOLS + fiasco_amd.VIDEO_SYMBOLS + fiasco_amd.SMOOTH_SYMBOLS, name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert hasattr(product.L, name), name
        assert getattr(product.L, name).argtypes == fiasco_amd._DISPLAY_SIGNATURES[name][1], name      # bound by Library.__init__
        assert hasattr(oracle.L, name) == (name in HOST), name      # the list is host code; the rest is the device's
    assert '#include "libfiasco_amd.h"' in src and '#include "libfiasco_amd_hip.h"' in src
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-x", "c", os.path.join(ROOT, "include", "libfiasco_amd_display.h")])
    assert re.search(r"fiasco_amd_batch_decode_device_shown\s*\(\s*const fiasco_amd_batch_t \*\w+,\s*int magnify,\s*int smoothing,", src)
    assert re.search(r"fiasco_amd_batch_decode_device_thumbnails_shown\s*\(\s*const fiasco_amd_batch_t \*\w+,\s*int smoothing,\s*"
                     r"const fiasco_amd_device_target \*targets,\s*unsigned reduce,", src)
    assert re.search(r"fiasco_amd_batch_smoothing_borders_magnified\s*\(\s*const fiasco_amd_batch_t \*\w+,\s*unsigned i,\s*int magnify,", src)
    assert [len(fiasco_amd._DISPLAY_SIGNATURES[n][1]) for n in NAMES] == [5, 5, 6, 7, 2]
    # the fused step has the signature of its per-pass sibling
    assert fiasco_amd._DISPLAY_SIGNATURES["fiasco_amd_smooth_planes_device_fused"] == fiasco_amd._SMOOTH_SIGNATURES["fiasco_amd_smooth_planes_device"]


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.decode_shown; "
            "assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


# ------------------------------------------------------------------ the lists

@pytest.fixture(scope="module")
def lists(oracle, inputs):
    """per fixture case: the coded list and the library's answer at every magnification from -3 to 3 -- a list or the
    refusal's message --, computed once on the oracle library and left alone"""
    out = {}
    for name, ent in shown_ref.fixture_cases().items():
        b, o = shown_ref.staged(oracle, inputs, ent)
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], name
        coded = b.smoothing_borders(0)
        at = {}
        for m in range(-3, 4):
            try:
                at[m] = b.smoothing_borders(0, magnify=m)
            except fiasco_amd.FiascoError as e:
                at[m] = str(e)
        b.free(); o.delete()
        out[name] = (ent, coded, at)
    return out


def test_fixture_holds_what_the_tests_rely_on():
    cases = shown_ref.fixture_cases()
    assert {"g256", "g256_q60", "c256sq", "c256", "g100x70", "g130x66", "carry74_a", "noise256", "g256_z1_q300"} <= set(cases)
    assert any(e["smoothing"] == 35 for e in cases.values())
    assert sorted(n for n, e in cases.items() if "3" in e["shown"]) == ["carry74_a", "g100x70"] and cases["carry74_a"]["color"]
    assert any(e["color"] and "md5" in e["shown"]["-3"] for e in cases.values())
    assert (cases["g100x70"]["shown"]["-1"]["width"], cases["g100x70"]["shown"]["-1"]["height"]) == (50, 36)
    assert (cases["g130x66"]["shown"]["-1"]["width"], cases["g130x66"]["shown"]["-1"]["height"]) == (66, 34)
    for name, e in cases.items():
        assert max(e["width"], e["height"]) <= 256, name
        for m, r in shown_ref.accepted(e):
            assert set(r["md5"]) == {"-1", "0", "35", "70"}, (name, m)
            assert all(r["md5"][str(n)] != r["md5"]["0"] for n in shown_ref.LEVELS), (name, m)
            assert r["md5"]["-1"] == r["md5"][str(e["smoothing"])], (name, m)
        assert (e["smoothing"] == 70) or all(r["md5"]["-1"] != r["md5"]["70"] for _, r in shown_ref.accepted(e)), name


def test_magnified_list_is_the_coded_list_shifted(lists):
    seen = 0
    for name, (ent, coded, at) in lists.items():
        assert at[0] == coded, name                                     # magnify = 0: smoothing_borders() itself
        for m, rec in shown_ref.accepted(ent):
            want = shown_ref.magnified_borders(coded, m, rec["width"], rec["height"])
            if (name, m) in shown_ref.LIBRARY_REFUSES:
                assert want is None and isinstance(at[m], str), (name, m)
                continue
            assert want is not None and at[m] == want, (name, m, at[m] if isinstance(at[m], str) else None)
            seen += 1
    assert seen >= 45
    # the ragged sizes clip a border at the size rounded up to even
    for name in ("g100x70", "g130x66"):
        ent, coded, at = lists[name]
        assert any(n < shown_ref.side(level) for _, _, n, level, _ in at[-1]), name
    # a list loses borders when the levels fall: level 7 -> 1 at -3
    ent, coded, at = lists["g256_q60"]
    assert min(b[3] for b in coded) == 7 and min(b[3] for b in at[-3]) == 1 and len(at[-3]) == len(coded)
    assert max(b[3] for b in at[2]) == max(b[3] for b in coded) + 4


def test_magnified_list_is_well_formed(lists):
    for name, (ent, coded, at) in lists.items():
        for m, rec in shown_ref.accepted(ent):
            if isinstance(at[m], str):
                continue
            w, h, borders = rec["width"], rec["height"], at[m]
            passes = [b[4] for b in borders]
            assert passes == sorted(passes) and passes[0] == 0 and set(passes) == set(range(passes[-1] + 1)), (name, m)
            level_of = {}
            for x, y, n, level, p in borders:
                assert level_of.setdefault(p, level) == level and level >= 1, (name, m, p)
                assert 1 <= n <= shown_ref.side(level), (name, m, x, y, n, level)
                if level & 1:
                    assert 1 <= y < h and x + n <= w, (name, m, x, y, n, level)
                else:
                    assert 1 <= x < w and y + n <= h, (name, m, x, y, n, level)
            shown_ref.pixels_touched(borders, w, h)                     # asserts: the borders of one pass share no pixel
            levels = [level_of[p] for p in sorted(level_of)]
            drops = [k for k in range(1, len(levels)) if levels[k] <= levels[k - 1]]
            assert len(drops) == (1 if ent["color"] else 0), (name, m, levels)


def test_refusal_of_a_state_that_falls_below_level_one(lists):
    ent, coded, at = lists["g256_z1_q300"]
    assert min(b[3] for b in coded) == 5
    msg = at[-3]
    assert isinstance(msg, str) and "fiasco_amd_batch_smoothing_borders_magnified: frame 0" in msg, msg
    assert "magnification -3" in msg and "level 5 falls to level -1" in msg and "reference's own result is undefined" in msg, msg
    assert isinstance(at[-2], list) and min(b[3] for b in at[-2]) == 1          # level 5 -> 1: accepted
    # no other case is refused where the reference decodes
    for name, (ent, coded, at) in lists.items():
        for m, _ in shown_ref.accepted(ent):
            assert isinstance(at[m], list) or (name, m) in shown_ref.LIBRARY_REFUSES, (name, m, at[m])


def test_size_rule_refuses_with_its_own_message(lists):
    for name, (ent, coded, at) in lists.items():
        for m, rec in shown_ref.refused(ent):
            assert isinstance(at[m], str), (name, m)
            word = "Minimum" if rec["refused"] == "minimum" else "Maximum"
            assert "%s value is %d." % (word, rec["limit"]) in at[m], (name, m, at[m])
    assert sum(len(shown_ref.refused(ent)) for ent, _, _ in lists.values()) >= 9


def test_synthetic_automaton_with_its_low_state_at_the_origin(oracle, tmp_path):
    """tests/shown_wfa_check.c builds automata by hand and calls fa_smoothing_borders_magnified() of the host code: a state
    of level 2 whose second half begins at (1, 0) lands on (0, 0) with level 0 at -1 -- where smooth_image would read the
    word before the plane -- and refuses the frame; out of sight it does not."""
    exe = str(tmp_path / "shown_wfa_check")
    lib = os.path.join(ROOT, "oracle")
    subprocess.check_call(["gcc", "-std=gnu99", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "fiasco_amd", "csrc", "host"),
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "shown_wfa_check.c"),
                           "-L" + lib, "-loracle_fiasco", "-Wl,-rpath," + lib, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "shown_wfa_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ------------------------------------------------------------------ the wrapper and the entries before a device is looked for

def test_refusals_that_come_before_the_device_is_looked_for(product, inputs):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    t = [FakeArray((64, 96))]
    for bad in (-2, 101, 1000):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_shown(t, magnify=1, smoothing=bad)
        assert "smoothing out of range" in str(e.value) and "fiasco_amd_batch_decode_device_shown" in str(e.value)
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_thumbnails(None, 1, [FakeArray((32, 48))], smoothing=bad)
        assert "smoothing out of range" in str(e.value) and "fiasco_amd_batch_decode_device_thumbnails_shown" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_shown([])                                              # one target per frame
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_thumbnails(None, 0, [FakeArray((32, 48))], smoothing=70)
    assert "reduce = 0" in str(e.value)
    # decode_device keeps refusing the pair, and says where to go
    for magnify in (1, -1):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_device(t, magnify=magnify, smoothing=70)
        assert "smoothing and magnify" in str(e.value) and "decode_shown" in str(e.value)
    L = product.L
    assert L.fiasco_amd_batch_decode_device_shown(None, 0, 70, None, None) == 0 and "empty batch" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_shown(b.handle, 1, 70, None, None) == 0 and "no targets" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_thumbnails_shown(b.handle, 70, None, 1, None, None) == 0 and "no thumbnails" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_thumbnails_shown(b.handle, 70, None, 16, fiasco_amd._device_targets(t), None) == 0
    assert "reduction out of range" in product.error_message()
    # the list of a batch without a finished pass; the fused step's argument checks are its sibling's
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.smoothing_borders(0, magnify=-1)
    assert "no finished automaton" in str(e.value)
    planes = FakeArray((64, 96), typestr="<i2")
    for bad in (-1, 101):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.smooth_planes_device(product, planes, [(8, 4, 4, 5, 0)], bad, fused=True)
        assert "0 .. 100" in str(e.value) and "fiasco_amd_smooth_planes_device_fused" in str(e.value)
    assert L.fiasco_amd_smooth_planes_device_fused(None, 96, 64, None, 0, 70, None) == 0 and "no plane" in product.error_message()
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
    t, th = [FakeArray((64, 96))], [FakeArray((32, 48))]
    assert b.decode_shown(t) == 1 and b.decode_shown(t, magnify=-1, smoothing=35) == 1
    (n0, a0), (n1, a1) = lib.calls
    assert n0 == n1 == "fiasco_amd_batch_decode_device_shown" and a0[:3] == (0x10, 0, -1) and a1[:3] == (0x10, -1, 35)
    del lib.calls[:]
    assert b.decode_thumbnails(t, 1, th) == 1 and b.decode_thumbnails(t, 1, th, smoothing=0) == 1
    assert [c[0] for c in lib.calls] == ["fiasco_amd_batch_decode_device_thumbnails"] * 2 and all(len(c[1]) == 5 for c in lib.calls)
    del lib.calls[:]
    assert b.decode_thumbnails(t, 1, th, smoothing=-1) == 1
    name, a = lib.calls[0]
    assert name == "fiasco_amd_batch_decode_device_thumbnails_shown" and a[:2] == (0x10, -1) and a[3] == 1 and len(a) == 6
    del lib.calls[:]
    b.smoothing_borders(0), b.smoothing_borders(0, magnify=2)
    assert [c[0] for c in lib.calls] == ["fiasco_amd_batch_smoothing_borders"] * 2 + ["fiasco_amd_batch_smoothing_borders_magnified"] * 2
    assert lib.calls[2][1][:3] == (0x10, 0, 2)
    del lib.calls[:]
    planes = FakeArray((64, 96), typestr="<i2")
    fiasco_amd.smooth_planes_device(lib, planes, [(8, 4, 4, 5, 0)], 35)
    fiasco_amd.smooth_planes_device(lib, planes, [(8, 4, 4, 5, 0)], 35, fused=True)
    assert [c[0] for c in lib.calls] == ["fiasco_amd_smooth_planes_device", "fiasco_amd_smooth_planes_device_fused"]
    assert lib.calls[0][1][:3] == lib.calls[1][1][:3] == (0x1000, 96, 64) and lib.calls[1][1][4:6] == (1, 35)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_the_calls_fail_loudly_without_gpu(product, inputs):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    assert b.encode() == [None]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_shown([FakeArray((128, 192))], magnify=1)
    assert "no HIP device available" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_thumbnails([FakeArray((64, 96))], 1, [FakeArray((32, 48))], smoothing=70)
    assert "no HIP device available" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.smooth_planes_device(product, FakeArray((64, 96), typestr="<i2"), [(8, 4, 4, 5, 0)], 70, fused=True)
    assert "no HIP device available" in str(e.value)
    b.free(); o.delete()


# ------------------------------------------------------------------ the policy

def test_fused_policy_is_monotone_and_false_above_the_recorded_threshold(product):
    """fiasco_amd_smooth_fused(pairs, passes): once false it stays false as the pairs grow; the threshold is the one
    profiles/shown_device.json records with the measurements it came from; a plane without passes has no launch."""
    f = product.L.fiasco_amd_smooth_fused
    rec = json.load(open(os.path.join(ROOT, "profiles", "shown_device.json")))
    limit = rec["threshold_pairs"]
    assert isinstance(limit, int) and limit >= 0
    for passes in (1, 2, 15, 40, 256):
        answers = [f(p, passes) for p in list(range(0, 70000, 97)) + [limit, limit + 1, 1 << 20, 1 << 40]]
        assert set(answers) <= {0, 1}
        assert answers[:-4] == sorted(answers[:-4], reverse=True), passes         # monotone: never true again after a false
        assert f(limit + 1, passes) == 0 and f(1 << 20, passes) == 0 and f(1 << 40, passes) == 0
        assert f(limit, passes) == (1 if limit else 0)
        assert all(f(p, passes) == 1 for p in (1, limit // 2, limit)) or not limit
    assert f(100, 0) == 0
    # the measured rows say what the threshold says: fused faster by more than the spread at and below it
    rows = sorted(rec["sweep"], key=lambda r: r["pairs"])
    wins = [r["pairs"] for r in rows if r["fused_wins"]]
    assert limit == (max(wins) if wins else 0)
