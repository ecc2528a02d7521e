"""Decoded frames smoothed along their partition borders on the device (fiasco_amd_batch_decode_device_smoothed,
fiasco_amd_batch_decode_distortion_device_smoothed, fiasco_amd_smooth_planes_device; csrc/hip/smooth.inc): what can be
checked without a GPU -- the names in their header (include/libfiasco_amd_smooth.h), the exports map and their symbol
list; the refusals that come before the device is looked for; the loud failure without a device; that the Python
defaults still call the unsmoothed entry points.  The step itself replayed on the CPU is tests/test_smooth_step_host.py, the device side
tests/test_gpu_smoothing_device.py (-m gpu)."""
import os
import re
import subprocess
import sys

import pytest

import fiasco_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fiasco_amd_batch_decode_device_smoothed", "fiasco_amd_batch_decode_distortion_device_smoothed",
         "fiasco_amd_smooth_planes_device"]


class FakeArray:
    def __init__(self, shape, typestr="|u1", ptr=0x1000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": None}


def _decls(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


def test_header_exports_map_and_symbol_list_hold_the_three_names(product, oracle):
    """The three entries live in a header of their own, include/libfiasco_amd_smooth.h, and in a symbol list of their
    own, fiasco_amd.SMOOTH_SYMBOLS, as the video entries do: tests/test_host_api.py pins the functions of
    libfiasco_amd.h + libfiasco_amd_hip.h and EXPORTED_SYMBOLS to each other as a closed set, so a name added to either
    would fail it.  Header, symbol list, parameter counts, exports map and the dynamic symbols agree."""
    src = _decls("libfiasco_amd_smooth.h")
    older = _decls("libfiasco_amd.h") + _decls("libfiasco_amd_hip.h") + _decls("libfiasco_amd_video.h")
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    assert patterns
    assert set(re.findall(r"\b(fiasco_\w*)\s*\(", src)) == set(NAMES) and fiasco_amd.SMOOTH_SYMBOLS == NAMES
    assert list(fiasco_amd._SMOOTH_SIGNATURES) == NAMES
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        assert params.count(",") + 1 == len(fiasco_amd._SMOOTH_SIGNATURES[name][1]), name
        assert not re.search(r"\b%s\s*\(" % name, older), name       # declared once
        assert name not in fiasco_amd.EXPORTED_SYMBOLS and name not in fiasco_amd.VIDEO_SYMBOLS, name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert hasattr(product.L, name), name
        assert getattr(product.L, name).argtypes == fiasco_amd._SMOOTH_SIGNATURES[name][1], name      # bound by Library.__init__
        assert not hasattr(oracle.L, name), name                    # device entries: not in the CPU oracle
    # the header includes the two it builds on and compiles on its own as C
    assert '#include "libfiasco_amd.h"' in src and '#include "libfiasco_amd_hip.h"' in src
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-x", "c", os.path.join(ROOT, "include", "libfiasco_amd_smooth.h")])
    # the signatures as the header spells them: smoothing is the second argument of the two batch entries
    assert re.search(r"fiasco_amd_batch_decode_device_smoothed\s*\(\s*const fiasco_amd_batch_t \*\w+,\s*int smoothing,", src)
    assert re.search(r"fiasco_amd_batch_decode_distortion_device_smoothed\s*\(\s*const fiasco_amd_batch_t \*\w+,\s*int smoothing,", src)
    assert re.search(r"fiasco_amd_smooth_planes_device\s*\(\s*int16_t \*\w+,\s*unsigned width,\s*unsigned height,\s*"
                     r"const fiasco_amd_border \*\w+,\s*unsigned n,\s*int smoothing,\s*void \*stream\)", src)
    assert [len(fiasco_amd._SMOOTH_SIGNATURES[n][1]) for n in NAMES] == [4, 6, 7]


def test_the_job_field_is_the_last_of_its_struct():
    """oracle/ is built against fa_host.h and fills fa_dec_job by name: a new field goes to the end"""
    src = open(os.path.join(ROOT, "fiasco_amd", "csrc", "host", "fa_host.h")).read()
    body = re.search(r"typedef struct fa_dec_job \{(.*?)\} fa_dec_job;", src, flags=re.S).group(1)
    fields = re.findall(r"(\w+)\s*(?:\[\d+\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields[-1] == "smoothing" and fields.index("magnify") < fields.index("smoothing")


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.smooth_planes_device; "
            "assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


def test_refusals_that_come_before_the_device_is_looked_for(product, inputs):
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    t = [FakeArray((64, 96))]
    for bad in (-2, 101, 1000):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_device(t, smoothing=bad)
        assert "smoothing out of range" in str(e.value) and "fiasco_amd_batch_decode_device_smoothed" in str(e.value)
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_distortion_device(smoothing=bad)
        assert "smoothing out of range" in str(e.value) and "fiasco_amd_batch_decode_distortion_device_smoothed" in str(e.value)
    for magnify in (1, -1):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_device(t, magnify=magnify, smoothing=70)
        assert "smoothing and magnify" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_device([], smoothing=70)                           # one target per frame
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_distortion_device([], smoothing=70)
    # the C entries themselves: no batch, no targets
    L = product.L
    assert L.fiasco_amd_batch_decode_device_smoothed(None, 70, None, None) == 0 and "empty batch" in product.error_message()
    assert L.fiasco_amd_batch_decode_device_smoothed(b.handle, 70, None, None) == 0 and "no targets" in product.error_message()
    assert L.fiasco_amd_batch_decode_distortion_device_smoothed(b.handle, 70, None, None, None, None) == 0
    assert "no result arrays and no targets" in product.error_message()
    # the step alone
    planes = FakeArray((64, 96), typestr="<i2")
    for bad in (-1, 101):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.smooth_planes_device(product, planes, [(8, 4, 4, 5, 0)], bad)
        assert "0 .. 100" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.smooth_planes_device(product, FakeArray((9000, 96), typestr="<i2"), [], 70)
    assert "1 .. 8192" in str(e.value)
    assert L.fiasco_amd_smooth_planes_device(None, 96, 64, None, 0, 70, None) == 0 and "no plane" in product.error_message()
    assert L.fiasco_amd_smooth_planes_device(0x1000, 96, 64, None, 3, 70, None) == 0 and "no borders" in product.error_message()
    for wrong in (FakeArray((64, 96)), FakeArray((2, 64, 96), typestr="<i2"), object()):
        with pytest.raises(fiasco_amd.FiascoError):
            fiasco_amd.smooth_planes_device(product, wrong, [], 70)
    b.free(); o.delete()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_the_calls_fail_loudly_without_gpu(product, inputs):
    """No HIP device: 0 and the library's message, no crash (the pointers are never looked at)."""
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    assert b.encode() == [None]
    for smoothing in (-1, 1, 70, 100):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_device([FakeArray((64, 96))], smoothing=smoothing)
        assert "no HIP device available" in str(e.value)
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_distortion_device(smoothing=smoothing)
        assert "no HIP device available" in str(e.value)
    for smoothing in (0, 70):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.smooth_planes_device(product, FakeArray((64, 96), typestr="<i2"), [(8, 4, 4, 5, 0)], smoothing)
        assert "no HIP device available" in str(e.value)
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


def test_python_defaults_call_the_unsmoothed_entry_points():
    lib = Recorder()
    b = fiasco_amd.Batch.__new__(fiasco_amd.Batch)
    b.lib, b.handle, b.n, b._keep, b._geom = lib, 0x10, 1, None, [(96, 64, 1)]
    t = [FakeArray((64, 96))]
    assert b.decode_device(t) == 1 and b.decode_device(t, smoothing=0) == 1 and b.decode_device(t, None, 0) == 1
    assert [c[0] for c in lib.calls] == ["fiasco_amd_batch_decode_device"] * 3 and all(len(c[1]) == 3 for c in lib.calls)
    del lib.calls[:]
    assert b.decode_device(t, magnify=1) == 1
    assert lib.calls[0][0] == "fiasco_amd_batch_decode_device_magnified" and lib.calls[0][1][1] == 1
    del lib.calls[:]
    assert b.decode_distortion_device()[0] == 1 and b.decode_distortion_device(t, smoothing=0)[0] == 1
    assert [c[0] for c in lib.calls] == ["fiasco_amd_batch_decode_distortion_device"] * 2 and all(len(c[1]) == 5 for c in lib.calls)
    del lib.calls[:]
    for n in (-1, 1, 70, 100):
        assert b.decode_device(t, smoothing=n) == 1 and b.decode_distortion_device(smoothing=n)[0] == 1
        (first, a), (second, c) = lib.calls[-2:]
        assert first == "fiasco_amd_batch_decode_device_smoothed" and a[0] == 0x10 and a[1] == n and len(a) == 4
        assert second == "fiasco_amd_batch_decode_distortion_device_smoothed" and c[0] == 0x10 and c[1] == n and len(c) == 6
    del lib.calls[:]
    fiasco_amd.smooth_planes_device(lib, FakeArray((64, 96), typestr="<i2"), [(8, 4, 4, 5, 0), (4, 8, 8, 6, 1)], 35)
    name, a = lib.calls[0]
    assert name == "fiasco_amd_smooth_planes_device" and a[:3] == (0x1000, 96, 64) and a[4:6] == (2, 35)
    assert [(x.x, x.y, x.len, x.level, x.pass_) for x in a[3][:2]] == [(8, 4, 4, 5, 0), (4, 8, 8, 6, 1)]
