"""Decoded frames as 8-bit pixels in device memory (fiasco_amd_batch_decode_device, fiasco_amd_planes_to_pixels_device):
what can be checked without a GPU.  The device side is tests/test_gpu_device_output.py (-m gpu)."""
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fiasco_amd
from conftest import GOLDEN, options_from_args
from pixels_ref import rgb_of_ints

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fiasco_amd_batch_decode_device", "fiasco_amd_planes_to_pixels_device"]


def test_header_declares_the_entry_points_and_the_symbol_list_holds_them(product):
    src = open(os.path.join(ROOT, "include", "libfiasco_amd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in fiasco_amd.EXPORTED_SYMBOLS
        assert hasattr(product.L, name), name
    m = re.search(r"typedef struct fiasco_amd_device_target \{(.*?)\} fiasco_amd_device_target;", src, flags=re.S)
    assert m, "struct fiasco_amd_device_target"
    fields = re.findall(r"(\w+)\s*(?:,|;)", m.group(1))
    assert fields == ["data", "pitch", "plane_stride", "width", "height", "layout"]
    assert fields == [f[0] for f in fiasco_amd.DeviceTarget._fields_]
    assert ctypes_layout(fiasco_amd.DeviceTarget) == ctypes_layout(fiasco_amd.DeviceFrame)
    # libfiasco_amd.h stays the reference's interface
    ref = open(os.path.join(ROOT, "include", "libfiasco_amd.h")).read()
    assert "device_target" not in ref and "decode_device" not in ref and "planes_to_pixels" not in ref


def ctypes_layout(struct):
    return [(n, getattr(struct, n).offset, getattr(struct, n).size) for n, _ in struct._fields_]


def test_the_oracle_library_still_loads_and_has_neither_symbol(oracle):
    """oracle/ compiles against fa_host.h and links the product's host files: it must not need what only the HIP core
    has (ctypes loads it with immediate binding), and the device outlets are not in it."""
    assert oracle.core_name() == "oracle-cpu"
    for name in NAMES:
        assert not hasattr(oracle.L, name), name
    assert hasattr(oracle.L, "fiasco_amd_batch_decode_plane")


def test_restatement_gives_the_references_bytes_from_the_oracles_bands(oracle, manifest, inputs):
    """The numpy restatement of color_write (tests/pixels_ref.py, the yardstick of the GPU tests) applied to the three
    bands the oracle decodes -- Y = byte, Cb = byte - 128, Cr = byte - 128; the generator asserted that no Y byte is
    clipped -- gives the bytes `dfiasco_ref -s 0 -o` wrote (tests/golden/DECODED_RGB.json)."""
    rec = json.load(open(os.path.join(GOLDEN, "DECODED_RGB.json")))["cases"]
    assert len(rec) >= 5
    for name, ent in rec.items():
        case = [c for c in manifest["cases"] if c["name"] == name][0]
        q, o = options_from_args(oracle, case["args"])
        b = fiasco_amd.Batch(oracle, [inputs.data(case["inputs"][0])], q, o)
        assert hashlib.md5(b.encode()[0]).hexdigest() == case["md5"], name
        w, h = ent["width"], ent["height"]
        y, cb, cr = (np.frombuffer(b.decode_plane(0, k, w, h), dtype=np.uint8).astype(np.int32).reshape(h, w) for k in range(3))
        b.free(); o.delete()
        assert y.min() > 0 and y.max() < 255, name
        assert hashlib.md5(rgb_of_ints(y, cb - 128, cr - 128).tobytes()).hexdigest() == ent["decoded_md5"], name


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.decode_device; "
            "fiasco_amd.planes_to_pixels_device; assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


class FakeArray:
    """Anything with __cuda_array_interface__ is a target; the strides decide pitch and plane stride."""
    def __init__(self, shape, strides=None, ptr=0x1000, typestr="|u1", readonly=False):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, readonly), "version": 3, "strides": strides}


def test_strides_become_pitch_and_plane_stride_of_targets():
    t = fiasco_amd._device_targets([FakeArray((64, 96)), FakeArray((64, 96), (128, 1)), None, FakeArray((64, 96, 3)),
                                    FakeArray((64, 96, 3), (400, 3, 1)), FakeArray((3, 64, 96), (10000, 128, 1), ptr=0x2000)])
    assert isinstance(t[0], fiasco_amd.DeviceTarget)
    got = [(d.data, d.layout, d.width, d.height, d.pitch, d.plane_stride) for d in t]
    assert got == [(0x1000, 0, 96, 64, 96, 0), (0x1000, 0, 96, 64, 128, 0), (None, 0, 0, 0, 0, 0), (0x1000, 1, 96, 64, 288, 0),
                   (0x1000, 1, 96, 64, 400, 0), (0x2000, 2, 96, 64, 128, 10000)]
    # one set of rules for frames and targets
    f = fiasco_amd._device_frames([FakeArray((3, 64, 96), (10000, 128, 1))])
    assert (f[0].layout, f[0].pitch, f[0].plane_stride) == (t[5].layout, t[5].pitch, t[5].plane_stride)
    for bad in (FakeArray((64, 96), readonly=True),
                FakeArray((64, 96), (1, 64)),               # transposed
                FakeArray((64, 96, 4)),                     # RGBA
                FakeArray((64, 96), typestr="<f4"),
                object()):
        with pytest.raises(fiasco_amd.FiascoError):
            fiasco_amd._device_targets([bad])
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd._device_targets([FakeArray((64, 96)), FakeArray((64, 96), readonly=True)])
    assert "target 1 is read-only" in str(e.value)
    fiasco_amd._device_frames([FakeArray((64, 96), readonly=True)])         # a source may be read-only


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_decode_device_fails_loudly_without_gpu(product, inputs):
    """No HIP device: 0 and the library's message, no crash (the pointers are never looked at)."""
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    assert b.encode() == [None]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_device([FakeArray((64, 96))])
    assert "no HIP device available" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_device([])                                  # one target per frame
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.planes_to_pixels_device(product, FakeArray((64, 96), typestr="<i2"), FakeArray((64, 96)))
    assert "no HIP device available" in str(e.value)
    b.free(); o.delete()
