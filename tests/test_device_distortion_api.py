"""Decoded distortion of a batch measured on the device (fiasco_amd_batch_decode_distortion_device,
fiasco_amd_planes_distortion_device): what can be checked without a GPU.  The device side is
tests/test_gpu_device_distortion.py (-m gpu)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fiasco_amd
from distortion_ref import GOLDEN_CASES, distortion_of_bytes, distortion_of_planes, legacy_mse, reference_of_batch, staged_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fiasco_amd_batch_decode_distortion_device", "fiasco_amd_planes_distortion_device"]


def test_header_declares_the_entry_points_and_the_symbol_list_holds_them(product):
    src = open(os.path.join(ROOT, "include", "libfiasco_amd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in fiasco_amd.EXPORTED_SYMBOLS
        assert hasattr(product.L, name), name
    # libfiasco_amd.h stays the reference's interface
    ref = open(os.path.join(ROOT, "include", "libfiasco_amd.h")).read()
    assert "distortion" not in ref


def test_the_oracle_library_still_loads_and_has_neither_symbol(oracle):
    """oracle/ links the product's host files: it must not need what only the HIP core has, and the device entries are
    not in it."""
    assert oracle.core_name() == "oracle-cpu"
    for name in NAMES:
        assert not hasattr(oracle.L, name), name
    assert hasattr(oracle.L, "fiasco_amd_batch_decode_psnr_all")


def test_restatement_of_small_arrays():
    a = np.array([[-32768, -2049, -2048, -2033], [-16, 0, 2031, 2032]], dtype=np.int16)
    c = np.array([[32767, -2048, -2049, -2032], [0, -1, 2047, 32767]], dtype=np.int16)
    # bytes: a = 0 0 0 0 / 127 128 254 255, c = 255 0 0 1 / 128 127 255 255
    assert distortion_of_planes(a, c) == ([255 * 255 + 1 + 1 + 1 + 1, 0, 0], [255, 0, 0])
    assert distortion_of_planes(np.stack([a, a, c]), np.stack([a, c, c])) == ([0, 255 * 255 + 4, 0], [0, 255, 0])
    assert distortion_of_bytes(np.zeros((3, 2, 2), np.uint8), np.full((3, 2, 2), 255, np.uint8)) == ([4 * 65025] * 3, [255] * 3)


def test_restatement_is_the_oracles_float_sum_below_two_to_the_24(oracle, manifest, inputs):
    """Below 2^24 every partial sum of psnr_of()'s float loop is an integer a float holds: the loop's sum is the exact
    one and its mean one float division.  The cap is a condition of the comparison and holds for every case here."""
    frames = {1: 0, 3: 0}
    for name in GOLDEN_CASES:
        b, o, out = staged_case(oracle, manifest, inputs, name)
        assert None not in out, (name, oracle.error_message())
        for i in range(b.n):
            w, h, bands = b._geom[i]
            sse, mx = reference_of_batch(b, i)
            psnr, mse = b.decode_psnr(i)
            for k in range(bands):
                assert sse[k] < 2 ** 24, (name, i, k, sse[k])
                assert legacy_mse(sse[k], w, h) == mse[k], (name, i, k, sse[k], mse[k])
                assert (mx[k] == 0) == (sse[k] == 0) and mx[k] * mx[k] <= sse[k]
            assert sse[bands:] == [0] * (3 - bands) and mse[bands:] == [0.0] * (3 - bands)
            frames[bands] += 1
        b.free(); o.delete()
    assert frames == {1: 4, 3: 3}


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.decode_distortion_device; "
            "fiasco_amd.planes_distortion_device; assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


class FakeArray:
    def __init__(self, shape, strides=None, ptr=0x1000, typestr="<i2"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


def test_planes_must_be_two_packed_int16_arrays_of_one_shape(product):
    for a, b in ((FakeArray((64, 96)), FakeArray((64, 64))),
                 (FakeArray((64, 96)), FakeArray((3, 64, 96))),
                 (FakeArray((2, 64, 96)), FakeArray((2, 64, 96))),
                 (FakeArray((64, 96), typestr="|u1"), FakeArray((64, 96), typestr="|u1")),
                 (FakeArray((64, 96), (256, 2)), FakeArray((64, 96))),
                 (object(), FakeArray((64, 96)))):
        with pytest.raises(fiasco_amd.FiascoError):
            fiasco_amd.planes_distortion_device(product, a, b)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_the_calls_fail_loudly_without_gpu(product, inputs):
    """No HIP device: 0 and the library's message, no crash (the pointers are never looked at)."""
    o = product.cli_options()
    b = fiasco_amd.Batch(product, [inputs.data("g96x64")], 20.0, o)
    assert b.encode() == [None]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_distortion_device()
    assert "no HIP device available" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_distortion_device([])                       # one target per frame
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.planes_distortion_device(product, FakeArray((64, 96)), FakeArray((64, 96)))
    assert "no HIP device available" in str(e.value)
    b.free(); o.delete()
