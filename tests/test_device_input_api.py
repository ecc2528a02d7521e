"""Frames that already live in device memory (fiasco_amd_batch_stage_device / _upload_device / _input_planes):
what can be checked without a GPU.  The device side is tests/test_gpu_device_input.py (-m gpu)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fiasco_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["fiasco_amd_batch_stage_device", "fiasco_amd_batch_upload_device", "fiasco_amd_batch_input_planes"]


def test_header_declares_the_entry_points_and_the_symbol_list_holds_them(product):
    src = open(os.path.join(ROOT, "include", "libfiasco_amd_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in fiasco_amd.EXPORTED_SYMBOLS
        assert hasattr(product.L, name), name
    m = re.search(r"typedef struct fiasco_amd_device_frame \{(.*?)\} fiasco_amd_device_frame;", src, flags=re.S)
    assert m, "struct fiasco_amd_device_frame"
    fields = re.findall(r"(\w+)\s*(?:,|;)", m.group(1))
    assert fields == ["data", "pitch", "plane_stride", "width", "height", "layout"]
    assert fields == [f[0] for f in fiasco_amd.DeviceFrame._fields_]
    assert re.search(r"FIASCO_AMD_GRAY8 = 0, FIASCO_AMD_RGB8_INTERLEAVED = 1, FIASCO_AMD_RGB8_PLANAR = 2", src)
    # libfiasco_amd.h stays the reference's interface
    ref = open(os.path.join(ROOT, "include", "libfiasco_amd.h")).read()
    assert "device_frame" not in ref and "stage_device" not in ref


def test_the_oracle_library_still_links_and_knows_nothing_of_device_frames(oracle):
    """oracle/ builds its library from an explicit list of the product's host files and ctypes loads it with immediate
    binding: the fixture fails if one of those files needs a function only the HIP core has.  The two entry points that
    need a device are not in it; the fetch of a frame's planes is host C and is."""
    assert oracle.core_name() == "oracle-cpu"
    assert not hasattr(oracle.L, "fiasco_amd_batch_stage_device") and not hasattr(oracle.L, "fiasco_amd_batch_upload_device")
    assert hasattr(oracle.L, "fiasco_amd_batch_input_planes")


def numpy_planes(rgb):
    """host/fa_image.c:108-110 in numpy float64, written left to right"""
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    y = ((+0.2989 * r + 0.5866 * g + 0.1145 * b - 128) * 16).astype(np.int32).astype(np.int16)
    cb = ((-0.1687 * r - 0.3312 * g + 0.5000 * b) * 16).astype(np.int32).astype(np.int16)
    cr = ((+0.5000 * r - 0.4183 * g - 0.0816 * b) * 16).astype(np.int32).astype(np.int16)
    return np.stack([y, cb, cr])


def test_numpy_form_of_the_conversion_equals_convert_planes_for_every_rgb_triple(oracle):
    """The yardstick of tests/test_gpu_device_input.py, checked where no GPU is needed: all 2^24 RGB triples as 64 PPM
    frames of 512 x 512 through the host's convert_planes() (input_planes() of a PNM-fed batch returns its output),
    against the three expressions in numpy float64.  And all 256 gray values."""
    import synth
    o = oracle.cli_options()
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8).reshape(64, 512, 512, 3)
    b = fiasco_amd.Batch(oracle, [synth.ppm_bytes(f) for f in rgb], 20.0, o)
    for k in range(64):
        got = b.input_planes(k)
        assert got.shape == (3, 512, 512) and got.dtype == np.int16
        assert np.array_equal(got, numpy_planes(rgb[k])), k
    b.free()
    gray = (np.arange(64 * 64, dtype=np.uint32) % 256).astype(np.uint8).reshape(64, 64)
    b = fiasco_amd.Batch(oracle, [synth.pgm_bytes(gray)], 20.0, o)
    assert np.array_equal(b.input_planes(0)[0], (gray.astype(np.int16) - 128) * 16)
    b.free(); o.delete()


def test_import_does_not_import_torch():
    code = "import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.from_device; assert 'torch' not in sys.modules" % ROOT
    subprocess.check_call([sys.executable, "-c", code])


class FakeArray:
    """Anything with __cuda_array_interface__ is a frame; the strides decide pitch and plane stride."""
    def __init__(self, shape, strides=None, ptr=0x1000, typestr="|u1"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": strides}


def test_strides_become_pitch_and_plane_stride():
    f = fiasco_amd._device_frames([FakeArray((64, 96)), FakeArray((64, 96), (128, 1)), FakeArray((64, 96, 3)),
                                   FakeArray((64, 96, 3), (400, 3, 1)), FakeArray((3, 64, 96), (10000, 128, 1))])
    got = [(d.layout, d.width, d.height, d.pitch, d.plane_stride) for d in f]
    assert got == [(0, 96, 64, 96, 0), (0, 96, 64, 128, 0), (1, 96, 64, 288, 0), (1, 96, 64, 400, 0), (2, 96, 64, 128, 10000)]
    for bad in (FakeArray((64, 96), (1, 64)),               # transposed
                FakeArray((64, 96), (192, 2)),              # every second column
                FakeArray((64, 96, 3), (96, 1, 6144)),      # a planar tensor permuted to H x W x 3
                FakeArray((64, 96, 4)),                     # RGBA
                FakeArray((64, 96), typestr="<f4"),
                object()):
        with pytest.raises(fiasco_amd.FiascoError):
            fiasco_amd._device_frames([bad])


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_stage_device_fails_loudly_without_gpu(product):
    """No HIP device: NULL and a message, no crash (the pointer is never looked at)."""
    o = product.cli_options()
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.Batch.from_device(product, [FakeArray((64, 96))], 20.0, o)
    assert "no HIP device available" in product.error_message()
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.Batch.from_device(product, [], 20.0, o)
    assert "No frames" in product.error_message()
    o.delete()
