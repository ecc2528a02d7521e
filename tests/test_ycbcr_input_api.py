"""Frames that are YCbCr already (include/libfiasco_amd_ycbcr.h), what can be checked without a GPU, on the CPU oracle library
(the host entries are host code, which the oracle is built from): the planes of NV12, NV21, I420 and planar 4:4:4 frames
against the definition in numpy (tests/ycbcr_ref.py); the tie to the reference-pinned PNM path on the gray values on which
both agree; the round trip of the definition; a video with P and B frames; every refusal.  The kernel's body replayed on the
CPU is tests/test_ycbcr_input_step_host.py, the device side tests/test_gpu_ycbcr_input.py (-m gpu)."""
import ctypes
import os
import re
import resource
import subprocess
import sys

import numpy as np
import pytest

import fiasco_amd
import synth
import ycbcr_ref as yr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["fiasco_amd_batch_stage_ycbcr", "fiasco_amd_seq_open_ycbcr"]
DEVICE = ["fiasco_amd_batch_stage_device_ycbcr", "fiasco_amd_batch_upload_device_ycbcr", "fiasco_amd_seq_open_device_ycbcr"]


def test_header_symbol_list_and_libraries_hold_the_five_names(product, oracle):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libfiasco_amd_ycbcr.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fiasco_\w*)\s*\(", src)) == set(HOST + DEVICE) and fiasco_amd.YCBCR_SYMBOLS == HOST + DEVICE
    assert HOST + DEVICE == list(fiasco_amd._YCBCR_SIGNATURES)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    for name in HOST + DEVICE:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        assert params.count(",") + 1 == len(fiasco_amd._YCBCR_SIGNATURES[name][1]), name
        assert name not in fiasco_amd.EXPORTED_SYMBOLS + fiasco_amd.VIDEO_SYMBOLS + fiasco_amd.YUV420_SYMBOLS, name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert getattr(product.L, name).argtypes == fiasco_amd._YCBCR_SIGNATURES[name][1], name        # bound by Library.__init__
        assert hasattr(oracle.L, name) == (name in HOST), name
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-x", "c", os.path.join(ROOT, "include", "libfiasco_amd_ycbcr.h")])
    fields = re.search(r"typedef struct fiasco_amd_ycbcr_frame \{(.*?)\}", src, flags=re.S).group(1)
    want = ["y", "y_pitch", "cb", "cr", "c_pitch", "c_step", "subsampling", "width", "height"]
    assert re.findall(r"(\w+)\s*[;,]", fields) == want == [f[0] for f in fiasco_amd.YCbCrFrame._fields_]
    assert ctypes.sizeof(fiasco_amd.YCbCrFrame) == 56
    # the frame of the RGB entries keeps its layout
    assert [f[0] for f in fiasco_amd.DeviceFrame._fields_] == ["data", "pitch", "plane_stride", "width", "height", "layout"]
    assert ctypes.sizeof(fiasco_amd.DeviceFrame) == 40


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Batch.from_device_ycbcr; "
            "fiasco_amd.Sequence.from_device_ycbcr; assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


@pytest.mark.parametrize("size,pad", [((32, 32), 0), ((38, 34), 5), ((102, 66), 9)])
def test_planes_are_the_definitions(oracle, size, pad):
    """Every layout of a frame whose samples walk through every byte value: input_planes() is ycbcr_ref.planes()."""
    w, h = size
    o = oracle.cli_options()
    for s, kinds in ((1, ["nv12", "nv21", "i420"]), (0, ["444"])):
        y, cb, cr = yr.every_value(w, h, s)
        if size == (32, 32):
            assert sorted(y.ravel().tolist()) == sorted(list(range(256)) * 4)
            if s:
                assert cb.shape == (16, 16) and sorted(cb.ravel().tolist()) == sorted(cr.ravel().tolist()) == list(range(256))
                assert not np.array_equal(cb, cr)
        want = yr.planes(y, cb, cr, s)
        assert want.shape == (3, h, w) and want.dtype == np.int16
        for kind in kinds:
            frame, order = yr.layout(kind, y, cb, cr, pad)
            if pad:
                assert frame[0].strides[0] == w + pad and not frame[1].flags["C_CONTIGUOUS"]
            b = fiasco_amd.Batch.from_ycbcr(oracle, [frame], 20.0, o, order=order)
            got = b.input_planes(0)
            b.free()
            assert np.array_equal(got, want), (kind, s, int((got != want).sum()))
    o.delete()


def test_the_planes_of_the_library_go_round(oracle):
    """clip255((planes >> 4) + 128) of the planes the LIBRARY made, sampled at (2 i, 2 j), gives the source bytes back, for every
    byte value in every plane and for NV12, NV21, I420 and 4:4:4; in 4:2:0 every one of the 2 x 2 pixels holds the sample."""
    o = oracle.cli_options()
    for kind in yr.KINDS:
        s = 0 if kind == "444" else 1
        y, cb, cr = yr.every_value(32, 32, s)
        frame, order = yr.layout(kind, y, cb, cr)
        b = fiasco_amd.Batch.from_ycbcr(oracle, [frame], 20.0, o, order=order)
        p = yr.bytes_of(b.input_planes(0))
        b.free()
        step = 2 if s else 1
        assert np.array_equal(p[0], y), kind
        assert np.array_equal(p[1][::step, ::step], cb) and np.array_equal(p[2][::step, ::step], cr), kind
        if s:
            for dy in (0, 1):
                for dx in (0, 1):
                    assert np.array_equal(p[1][dy::2, dx::2], cb) and np.array_equal(p[2][dy::2, dx::2], cr), (kind, dy, dx)
    o.delete()


def test_neutral_chroma_frames_give_the_streams_of_their_gray_ppm(oracle):
    """The tie to the PNM path, which is pinned to the reference: on 242 of the 256 gray values the reader's arithmetic on
    r = g = b = v gives exactly ((v - 128) * 16, 0, 0).  An image of those values as PPM, as a 4:4:4 frame and as NV12
    (Y = v, Cb = Cr = 128) has the same planes -- asserted, or the comparison would be vacuous -- and the same stream."""
    good = yr.agreeing_values()
    assert len(good) == 242 and sorted(set(range(256)) - set(good)) == yr.EXCEPTIONS
    img = yr.onto_agreeing(synth.synth(96, 64, 21))
    assert set(np.unique(img).tolist()) <= set(good) and len(np.unique(img)) > 100
    ppm = synth.ppm_bytes(np.stack([img, img, img], axis=-1))
    full = np.full((64, 96), 128, dtype=np.uint8)
    half = np.full((32, 48), 128, dtype=np.uint8)
    want_planes = yr.planes(img, full, full, 0)
    assert not want_planes[1].any() and not want_planes[2].any()
    for o in (oracle.cli_options(), oracle.cli_options(optimize=1)):          # defaults, and -z 1
        p = fiasco_amd.Batch(oracle, [ppm], 20.0, o)
        assert np.array_equal(p.input_planes(0), want_planes)
        a = fiasco_amd.Batch.from_ycbcr(oracle, [(img, full, full)], 20.0, o)
        n = fiasco_amd.Batch.from_ycbcr(oracle, [(img, np.stack([half, half], axis=-1))], 20.0, o)
        assert np.array_equal(a.input_planes(0), want_planes) and np.array_equal(n.input_planes(0), want_planes)
        sp, sa, sn = p.encode(), a.encode(), n.encode()
        assert sp[0] is not None, oracle.error_message()
        assert sa == sp and sn == sp
        # ... and the stream does depend on the pixels: the frame upside down gives another one
        u = fiasco_amd.Batch.from_ycbcr(oracle, [(img[::-1].copy(), full, full)], 20.0, o)
        assert u.encode()[0] not in (None, sp[0])
        u.free()
        p.free(); a.free(); n.free(); o.delete()


def test_a_video_of_420_frames_is_the_video_of_its_replicated_444_frames(oracle):
    """Five frames of 64 x 48 with moving content, I, P and B frames: the stream and the reconstructed frames of the NV12 video
    are those of the same planes fed as 4:4:4 with the chroma replicated by numpy beforehand."""
    frames = yr.moving(5, 64, 48, 1)
    o = oracle.cli_options(pattern="ibbpp")
    nv12 = [yr.layout("nv12", *f)[0] for f in frames]
    up = lambda c: np.repeat(np.repeat(c, 2, axis=0), 2, axis=1)
    full = [(y, up(cb), up(cr)) for y, cb, cr in frames]
    got = []
    for fr in (nv12, full):
        seq = fiasco_amd.Sequence.from_ycbcr(oracle, fr, 20.0, o)
        assert seq.n == 5 and seq.frames == 5
        seq.keep_reconstructed()
        stream = seq.encode()
        rec = [seq.reconstructed_planes(d) for d in range(5)]
        seq.free()
        assert stream.startswith(b"FIASCO")
        assert [p.shape for p, _ in rec] == [(3, 48, 64)] * 5 and [t for _, t in rec] == [0, 2, 2, 1, 1]
        got.append((stream, rec))
    o.delete()
    assert got[0][0] == got[1][0]
    for (a, _), (b, _) in zip(got[0][1], got[1][1]):
        assert np.array_equal(a, b)
    # the frames do move: P and B frames have something to predict
    assert not np.array_equal(frames[0][0], frames[1][0])


class Raw:
    """a plane by address, shape and strides"""
    def __init__(self, ptr, shape, strides=None):
        self.__array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}


def _frame(lib, **kw):
    """one fiasco_amd_ycbcr_frame of 64 x 48 NV12 over a buffer, with fields replaced"""
    buf = np.full(64 * 48 * 3, 128, dtype=np.uint8)
    f = fiasco_amd.YCbCrFrame()
    f.y, f.cb, f.cr = buf.ctypes.data, buf.ctypes.data + 64 * 48, buf.ctypes.data + 64 * 48 + 1
    f.c_step, f.subsampling, f.width, f.height = 2, 1, 64, 48
    for k, v in kw.items():
        setattr(f, k, v)
    return f, buf


def test_refusals_by_message_and_nothing_leaks(oracle):
    o = oracle.cli_options()
    L = oracle.L
    cases = [
        (dict(y=None), "no Y plane"), (dict(cb=None), "no Cb plane"), (dict(cr=None), "no Cr plane"),
        (dict(c_step=0), "c_step 0"), (dict(c_step=3), "c_step 3"),
        (dict(subsampling=2), "subsampling 2"),
        (dict(subsampling=0), "c_step 2 with subsampling 0"),
        (dict(cr_off=2), "not one byte apart"),
        (dict(width=30), "Width of image"), (dict(height=30), "Height of image"), (dict(width=66, height=47), "even numbers"),
        (dict(width=8194), "too large"),
        (dict(y_pitch=63), "Y pitch of 63 bytes is smaller than a row"),
        (dict(c_pitch=63), "chroma pitch of 63 bytes is smaller than a row"),
    ]

    def refused():
        for kw, msg in cases:
            kw = dict(kw)
            off = kw.pop("cr_off", None)
            f, buf = _frame(oracle, **kw)
            if off is not None:
                f.cr = f.cb + off
            arr = (fiasco_amd.YCbCrFrame * 2)()
            good, buf2 = _frame(oracle)
            arr[0], arr[1] = good, f
            assert not L.fiasco_amd_batch_stage_ycbcr(2, arr, ctypes.c_float(20.0), o.handle)
            assert msg in oracle.error_message(), (msg, oracle.error_message())
            assert "<YCbCr frame 1>" in oracle.error_message() or msg == "even numbers"      # the PNM reader's message names no image
            assert not L.fiasco_amd_seq_open_ycbcr(2, arr, ctypes.c_float(20.0), o.handle, 0, 1)
            assert msg in oracle.error_message(), (msg, oracle.error_message())
        good, buf = _frame(oracle)
        arr = (fiasco_amd.YCbCrFrame * 1)(good)
        assert not L.fiasco_amd_batch_stage_ycbcr(0, arr, ctypes.c_float(20.0), o.handle) and "No frames" in oracle.error_message()
        assert not L.fiasco_amd_batch_stage_ycbcr(1, None, ctypes.c_float(20.0), o.handle) and "No frames" in oracle.error_message()
        assert not L.fiasco_amd_batch_stage_ycbcr(1, arr, ctypes.c_float(0.0), o.handle) and "quality" in oracle.error_message()
        assert not L.fiasco_amd_seq_open_ycbcr(0, arr, ctypes.c_float(20.0), o.handle, 0, 1) and "No frames" in oracle.error_message()
        assert not L.fiasco_amd_seq_open_ycbcr(1, arr, ctypes.c_float(20.0), o.handle, 1, 1) and "rank" in oracle.error_message()
        # frames of a video have one size
        a, keep_a = _frame(oracle)
        b, keep_b = _frame(oracle, height=46)            # the frames are converted before the sizes are compared
        two = (fiasco_amd.YCbCrFrame * 2)(a, b)
        assert not L.fiasco_amd_seq_open_ycbcr(2, two, ctypes.c_float(20.0), o.handle, 0, 1) and "same size" in oracle.error_message()
        del keep_a, keep_b

    refused()
    # what the binding itself refuses: a chroma shape that is neither full nor half size, a plane that is no byte array
    y = np.zeros((48, 64), dtype=np.uint8)
    for frame, msg in [((y, np.zeros((24, 31), np.uint8), np.zeros((24, 31), np.uint8)), "chroma planes"),
                       ((y, np.zeros((24, 32), np.uint8), np.zeros((48, 64), np.uint8)), "chroma planes"),
                       ((y, np.zeros((24, 32, 3), np.uint8)), "cannot be described by a pitch"),
                       ((y, np.zeros((48, 64, 2), np.uint8)), "interleaved chroma plane"),
                       ((y, np.zeros((24, 32), np.int16), np.zeros((24, 32), np.int16)), "not bytes"),
                       ((y,), "expected, not 1 arrays"),
                       ((y, y[::2, ::2], y[::2, ::2]), "cannot be described by a pitch")]:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.Batch.from_ycbcr(oracle, [frame], 20.0, o)
        assert msg in str(e.value), (msg, str(e.value))
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.Batch.from_ycbcr(oracle, [(y, np.zeros((24, 32, 2), np.uint8))], 20.0, o, order="nv16")
    assert "nv12" in str(e.value)
    # free and re-stage, refusals in between: 50 rounds of a 256 x 256 frame (384 KiB of planes a batch) leave the peak
    # resident size where the first rounds put it -- 50 leaked batches would add 19 MiB
    big = yr.layout("nv12", *yr.textured(256, 256, 1))[0]

    def round_():
        refused()
        b = fiasco_amd.Batch.from_ycbcr(oracle, [big], 20.0, o)
        assert b.input_planes(0).shape == (3, 256, 256)
        b.free()
        s = fiasco_amd.Sequence.from_ycbcr(oracle, [big, big], 20.0, o)
        s.free()

    for _ in range(3):
        round_()
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    for _ in range(50):
        round_()
    grown = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - before
    assert grown < 6 * 1024, "peak resident size grew by %d KiB over 50 rounds" % grown
    o.delete()
