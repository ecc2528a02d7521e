"""Frames that are YCbCr already, in device memory (include/libfiasco_amd_ycbcr.h: fiasco_amd_batch_stage_device_ycbcr,
_upload_device_ycbcr, fiasco_amd_seq_open_device_ycbcr; csrc/hip/input_convert_ycbcr.inc), on the device: the planes of the
conversion kernel against the definition in numpy (tests/ycbcr_ref.py) and against the host entry, the streams against the CPU
oracle's, the loop decode_420 -> from_device_ycbcr, the hand-over of replacement frames with the caller's stream in between, a
video, and every refusal.  Everything is compared exactly.  The frames are torch tensors."""
import ctypes
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    # before the product library is loaded: torch brings the HIP runtime both then share
    import torch

import fiasco_amd
import synth
import ycbcr_ref as yr
from conftest import options_from_args

pytestmark = pytest.mark.gpu

MIXED = ["nv12", "nv21", "i420", "444", "nv12"]         # the layouts of the five sizes of ycbcr_ref.SIZES in one batch
PADS = [0, 5, 0, 9, 3]


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def five(make):
    """the five sizes, layouts mixed: -> (frames on the host, the same on the device, orders, (y, cb, cr, s) per frame)"""
    host, dev, orders, src = [], [], [], []
    for (w, h), kind, pad in zip(yr.SIZES, MIXED, PADS):
        s = 0 if kind == "444" else 1
        y, cb, cr = make(w, h, s)
        fh, order = yr.layout(kind, y, cb, cr, pad)
        fd, _ = yr.layout(kind, y, cb, cr, pad, put=to_gpu)
        host.append(fh); dev.append(fd); orders.append(order); src.append((y, cb, cr, s))
    return host, dev, orders, src


def test_planes_on_the_device_are_the_definitions(gpu):
    """Frames of five sizes and four layouts, some with pitches above their rows, whose samples walk through every byte value,
    in ONE batch -- one launch walks frames of different sizes and kinds: input_planes() is ycbcr_ref.planes() and what the
    host entry of the same library gives for the same bytes."""
    o = gpu.cli_options()
    host, dev, orders, src = five(yr.every_value)
    assert any(not f[0].is_contiguous() for f in dev)
    d = fiasco_amd.Batch.from_device_ycbcr(gpu, dev, 20.0, o, order=orders)
    h = fiasco_amd.Batch.from_ycbcr(gpu, host, 20.0, o, order=orders)
    for i, (y, cb, cr, s) in enumerate(src):
        want = yr.planes(y, cb, cr, s)
        got = d.input_planes(i)
        assert got.shape == want.shape and got.dtype == np.int16
        assert np.array_equal(got, want), (i, MIXED[i], int((got != want).sum()))
        assert np.array_equal(h.input_planes(i), want), i
    d.free(); h.free(); o.delete()


def test_strided_sources_are_read_in_place(gpu):
    """A Y view cut out of a larger tensor at an odd column, a cbcr view with a pitch of its own, I420 planes that are slices of
    one allocation: the same planes and the same streams as their contiguous copies."""
    o = gpu.cli_options()
    w, h = 102, 66
    y, cb, cr = yr.textured(w, h, 1)
    cw, ch = w // 2, h // 2
    big = torch.full((h + 9, w + 40), 3, dtype=torch.uint8, device="cuda")
    big[5:5 + h, 33:33 + w] = to_gpu(y)
    bigc = torch.full((ch + 3, cw + 6, 2), 4, dtype=torch.uint8, device="cuda")
    bigc[2:2 + ch, 1:1 + cw] = to_gpu(np.stack([cb, cr], axis=-1))
    yv, cv = big[5:5 + h, 33:33 + w], bigc[2:2 + ch, 1:1 + cw]
    assert yv.data_ptr() % 2 == 1 and yv.stride(0) == w + 40 and cv.stride(0) == 2 * (cw + 6) and not cv.is_contiguous()
    flat = torch.empty(1 + w * h + 2 * cw * ch, dtype=torch.uint8, device="cuda")
    flat[1:1 + w * h] = to_gpu(y).reshape(-1)
    flat[1 + w * h:1 + w * h + cw * ch] = to_gpu(cb).reshape(-1)
    flat[1 + w * h + cw * ch:] = to_gpu(cr).reshape(-1)
    i420 = (flat[1:1 + w * h].view(h, w), flat[1 + w * h:1 + w * h + cw * ch].view(ch, cw), flat[1 + w * h + cw * ch:].view(ch, cw))
    assert i420[0].data_ptr() % 2 == 1 and i420[1].data_ptr() - i420[0].data_ptr() == w * h
    want_planes = yr.planes(y, cb, cr, 1)
    streams = []
    for frame in ((yv, cv), (to_gpu(y), cv), (yv, to_gpu(np.stack([cb, cr], axis=-1))), i420):
        got = fiasco_amd.Batch.from_device_ycbcr(gpu, [frame], 20.0, o)
        ref = fiasco_amd.Batch.from_device_ycbcr(gpu, [tuple(t.contiguous().clone() for t in frame)], 20.0, o)
        assert np.array_equal(got.input_planes(0), want_planes) and np.array_equal(ref.input_planes(0), want_planes)
        a, b = got.encode(), ref.encode()
        assert a[0] is not None and a == b, gpu.error_message()
        streams.append(a[0])
        got.free(); ref.free()
    assert len(set(streams)) == 1
    o.delete()


@pytest.mark.parametrize("args", [[], ["--dictionary-size", "64"], ["--prediction"]])
def test_streams_are_the_oracles(gpu, oracle, args):
    """The five sizes with textured chroma, layouts mixed, at quality 20 and `cfiasco' defaults and under two option variants
    of the manifest's cases: the device-fed batch of the product writes the streams the host-fed batch of the CPU oracle
    writes."""
    host, dev, orders, _ = five(lambda w, h, s: yr.textured(w, h, s))
    q, og = options_from_args(gpu, args)
    _, oo = options_from_args(oracle, args)
    assert q == 20.0
    want = fiasco_amd.Batch.from_ycbcr(oracle, host, q, oo, order=orders)
    sw = want.encode()
    assert None not in sw, oracle.error_message()
    got = fiasco_amd.Batch.from_device_ycbcr(gpu, dev, q, og, order=orders)
    sg = got.encode()
    assert sg == sw, gpu.error_message()
    want.free(); got.free(); og.delete(); oo.delete()


def test_neutral_chroma_frames_give_the_streams_of_their_gray_ppm_on_the_device(gpu):
    """The tie of tests/test_ycbcr_input_api.py on the device: an image of gray values on which the PNM reader gives exactly
    ((v - 128) * 16, 0, 0), as 4:4:4 and as NV12 with Cb = Cr = 128 in device memory, against encode_batch of its PPM."""
    o = gpu.cli_options()
    img = yr.onto_agreeing(synth.synth(96, 64, 21))
    ppm = synth.ppm_bytes(np.stack([img, img, img], axis=-1))
    want = gpu.encode_batch([ppm], 20.0, o)
    assert want[0] is not None, gpu.error_message()
    full = to_gpu(np.full((64, 96), 128, dtype=np.uint8))
    pairs = to_gpu(np.full((32, 48, 2), 128, dtype=np.uint8))
    p = fiasco_amd.Batch(gpu, [ppm], 20.0, o)
    for frame in ((to_gpu(img), full, full), (to_gpu(img), pairs)):
        b = fiasco_amd.Batch.from_device_ycbcr(gpu, [frame], 20.0, o)
        assert np.array_equal(b.input_planes(0), p.input_planes(0))
        assert b.encode() == want
        b.free()
    p.free(); o.delete()


def test_decoded_420_buffers_go_straight_back_in(gpu):
    """The loop the feature closes: a 160 x 120 colour still from PPM, decoded in 4:2:0 into (y, cbcr) tensors, staged from
    there: the planes are the definition's of the decoded bytes, the second encode succeeds and its decoded frames are
    measured against those planes on the device."""
    o = gpu.cli_options()
    first = fiasco_amd.Batch(gpu, [synth.ppm_bytes(synth.synth_color_k(160, 120))], 20.0, o)
    assert first.encode()[0] is not None, gpu.error_message()
    y = torch.zeros((120, 160), dtype=torch.uint8, device="cuda")
    cbcr = torch.zeros((60, 80, 2), dtype=torch.uint8, device="cuda")
    assert first.decode_420([(y, cbcr)]) == 1, gpu.error_message()
    second = fiasco_amd.Batch.from_device_ycbcr(gpu, [(y, cbcr)], 20.0, o)
    yh, ch = y.cpu().numpy(), cbcr.cpu().numpy()
    assert len(np.unique(yh)) > 50 and len(np.unique(ch)) > 4          # a picture was decoded
    want = yr.planes(yh, ch[:, :, 0].copy(), ch[:, :, 1].copy(), 1)
    assert np.array_equal(second.input_planes(0), want)
    y.zero_(); cbcr.zero_()                                            # the planes were converted: the source is the caller's again
    out = second.encode()
    assert out[0] is not None, gpu.error_message()
    good, sse, mx, psnr = second.decode_distortion_device()
    assert good == 1 and all(isinstance(v, int) and v >= 0 for v in sse[0] + mx[0])
    assert sum(sse[0]) > 0 and max(mx[0]) > 0 and max(mx[0]) < 256          # a second generation is not the first
    assert np.array_equal(second.input_planes(0), want)
    first.free(); second.free(); o.delete()


def nv12_set(shifts, w=96, h=64):
    return [yr.textured(w, h, 1, shift=k) for k in shifts]


def pairs_of(frames):
    """-> (Y [n, h, w], CbCr [n, h / 2, w / 2, 2]) of a list of (y, cb, cr)"""
    return np.stack([f[0] for f in frames]), np.stack([np.stack([f[1], f[2]], axis=-1) for f in frames])


def test_upload_device_ycbcr_replaces_inputs(gpu):
    """test_upload_device_replaces_inputs of tests/test_gpu_device_input.py with NV12 frames: pass after pass, pipelined, from
    a side stream that fills the tensors just before the call and scribbles over them just after, mixed with upload() and
    upload_device()."""
    o = gpu.cli_options()
    sets = [nv12_set(range(3 + 9 * k, 12 + 9 * k)) for k in range(3)]             # shifts 3 .. 29
    want = []
    for s in sets:
        hb = fiasco_amd.Batch.from_ycbcr(gpu, [yr.layout("nv12", *f)[0] for f in s], 20.0, o)
        want.append(hb.encode())
        hb.free()
    assert all(None not in w for w in want) and want[0] != want[1] != want[2]
    rgb = [synth.synth_color_k(96, 64, 1234, k) for k in range(13, 22)]
    ppm = [synth.ppm_bytes(a) for a in rgb]
    want_rgb = gpu.encode_batch(ppm, 20.0, o)
    assert None not in want_rgb
    pinned = [tuple(torch.from_numpy(a).pin_memory() for a in pairs_of(s)) for s in sets]
    side = torch.cuda.Stream()
    by = torch.zeros((9, 64, 96), dtype=torch.uint8, device="cuda")
    bc = torch.zeros((9, 32, 48, 2), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def frames():
        return [(by[i], bc[i]) for i in range(9)]

    def upload(b, k, stream=None):
        """set k through the two buffers on the side stream: filled just before the call, scribbled over just after"""
        with torch.cuda.stream(side):
            by.copy_(pinned[k][0], non_blocking=True); bc.copy_(pinned[k][1], non_blocking=True)
            b.upload_device_ycbcr(frames(), stream=stream)
            by.fill_(0); bc.fill_(0)

    with torch.cuda.stream(side):
        by.copy_(pinned[0][0], non_blocking=True); bc.copy_(pinned[0][1], non_blocking=True)
        b = fiasco_amd.Batch.from_device_ycbcr(gpu, frames(), 20.0, o)
        by.fill_(0); bc.fill_(0)
    assert b.encode() == want[0]
    upload(b, 1)
    assert b.encode() == want[1]
    # pipelined: the frames of pass i + 1 are handed over while pass i is in flight
    b.submit()
    upload(b, 2, stream=side.cuda_stream)
    assert b.collect(resubmit=True) == want[1]
    upload(b, 0)
    assert b.collect(resubmit=True) == want[2]
    assert b.collect() == want[0]
    # mixed: PNM upload, YCbCr upload, RGB upload from device memory, YCbCr upload
    b.submit()
    b.upload(ppm)
    assert b.collect(resubmit=True) == want[0]
    upload(b, 2)
    assert b.collect(resubmit=True) == want_rgb
    b.upload_device(list(to_gpu(np.stack(rgb))))
    assert b.collect(resubmit=True) == want[2]
    upload(b, 1)
    assert b.collect(resubmit=True) == want_rgb
    assert b.collect() == want[1]
    assert np.array_equal(b.input_planes(3), yr.planes(*sets[1][3], 1))
    # a batch staged from PNM takes YCbCr frames
    p = fiasco_amd.Batch(gpu, ppm, 20.0, o)
    p.submit()
    upload(p, 1)
    assert p.collect(resubmit=True) == want_rgb
    assert p.collect() == want[1]
    torch.cuda.synchronize()
    p.free(); b.free(); o.delete()


def test_several_shares_convert_their_own_ycbcr_frames(gpu):
    """set_devices([0, 0]): two shares on one GPU, nine NV12 frames dealt round robin, staged and replaced from device memory:
    every share converts the frames it is dealt.  Same streams as with one share."""
    o = gpu.cli_options()
    A, B = nv12_set(range(3, 12)), nv12_set(range(13, 22))
    want = []
    for s in (A, B):
        hb = fiasco_amd.Batch.from_ycbcr(gpu, [yr.layout("nv12", *f)[0] for f in s], 20.0, o)
        want.append(hb.encode())
        hb.free()
    assert None not in want[0] + want[1]
    dev = [[yr.layout("nv12", *f, put=to_gpu)[0] for f in s] for s in (A, B)]
    gpu.set_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        b = fiasco_amd.Batch.from_device_ycbcr(gpu, dev[0], 20.0, o)
        assert b.encode() == want[0], gpu.error_message()
        for i in (0, 1, 8):
            assert np.array_equal(b.input_planes(i), yr.planes(*A[i], 1))
        b.submit()
        b.upload_device_ycbcr(dev[1])
        assert b.collect(resubmit=True) == want[0]
        assert np.array_equal(b.input_planes(4), yr.planes(*B[4], 1))
        b.upload_device_ycbcr(dev[0])
        assert b.collect(resubmit=True) == want[1]
        assert b.collect() == want[0]
        b.free()
    finally:
        gpu.set_devices([])
        o.delete()


def test_a_video_from_device_memory(gpu, oracle):
    """Five NV12 frames of 64 x 48 with moving content, I, B and P frames: the stream is the oracle's of the same bytes on the
    host; with outputs set every frame is written and the sum of squared differences of frame 0 is that of the measuring
    kernel on its reconstructed and original planes."""
    frames = yr.moving(5, 64, 48, 1)
    og, oo = gpu.cli_options(pattern="ibbpp"), oracle.cli_options(pattern="ibbpp")
    so = fiasco_amd.Sequence.from_ycbcr(oracle, [yr.layout("nv12", *f)[0] for f in frames], 20.0, oo)
    want = so.encode()
    so.free(); oo.delete()
    # the host entry of the HIP library: the planes are lent to the searches from host memory
    sh = fiasco_amd.Sequence.from_ycbcr(gpu, [yr.layout("nv12", *f)[0] for f in frames], 20.0, og)
    assert sh.encode() == want, gpu.error_message()
    sh.free()
    dev = [yr.layout("nv12", *f, put=to_gpu)[0] for f in frames]
    seq = fiasco_amd.Sequence.from_device_ycbcr(gpu, dev, 20.0, og)
    for yv, cv in dev:
        yv.zero_(); cv.zero_()                          # right after open, in stream order: the planes were converted before
    targets = [torch.full((48, 64, 3), 7, dtype=torch.uint8, device="cuda") for _ in range(5)]
    seq.set_outputs(targets, distortion=True)
    seq.keep_reconstructed()
    got = seq.encode()
    assert got == want, gpu.error_message()
    sse, mx, written = seq.distortion()
    assert written.tolist() == [1] * 5
    rec, ftype = seq.reconstructed_planes(0)
    assert ftype == 0 and rec.shape == (3, 48, 64)
    s0, m0 = fiasco_amd.planes_distortion_device(gpu, to_gpu(rec), to_gpu(yr.planes(*frames[0], 1)))
    assert sse[0].tolist() == s0 and mx[0].tolist() == m0 and sum(s0) > 0
    assert all(int(t.min()) != 7 or int(t.max()) != 7 for t in targets)
    seq.free(); og.delete()


class Raw:
    def __init__(self, ptr, shape, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}


def test_refusals_leave_the_batch_as_it_was(gpu):
    o = gpu.cli_options()
    L = gpu.L
    src = nv12_set(range(3, 6))
    good = [yr.layout("nv12", *f, put=to_gpu)[0] for f in src]
    b = fiasco_amd.Batch.from_device_ycbcr(gpu, good, 20.0, o)
    want = b.encode()
    assert None not in want, gpu.error_message()
    hosty = np.zeros((64, 96), dtype=np.uint8)
    hostc = np.zeros((32, 48, 2), dtype=np.uint8)
    y1, c1 = good[1]

    def struct(**kw):
        f = fiasco_amd.YCbCrFrame()
        f.y, f.cb, f.cr = y1.data_ptr(), c1.data_ptr(), c1.data_ptr() + 1
        f.c_step, f.subsampling, f.width, f.height = 2, 1, 96, 64
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def arr_with(f):
        base = fiasco_amd._ycbcr_frames(good, "nv12", "__cuda_array_interface__")
        a = (fiasco_amd.YCbCrFrame * 3)(base[0], f, base[2])
        return a

    raw = [
        (struct(y=hosty.ctypes.data), "Y plane is not in device memory"),
        (struct(cb=hostc.ctypes.data, cr=hostc.ctypes.data + 1), "chroma plane is not in device memory"),
        (struct(y_pitch=95), "Y pitch of 95 bytes is smaller than a row"),
        (struct(c_pitch=95), "chroma pitch of 95 bytes is smaller than a row"),
        (struct(c_step=3), "c_step 3"),
        (struct(cr=c1.data_ptr() + 2), "not one byte apart"),
        (struct(subsampling=0), "c_step 2 with subsampling 0"),
        (struct(subsampling=2), "subsampling 2"),
        (struct(y=None), "no Y plane"), (struct(cb=None), "no Cb plane"), (struct(cr=None), "no Cr plane"),
        (struct(width=64), "size and colour model"),
        (struct(width=30), "Width of image"), (struct(height=63), "even numbers"),
    ]
    for f, msg in raw:
        assert not L.fiasco_amd_batch_upload_device_ycbcr(b.handle, arr_with(f), None)
        assert msg in gpu.error_message(), (msg, gpu.error_message())
        assert b.encode() == want
        one = (fiasco_amd.YCbCrFrame * 1)(f)
        if msg != "size and colour model":
            assert not L.fiasco_amd_batch_stage_device_ycbcr(1, one, None, ctypes.c_float(20.0), o.handle)
            assert msg in gpu.error_message(), (msg, gpu.error_message())
            assert not L.fiasco_amd_seq_open_device_ycbcr(1, one, None, ctypes.c_float(20.0), o.handle, 0, 1)
            assert msg in gpu.error_message(), (msg, gpu.error_message())
    # rows beyond the allocation: a frame of 8192 x 8192 declared over a small tensor
    one = (fiasco_amd.YCbCrFrame * 1)(struct(width=8192, height=8192))
    assert not L.fiasco_amd_batch_stage_device_ycbcr(1, one, None, ctypes.c_float(20.0), o.handle)
    assert "beyond the end of their device allocation" in gpu.error_message(), gpu.error_message()
    # through the binding: the wrong number of frames, host arrays, no frames
    with pytest.raises(fiasco_amd.FiascoError):
        b.upload_device_ycbcr(good[:2])
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.upload_device_ycbcr([(hosty, hostc)] * 3)
    assert "not in device memory" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.Batch.from_device_ycbcr(gpu, [], 20.0, o)
    assert "No frames" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.Batch.from_device_ycbcr(gpu, good, 0.0, o)
    assert "quality" in str(e.value)
    assert b.encode() == want
    # a YCbCr frame into a gray batch
    gray = [to_gpu(synth.synth(96, 64, 30 + i)) for i in range(3)]
    g = fiasco_amd.Batch.from_device(gpu, gray, 20.0, o)
    wantg = g.encode()
    assert None not in wantg
    with pytest.raises(fiasco_amd.FiascoError) as e:
        g.upload_device_ycbcr(good)
    assert "colour model" in str(e.value)
    assert g.encode() == wantg
    # and a gray frame into the YCbCr batch
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.upload_device(gray)
    assert "colour model" in str(e.value)
    assert b.encode() == want
    b.free(); g.free(); o.delete()
