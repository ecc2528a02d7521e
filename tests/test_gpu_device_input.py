"""Frames that already live in device memory (include/libfiasco_amd_hip.h: fiasco_amd_batch_stage_device,
_upload_device, _input_planes; csrc/hip/input_convert.inc), on the device: the conversion kernel against the host's
convert_planes() for every pixel value there is, the streams against the real reference's, and the hand-over of
replacement frames with the caller's stream in between.  The frames are torch tensors: torch is what a user of
these entry points holds them in."""
import hashlib
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    # before the product library is loaded: torch brings the HIP runtime both then share (one runtime, one set of
    # allocations -- the library must recognise torch's pointers as device memory)
    import torch

import fiasco_amd
import synth
from conftest import options_from_args

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def pnm_array(data):
    """raw PGM / PPM bytes -> uint8 array H x W or H x W x 3"""
    w, h, bands = fiasco_amd._pnm_geometry(data)
    a = np.frombuffer(data[len(data) - w * h * bands:], dtype=np.uint8)
    return a.reshape(h, w) if bands == 1 else a.reshape(h, w, 3)


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def numpy_planes(rgb):
    """host/fa_image.c:108-110 in numpy float64, written left to right (equal to the host's convert_planes() for all
    2^24 triples: tests/test_device_input_api.py checks that without a GPU, the first test below with one)"""
    r, g, b = (rgb[..., k].astype(np.float64) for k in range(3))
    y = ((+0.2989 * r + 0.5866 * g + 0.1145 * b - 128) * 16).astype(np.int32).astype(np.int16)
    cb = ((-0.1687 * r - 0.3312 * g + 0.5000 * b) * 16).astype(np.int32).astype(np.int16)
    cr = ((+0.5000 * r - 0.4183 * g - 0.0816 * b) * 16).astype(np.int32).astype(np.int16)
    return np.stack([y, cb, cr])


def test_conversion_is_exact_for_every_pixel_value(gpu):
    """All 2^24 RGB triples as 64 colour frames of 512 x 512, interleaved and planar, and all 256 gray values: the
    planes of the device-fed batch are the planes of the PNM-fed batch of the same pixels and the numpy evaluation."""
    o = gpu.cli_options()
    i = np.arange(1 << 24, dtype=np.uint32)
    rgb = np.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], axis=-1).astype(np.uint8).reshape(64, 512, 512, 3)
    pnm = fiasco_amd.Batch(gpu, [synth.ppm_bytes(f) for f in rgb], 20.0, o)
    inter = fiasco_amd.Batch.from_device(gpu, list(to_gpu(rgb)), 20.0, o)
    planar = fiasco_amd.Batch.from_device(gpu, list(to_gpu(rgb.transpose(0, 3, 1, 2))), 20.0, o)
    for k in range(64):
        want = pnm.input_planes(k)
        assert want.shape == (3, 512, 512) and want.dtype == np.int16
        assert np.array_equal(want, numpy_planes(rgb[k])), k
        for name, b in (("interleaved", inter), ("planar", planar)):
            got = b.input_planes(k)
            assert np.array_equal(got, want), (name, k, int((got != want).sum()))
    for b in (pnm, inter, planar):
        b.free()
    gray = (np.arange(64 * 64, dtype=np.uint32) % 256).astype(np.uint8).reshape(64, 64)
    pnm = fiasco_amd.Batch(gpu, [synth.pgm_bytes(gray)], 20.0, o)
    dev = fiasco_amd.Batch.from_device(gpu, [to_gpu(gray)], 20.0, o)
    want = pnm.input_planes(0)
    assert np.array_equal(want[0], (gray.astype(np.int16) - 128) * 16)
    assert np.array_equal(dev.input_planes(0), want)
    pnm.free(); dev.free(); o.delete()


def still_cases(manifest):
    return [c for c in manifest["cases"] if len(c["inputs"]) == 1]


def test_streams_are_the_references(gpu, manifest, inputs):
    """Every still case of the manifest (one input: gray and colour, odd aspect ratios, the -q / -z / option
    variants), its PNM decoded to a tensor on the GPU: the stream is the one the real reference wrote."""
    cases = still_cases(manifest)
    assert len(cases) >= 40 and {"g100x70_q20", "c00_q20", "k1080_z1", "g256_q99"} <= {c["name"] for c in cases}
    done = []
    for case in cases:
        q, o = options_from_args(gpu, case["args"])
        b = fiasco_amd.Batch.from_device(gpu, [to_gpu(pnm_array(inputs.data(case["inputs"][0])))], q, o)
        out = b.encode()
        b.free(); o.delete()
        assert out[0] is not None, (case["name"], gpu.error_message())
        assert len(out[0]) == case["bytes"] and hashlib.md5(out[0]).hexdigest() == case["md5"], case["name"]
        done.append(case["name"])
    assert done == [c["name"] for c in manifest["cases"] if len(c["inputs"]) == 1]        # nothing left out


def test_strided_sources(gpu):
    """A frame cut out of a larger tensor, a planar frame with padded planes, a source that starts at an odd column
    (no 16-byte alignment): read in place, same streams as their packed copies."""
    o = gpu.cli_options()
    big = to_gpu(synth.synth(400, 300, 5))                                       # gray 300 x 400
    rgb = np.ascontiguousarray(synth.synth_color_c(256, 192, 1))                 # 192 x 256 x 3
    bigc = to_gpu(np.pad(rgb, ((7, 9), (5, 11), (0, 0))))
    padded = torch.zeros((3, 200, 272), dtype=torch.uint8, device="cuda")
    padded[:, :192, :256] = to_gpu(rgb.transpose(2, 0, 1))
    views = [big[20:140, 64:224], big[21:141, 33:193], big[0:64, 1:97],
             bigc[7:199, 5:261], padded[:, :192, :256], padded[:, 4:196, 3:259]]
    assert views[0].stride(0) == 400 and views[1].data_ptr() % 2 == 1 and views[4].stride(0) == 200 * 272
    for v in views:
        assert not v.is_contiguous()
        got = fiasco_amd.Batch.from_device(gpu, [v], 20.0, o)
        ref = fiasco_amd.Batch.from_device(gpu, [v.contiguous()], 20.0, o)
        a = v.cpu().numpy()
        pnm = synth.pgm_bytes(a) if a.ndim == 2 else synth.ppm_bytes(a if a.shape[2] == 3 else a.transpose(1, 2, 0))
        want = gpu.encode_batch([pnm], 20.0, o)
        assert want[0] is not None
        assert np.array_equal(got.input_planes(0), ref.input_planes(0))
        assert got.encode() == want and ref.encode() == want, (tuple(v.shape), v.stride())
        got.free(); ref.free()
    # all of them in one batch: frames of different sizes and layouts in one launch of the kernel
    b = fiasco_amd.Batch.from_device(gpu, views, 20.0, o)
    outs = b.encode()
    for v, out in zip(views, outs):
        a = v.cpu().numpy()
        pnm = synth.pgm_bytes(a) if a.ndim == 2 else synth.ppm_bytes(a if a.shape[2] == 3 else a.transpose(1, 2, 0))
        assert [out] == gpu.encode_batch([pnm], 20.0, o)
    b.free(); o.delete()


def test_upload_device_replaces_inputs(gpu):
    """check_upload_replaces_inputs() of tests/test_host_api.py with upload_device: pass after pass, pipelined, mixed
    with PNM uploads, from a side stream that fills the tensors just before the call (the library orders its
    conversion behind the stream and the stream behind the conversion: the tensors are overwritten right after)."""
    o = gpu.cli_options()
    arrs = [[synth.synth(96, 64, 10 * k + i) for i in range(9)] for k in range(3)]
    sets = [[synth.pgm_bytes(a) for a in s] for s in arrs]
    want = [gpu.encode_batch(s, 20.0, o) for s in sets]
    assert all(None not in w for w in want)
    pinned = [torch.from_numpy(np.stack(s)).pin_memory() for s in arrs]
    side = torch.cuda.Stream()
    buf = torch.zeros((9, 64, 96), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def upload(b, k, stream=None):
        """set k through `buf' on the side stream: filled just before the call, scribbled over just after"""
        with torch.cuda.stream(side):
            buf.copy_(pinned[k], non_blocking=True)
            b.upload_device(list(buf), stream=stream)
            buf.fill_(0)

    with torch.cuda.stream(side):
        buf.copy_(pinned[0], non_blocking=True)
        b = fiasco_amd.Batch.from_device(gpu, list(buf), 20.0, o)
        buf.fill_(0)
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
    # mixed: PNM upload, device upload, PNM upload
    b.submit()
    b.upload(sets[1])
    assert b.collect(resubmit=True) == want[0]
    upload(b, 2)
    assert b.collect(resubmit=True) == want[1]
    b.upload(sets[0])
    assert b.collect(resubmit=True) == want[2]
    assert b.collect() == want[0]
    assert np.array_equal(b.input_planes(3)[0], (arrs[0][3].astype(np.int16) - 128) * 16)
    # a frame of another size is refused and the batch keeps its frames
    bad = list(to_gpu(np.stack(arrs[1])))
    bad[3] = to_gpu(synth.synth(64, 64, 1))
    with pytest.raises(fiasco_amd.FiascoError):
        b.upload_device(bad)
    assert "size" in gpu.error_message()
    assert b.encode() == want[0]
    # and a batch staged from PNM takes device frames
    p = fiasco_amd.Batch(gpu, sets[0], 20.0, o)
    p.submit()
    upload(p, 1)
    assert p.collect(resubmit=True) == want[0]
    assert p.collect() == want[1]
    torch.cuda.synchronize()
    p.free(); b.free(); o.delete()


def test_reencode_during_an_overlapped_device_upload_reads_its_own_pass(gpu, monkeypatch):
    """tests/test_gpu_parity.py test_reencode_during_an_overlapped_upload_reads_its_own_pass with device frames: the
    running pass re-stages every frame (capacity guess of 64 states) while the next pass's frames are converted."""
    o = gpu.cli_options()
    arr = {k: [synth.synth(160, 120, s + i) for i in range(9)] for k, s in (("A", 700), ("B", 800), ("C", 900))}
    want = {}
    for name, fr in arr.items():
        want[name] = gpu.encode_batch([synth.pgm_bytes(a) for a in fr], 20.0, o)
        assert None not in want[name], gpu.error_message()
    dev = {k: list(to_gpu(np.stack(v))) for k, v in arr.items()}
    monkeypatch.setenv("FIASCO_AMD_CAP_GUESS", "64")       # every frame outgrows it: re-encode at 1.5 x
    for slabs in ("3", None):                              # through the frame queue / one slab per frame
        if slabs: monkeypatch.setenv("FIASCO_AMD_QUEUE_SLABS", slabs)
        else: monkeypatch.delenv("FIASCO_AMD_QUEUE_SLABS")
        b = fiasco_amd.Batch.from_device(gpu, dev["A"], 20.0, o)
        b.submit()
        b.upload_device(dev["B"])                          # pass A is in flight and will re-stage
        assert b.collect(resubmit=True) == want["A"], gpu.error_message()
        b.upload_device(dev["C"])                          # the buffer pass A read
        assert b.collect(resubmit=True) == want["B"], gpu.error_message()
        assert b.collect(resubmit=False) == want["C"], gpu.error_message()
        b.free()
    o.delete()


def test_decoded_psnr_of_device_frames(gpu, manifest, inputs):
    """decode_psnr, decode_psnr_all and decode_plane of a device-fed batch fetch the original from the device: equal
    to the PNM-fed batch's.  (The manifest's "decoded_psnr" holds gray cases only: g256_q20 from there, with the
    reference tool's figure, and the colour still c256_q20.)"""
    for name in ("g256_q20", "c256_q20"):
        case = [c for c in manifest["cases"] if c["name"] == name][0]
        data = inputs.data(case["inputs"][0])
        w, h, bands = fiasco_amd._pnm_geometry(data)
        res = []
        for fed in ("pnm", "device"):
            q, o = options_from_args(gpu, case["args"])
            b = (fiasco_amd.Batch(gpu, [data], q, o) if fed == "pnm"
                 else fiasco_amd.Batch.from_device(gpu, [to_gpu(pnm_array(data))], q, o))
            out = b.encode()
            assert hashlib.md5(out[0]).hexdigest() == case["md5"]
            res.append((b.decode_psnr_all(), b.decode_psnr(0), [b.decode_plane(0, k, w, h) for k in range(bands)]))
            b.free(); o.delete()
        assert res[0] == res[1], name
        assert res[0][0][0] == 1 and all(np.isfinite(v) and v > 20 for v in res[0][1][0][:bands])
        if name in manifest["decoded_psnr"]:
            assert "%.2f" % res[1][1][0][0] == manifest["decoded_psnr"][name]["psnr_db"]


def test_several_shares_convert_their_own_frames(gpu):
    """set_devices([0, 0]): two shares on one GPU, nine frames dealt round robin, staged and replaced from device
    memory -- every share converts the frames fa_share_of() deals it.  Same streams as with one share."""
    o = gpu.cli_options()
    A = [synth.synth(160, 120, 40 + i) for i in range(9)]
    B = [synth.synth(160, 120, 60 + i) for i in range(9)]
    wantA = gpu.encode_batch([synth.pgm_bytes(a) for a in A], 20.0, o)
    wantB = gpu.encode_batch([synth.pgm_bytes(a) for a in B], 20.0, o)
    assert None not in wantA + wantB
    dA, dB = list(to_gpu(np.stack(A))), list(to_gpu(np.stack(B)))
    gpu.set_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        b = fiasco_amd.Batch.from_device(gpu, dA, 20.0, o)
        assert b.encode() == wantA, gpu.error_message()
        for i in (0, 1, 8):
            assert np.array_equal(b.input_planes(i)[0], (A[i].astype(np.int16) - 128) * 16)
        b.submit()
        b.upload_device(dB)
        assert b.collect(resubmit=True) == wantA
        assert np.array_equal(b.input_planes(4)[0], (B[4].astype(np.int16) - 128) * 16)
        b.upload([synth.pgm_bytes(a) for a in A])
        assert b.collect(resubmit=True) == wantB
        assert b.collect() == wantA
        b.free()
    finally:
        gpu.set_devices([])
        o.delete()


def test_refusals_leave_the_batch_as_it_was(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(96, 64, 30 + i) for i in range(3)]
    want = gpu.encode_batch([synth.pgm_bytes(a) for a in arrs], 20.0, o)
    good = list(to_gpu(np.stack(arrs)))
    b = fiasco_amd.Batch.from_device(gpu, good, 20.0, o)

    class Raw:
        def __init__(self, ptr, shape, strides=None):
            self.__cuda_array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}

    host = np.zeros((64, 96), dtype=np.uint8)
    wide = to_gpu(synth.synth(30, 64, 1)); odd = to_gpu(synth.synth(96, 63, 1))
    col = to_gpu(np.ascontiguousarray(synth.synth_color_c(96, 64, 0)))
    cases = [
        ([good[0], Raw(host.ctypes.data, (64, 96)), good[2]], "not in device memory"),
        ([good[0], Raw(good[1].data_ptr(), (64, 96), (95, 1)), good[2]], "smaller than a row"),
        ([good[0], good[1], col], "colour model"),
        ([good[0], good[1], to_gpu(synth.synth(64, 64, 1))], "size"),
    ]
    for frames, msg in cases:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.upload_device(frames)
        assert msg in str(e.value), (msg, str(e.value))
        assert b.encode() == want
    for frames, msg in [([Raw(host.ctypes.data, (64, 96))], "not in device memory"),
                        ([Raw(good[1].data_ptr(), (64, 96), (95, 1))], "smaller than a row"),
                        ([wide], "Width of image"), ([odd], "even numbers"), ([], "No frames")]:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.Batch.from_device(gpu, frames, 20.0, o)
        assert msg in str(e.value), (msg, str(e.value))
    # a gray tensor into a colour batch
    c = fiasco_amd.Batch.from_device(gpu, [col], 20.0, o)
    wantc = c.encode()
    assert wantc == gpu.encode_batch([synth.ppm_bytes(col.cpu().numpy())], 20.0, o)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        c.upload_device([good[0]])
    assert "colour model" in str(e.value)
    assert c.encode() == wantc
    assert b.encode() == want
    b.free(); c.free(); o.delete()


def test_1024_frames_of_1080p_from_one_tensor(gpu):
    """The headline geometry fed the way the feature is meant to be used: 1024 gray 1080p frames, one
    [1024, 1080, 1920] tensor, staged by one call (one conversion launch) and encoded once.  Same streams as the
    PNM-fed batch of the same frames."""
    o = gpu.cli_options()
    base = synth.synth(1920 + 64, 1080 + 64, 11)
    frames = np.empty((1024, 1080, 1920), dtype=np.uint8)
    for i in range(1024):
        frames[i] = base[i % 64:i % 64 + 1080, (i // 64) * 4:(i // 64) * 4 + 1920]
    t = torch.from_numpy(frames).cuda()
    b = fiasco_amd.Batch.from_device(gpu, t, 20.0, o)
    got = b.encode()
    b.free()
    del t
    assert None not in got, gpu.error_message()
    hdr = b"P5\n1920 1080\n255\n"
    p = fiasco_amd.Batch(gpu, [hdr + f.tobytes() for f in frames], 20.0, o)
    want = p.encode()
    p.free(); o.delete()
    assert got == want
