"""Decoded frames as 8-bit pixels in device memory (include/libfiasco_amd_hip.h: fiasco_amd_batch_decode_device,
fiasco_amd_planes_to_pixels_device; csrc/hip/output_convert.inc), on the device: the conversion kernel against the
numpy restatement of the reference's write_image (tests/pixels_ref.py, pinned to the reference's bytes by
tests/test_device_output_api.py) over its whole domain, the decoded frames against the bytes `dfiasco -s 0 -o`
writes, the shapes at which the kernel takes another path, the ordering against the caller's stream, the refusals.
The targets are torch tensors: torch is what a user of these entry points holds them in."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import synth
from conftest import GOLDEN, REF_SHARE, ROOT, options_from_args
from pixels_ref import pixels_of_planes, rgb_of_ints

pytestmark = pytest.mark.gpu

DFIASCO = os.path.join(ROOT, "oracle", "_ref", "dfiasco_ref")


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pattern(*shape):
    """a tensor of bytes that no decoded frame looks like: what a call must leave alone is compared with it"""
    n = int(np.prod(shape))
    return to_gpu(((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8).reshape(shape))


def packed(geom):
    """a packed target for a frame of (width, height, bands): H x W or H x W x 3"""
    w, h, bands = geom
    return torch.zeros((h, w) if bands == 1 else (h, w, 3), dtype=torch.uint8, device="cuda")


def decoded(b):
    """every frame of a finished batch through decode_device into packed tensors -> list of numpy arrays"""
    ts = [packed(g) for g in b._geom]
    assert b.decode_device(ts) == b.n, b.lib.error_message()
    return [t.cpu().numpy() for t in ts]


def colour(w, h):
    """a colour frame; at these sizes and seeds the coder finishes (small colour frames can run into the reference's
    "Can't write more than n weights")"""
    assert (w, h) in ((34, 32), (50, 34), (128, 96))
    return synth.synth_color_k(w, h, 5)


def pnm_of(a):
    return synth.pgm_bytes(a) if a.ndim == 2 else synth.ppm_bytes(a)


# ------------------------------------------------------------------ 1. the conversion over its whole domain

def convert(gpu, planes, layout):
    """planes (numpy int16, H x W or 3 x H x W) through the kernel -> numpy uint8 H x W or H x W x 3"""
    d = to_gpu(planes)
    h, w = planes.shape[-2:]
    if planes.ndim == 2:
        t = pattern(h, w)
    elif layout == "interleaved":
        t = pattern(h, w, 3)
    else:
        t = pattern(3, h, w)
    fiasco_amd.planes_to_pixels_device(gpu, d, t)
    torch.cuda.synchronize()
    out = t.cpu().numpy()
    return out.transpose(1, 2, 0) if layout == "planar" else out


def luminances():
    """64 values of Y >> 4 from -2048 .. 2047: the ends, dense around both clip edges (yval = 0 and 255 before the
    chroma terms, which reach +-226), the stretch between and around them"""
    ys = np.concatenate([[-2048, -1500, -900, -500, 500, 900, 1500, 2047], np.arange(-138, -118), np.arange(117, 137),
                         [-360, -310, -262, -214, -166, -70, -22, 26, 74, 160, 208, 256, 304, 352, 400, 448]])
    assert len(np.unique(ys)) == 64
    return ys


def test_conversion_is_exact_over_its_whole_domain(gpu):
    rng = np.random.default_rng(4242)

    def fixed(ints):
        """12.4 fixed point with a random low nibble: the shift is exercised on negatives"""
        return ((ints.astype(np.int32) << 4) | rng.integers(0, 16, ints.shape)).astype(np.int16)

    # gray: all 65 536 int16 values (in a shuffled order) as one frame of 256 x 256
    g = rng.permutation(np.arange(-32768, 32768, dtype=np.int32)).astype(np.int16).reshape(256, 256)
    want = pixels_of_planes(g)
    assert want.min() == 0 and want.max() == 255
    assert np.array_equal(convert(gpu, g, "gray"), want)
    # colour set A: all 65 536 (cb, cr) byte pairs x 64 luminances = 16 frames of 512 x 512
    pair = np.arange(65536, dtype=np.int32)
    cb = np.repeat(((pair >> 8) - 128)[None, :], 64, axis=0)
    cr = np.repeat(((pair & 255) - 128)[None, :], 64, axis=0)
    yy = np.repeat(luminances()[:, None], 65536, axis=1)
    setA = np.stack([fixed(v).reshape(16, 512, 512) for v in (yy, cb, cr)], axis=1)
    # colour set B: all 4 096 values of Y >> 4 x all 256 cr, cb a permutation of cr = 4 frames of 512 x 512
    perm = rng.permutation(256)
    yy = np.repeat(np.arange(-2048, 2048, dtype=np.int32)[:, None], 256, axis=1)
    crb = np.repeat((np.arange(256, dtype=np.int32) - 128)[None, :], 4096, axis=0)
    cbb = np.repeat((perm.astype(np.int32) - 128)[None, :], 4096, axis=0)
    setB = np.stack([fixed(v).reshape(4, 512, 512) for v in (yy, cbb, crb)], axis=1)
    # one frame more whose chroma planes leave +-128 (the clamp): every plane random over all of int16
    setC = rng.integers(-32768, 32768, (1, 3, 512, 512)).astype(np.int16)
    assert (np.abs(setC[0, 1:].astype(np.int32) >> 4) > 128).mean() > 0.9
    frames = np.concatenate([setA, setB, setC])
    assert frames.shape == (21, 3, 512, 512)
    for k, planes in enumerate(frames):
        want = pixels_of_planes(planes)
        for layout in ("interleaved", "planar"):
            got = convert(gpu, planes, layout)
            assert np.array_equal(got, want), (k, layout, int((got != want).sum()))


# ------------------------------------------------------------------ 2. decoded frames are the reference's bytes

def test_decoded_frames_are_the_references_bytes(gpu, manifest, inputs):
    rec = json.load(open(os.path.join(GOLDEN, "DECODED_RGB.json")))["cases"]
    todo = [(name, ent["decoded_md5"], 3) for name, ent in rec.items()]
    todo += [(name, ent["decoded_md5"], 1) for name, ent in manifest["decoded_psnr"].items()]
    count = {1: 0, 3: 0}
    for name, md5, bands in todo:
        case = [c for c in manifest["cases"] if c["name"] == name][0]
        data = inputs.data(case["inputs"][0])
        w, h, nb = fiasco_amd._pnm_geometry(data)
        assert nb == bands, name
        if w > 512:
            continue
        q, o = options_from_args(gpu, case["args"])
        b = fiasco_amd.Batch(gpu, [data], q, o)
        out = b.encode()
        assert out[0] is not None and hashlib.md5(out[0]).hexdigest() == case["md5"], (name, gpu.error_message())
        got = decoded(b)[0]
        b.free(); o.delete()
        assert got.shape == ((h, w, 3) if bands == 3 else (h, w))
        assert hashlib.md5(got.tobytes()).hexdigest() == md5, name
        count[bands] += 1
    assert count[3] >= 4 and count[1] >= 4, count           # the comparison must not be hollow


def test_decoded_frames_equal_dfiasco_on_random_frames(gpu, tmp_path):
    """Six random frames, encoded on the device; the reference's decoder run on the stream the device just wrote."""
    if not os.path.exists(DFIASCO):
        pytest.skip("the reference's binaries did not travel (oracle/ref_build.sh builds them in the build container)")
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    rng = np.random.default_rng(90210)
    for k in range(6):
        colour = bool(k & 1)
        w, h = (int(rng.integers(16, 101)) * 2 for _ in range(2))
        q = float(rng.choice([5, 12, 20, 45, 70, 90]))
        a = synth.synth_color_k(w, h, 300 + k) if colour else synth.synth(w, h, 300 + k)
        o = gpu.cli_options()
        b = fiasco_amd.Batch.from_device(gpu, [to_gpu(a)], q, o)
        out = b.encode()
        assert out[0] is not None, gpu.error_message()
        got = decoded(b)[0]
        b.free(); o.delete()
        fco, dec = str(tmp_path / ("r%d.fco" % k)), str(tmp_path / ("r%d.pnm" % k))
        open(fco, "wb").write(out[0])
        subprocess.check_call([DFIASCO, "-s", "0", "-o", dec, fco], env=env, stderr=subprocess.DEVNULL)
        raw = open(dec, "rb").read()
        assert raw[:2] == (b"P6" if colour else b"P5")
        assert raw[len(raw) - got.size:] == got.tobytes(), (k, w, h, colour, q)


# ------------------------------------------------------------------ 3. shapes at which the kernel can go wrong

def untouched(big, before, region):
    """the bytes of `big' outside `region' (a tuple of slices) are those of `before'"""
    mask = torch.ones_like(big, dtype=torch.bool)
    mask[region] = False
    return bool(torch.equal(big[mask], before[mask]))


def test_ragged_rows_strided_and_unaligned_targets(gpu):
    o = gpu.cli_options()
    for w, h in ((34, 32), (50, 34), (128, 96)):
        gray, col = synth.synth(w, h, 3), colour(w, h)
        b = fiasco_amd.Batch(gpu, [pnm_of(gray), pnm_of(col)], 20.0, o)
        assert None not in b.encode(), gpu.error_message()
        wantg, wantc = decoded(b)
        # the host outlet for the gray frame; for the colour frame wherever it did not clip Y
        assert wantg.tobytes() == b.decode_plane(0, 0, w, h)
        yb, cbb, crb = (np.frombuffer(b.decode_plane(1, k, w, h), np.uint8).astype(np.int32).reshape(h, w) for k in range(3))
        ok = (yb > 0) & (yb < 255)
        assert ok.mean() > 0.9 and np.array_equal(wantc[ok], rgb_of_ints(yb, cbb - 128, crb - 128)[ok])
        # cut out of larger tensors, starting at an odd byte column; an interleaved pitch > 3 w; padded planes
        bigg, bigc, bigp = pattern(h + 20, w + 30), pattern(h + 20, w + 30, 3), pattern(3, h + 8, w + 16)
        wide = pattern(h, w + 10, 3)
        keep = [t.clone() for t in (bigg, bigc, bigp, wide)]
        rg, rc, rp, rw = (slice(7, 7 + h), slice(5, 5 + w)), (slice(7, 7 + h), slice(5, 5 + w)), \
            (slice(None), slice(4, 4 + h), slice(3, 3 + w)), (slice(None), slice(0, w))
        assert bigg[rg].data_ptr() % 2 == 1 and bigc[rc].data_ptr() % 2 == 1 and wide[rw].stride(0) > 3 * w
        assert b.decode_device([bigg[rg], bigc[rc]]) == 2
        assert np.array_equal(bigg[rg].cpu().numpy(), wantg) and np.array_equal(bigc[rc].cpu().numpy(), wantc)
        assert b.decode_device([None, bigp[rp]]) == 1
        assert np.array_equal(bigp[rp].cpu().numpy().transpose(1, 2, 0), wantc)
        assert b.decode_device([None, wide[rw]]) == 1
        assert np.array_equal(wide[rw].cpu().numpy(), wantc)
        for t, before, region in zip((bigg, bigc, bigp, wide), keep, (rg, rc, rp, rw)):
            assert untouched(t, before, region), (w, h, tuple(t.shape))
        # packed planar
        pl = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
        assert b.decode_device([None, pl]) == 1
        assert np.array_equal(pl.cpu().numpy().transpose(1, 2, 0), wantc)
        b.free()
    o.delete()


def test_frames_of_different_sizes_in_one_flight_and_two_flights(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(96, 64, 1), colour(50, 34), synth.synth(34, 40, 2)]
    single = []
    for a in arrs:
        b = fiasco_amd.Batch(gpu, [pnm_of(a)], 20.0, o)
        assert None not in b.encode()
        single.append(decoded(b)[0])
        b.free()
    b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in arrs], 20.0, o)
    assert None not in b.encode()
    gpu.reset_stats()
    got = decoded(b)
    st = gpu.get_stats()
    b.free()
    for g, s in zip(got, single):
        assert np.array_equal(g, s)
    assert st.decoder_frames == 3 and st.decoder_bytes > 3 * sum(a.size for a in arrs)
    # 34 gray frames of 32 x 32: two flights
    arrs = [synth.synth(32, 32, 100 + i) for i in range(34)]
    b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in arrs], 20.0, o)
    assert None not in b.encode()
    big = pattern(34, 40, 48)
    keep = big.clone()
    assert b.decode_device([big[i, 3:35, 9:41] for i in range(34)]) == 34
    for i in range(34):
        assert big[i, 3:35, 9:41].cpu().numpy().tobytes() == b.decode_plane(i, 0, 32, 32), i
    assert untouched(big, keep, (slice(None), slice(3, 35), slice(9, 41)))
    b.free(); o.delete()


# ------------------------------------------------------------------ 4. agreement with the existing outlet

def test_gray_result_is_decode_plane(gpu, inputs):
    o = gpu.cli_options()
    data = inputs.data("g256")
    b = fiasco_amd.Batch(gpu, [data], 20.0, o)
    assert None not in b.encode()
    assert decoded(b)[0].tobytes() == b.decode_plane(0, 0, 256, 256)
    b.free(); o.delete()


# ------------------------------------------------------------------ 5. round trip on the device

def test_round_trip_on_a_side_stream_without_host_synchronisation(gpu):
    o = gpu.cli_options()
    host = np.stack([synth.synth(96, 64, 50 + i) for i in range(4)])
    hostc = colour(128, 96)
    # everything synchronised
    frames = [*to_gpu(host), to_gpu(hostc)]
    torch.cuda.synchronize()
    b = fiasco_amd.Batch.from_device(gpu, frames, 20.0, o)
    assert None not in b.encode()
    torch.cuda.synchronize()
    want = [packed(g) for g in b._geom]
    assert b.decode_device(want) == 5
    torch.cuda.synchronize()
    b.free()
    # on a side stream: the targets are written just before the call and read just after it, in stream order only
    side = torch.cuda.Stream()
    pinned, pinnedc = torch.from_numpy(host).pin_memory(), torch.from_numpy(hostc).pin_memory()
    with torch.cuda.stream(side):
        frames = [*pinned.cuda(non_blocking=True), pinnedc.cuda(non_blocking=True)]
        b = fiasco_amd.Batch.from_device(gpu, frames, 20.0, o)
        assert None not in b.encode()
        targets = [torch.empty_like(t) for t in want]
        for t in targets:
            t.fill_(7)                                  # the conversion must wait for this
        assert b.decode_device(targets) == 5            # stream: torch's current one, the side stream
        got = [t.clone() for t in targets]              # reads on the side stream, no host synchronisation
        sums = torch.stack([t.sum(dtype=torch.int64) for t in targets])
    side.synchronize()
    for g, t in zip(got, want):
        assert torch.equal(g, t)
    assert sums.tolist() == [int(t.sum(dtype=torch.int64)) for t in want]
    # an explicit stream handle does the same
    with torch.cuda.stream(side):
        for t in targets:
            t.fill_(9)
    assert b.decode_device(targets, stream=side.cuda_stream) == 5
    with torch.cuda.stream(side):
        got = [t.clone() for t in targets]
    side.synchronize()
    for g, t in zip(got, want):
        assert torch.equal(g, t)
    b.free(); o.delete()


# ------------------------------------------------------------------ 6. refusals, skipped frames, two shares

class Raw:
    def __init__(self, ptr, shape, strides=None):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}


def test_refusals_write_nothing_and_name_the_frame(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(96, 64, 30 + i) for i in range(3)]
    b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in arrs], 20.0, o)
    good = [pattern(64, 96) for _ in range(3)]
    keep = good[0].clone()
    with pytest.raises(fiasco_amd.FiascoError) as e:                 # no finished pass
        b.decode_device(good)
    assert "no finished pass" in str(e.value)
    assert None not in b.encode()
    host = np.zeros((64, 96), dtype=np.uint8)
    col = pattern(64, 96, 3)
    cases = [
        (Raw(host.ctypes.data, (64, 96)), "not in device memory"),
        (Raw(good[1].data_ptr(), (64, 96), (1 << 32, 1)), "beyond the end of their device allocation"),
        (Raw(good[1].data_ptr(), (64, 96), (95, 1)), "smaller than a row"),
        (pattern(64, 64), "96 x 64"),
        (pattern(66, 96), "96 x 64"),
        (col, "colour model"),
        (pattern(3, 64, 96), "colour model"),
    ]
    for bad, msg in cases:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_device([good[0], bad, good[2]])
        assert msg in str(e.value) and "<device target 1>" in str(e.value), (msg, str(e.value))
        assert torch.equal(good[0], keep) and torch.equal(good[2], keep)
    # the C entry itself: no batch
    f = gpu.L.fiasco_amd_batch_decode_device
    assert f(None, fiasco_amd._device_targets(good), None) == 0 and "empty batch" in gpu.error_message()
    # a gray target for a colour frame
    c = fiasco_amd.Batch(gpu, [pnm_of(colour(128, 96))], 20.0, o)
    assert None not in c.encode()
    grayt = pattern(96, 128)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        c.decode_device([grayt])
    assert "colour model" in str(e.value) and "<device target 0>" in str(e.value) and torch.equal(grayt, pattern(96, 128))
    c.free()
    # None skips a frame and is counted out
    want = decoded(b)
    assert b.decode_device([good[0], None, good[2]]) == 2
    assert np.array_equal(good[0].cpu().numpy(), want[0]) and np.array_equal(good[2].cpu().numpy(), want[2])
    assert torch.equal(good[1], keep)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_device([None, None, None])
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_device(good[:2])
    # planes_to_pixels_device: planes and target must agree
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.planes_to_pixels_device(gpu, torch.zeros((64, 96), dtype=torch.int16, device="cuda"), col)
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.planes_to_pixels_device(gpu, torch.zeros((64, 64), dtype=torch.int16, device="cuda"), good[1])
    assert torch.equal(good[1], keep)
    b.free(); o.delete()


def test_a_failed_frame_is_skipped_and_counted_out(gpu, inputs):
    """MAXSTATES 103: the 256 x 256 survey image needs one state more and fails, a flat frame does not."""
    o = gpu.cli_options()
    flat = np.full((64, 64), 90, dtype=np.uint8)
    try:
        gpu.set_limits(103, 22)
        b = fiasco_amd.Batch(gpu, [inputs.data("g256"), pnm_of(flat)], 20.0, o)
        out = b.encode()
        assert out[0] is None and out[1] is not None, gpu.error_message()
        t0, t1 = pattern(256, 256), pattern(64, 64)
        keep = t0.clone()
        assert b.decode_device([t0, t1]) == 1
        assert torch.equal(t0, keep) and t1.cpu().numpy().tobytes() == b.decode_plane(1, 0, 64, 64)
        b.free()
    finally:
        gpu.set_limits(6000, 22)
        o.delete()


def test_two_shares_on_one_gpu_give_the_same_bytes(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(96, 64, 70 + i) for i in range(4)] + [colour(128, 96)]
    b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in arrs], 20.0, o)
    assert None not in b.encode()
    want = decoded(b)
    b.free()
    gpu.set_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in arrs], 20.0, o)
        assert None not in b.encode(), gpu.error_message()
        got = decoded(b)
        b.free()
    finally:
        gpu.set_devices([])
        o.delete()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
