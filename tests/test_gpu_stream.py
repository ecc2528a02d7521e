""".fco streams read back and decoded on the device, video frames included -- run on a real MI355X: -m gpu.
(include/libfiasco_amd_stream.h; csrc/host/fa_reader.c, fa_stream.c; csrc/hip/stream_decode.inc, frame_decoder.inc: the
blocks of a magnified P/B frame, dec_mc420_kernel, the smoothed copy of a frame that is also a reference.)

Yardsticks, all compared with ==:
  tests/golden/DECODED_STREAMS.json (tests/golden/make_decoded_streams.py): per stream, display frame, magnification,
    format and smoothing the md5 of what the REFERENCE's decoder library hands out -- the 12.4 planes and the bytes;
  tests/golden/RECONST.json: the reference CODER's reconstructed planes of the pinned videos, which `dfiasco -s 0' and so
    Stream.decode_planes() show at the default mantissas;
  the library's own coder side, no fixture: the outputs of a Sequence and Batch.decode_shown / decode_420.
No frame is larger than 256 x 256, no video longer than 5 frames; a case takes well under a second on the device.
No stream is fed here that the reader has not validated: mutated streams are a CPU matter (tests/test_stream_check.py)."""
import hashlib
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch            # before the product library is loaded: one HIP runtime for both

import fiasco_amd
import reconst_cases as rc
import stream_cases as sc
import synth
from conftest import GOLDEN, options_from_args

pytestmark = pytest.mark.gpu

FIX = sc.fixture()


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def targets_of(w, h, colour, n):
    return [torch.full((h, w, 3) if colour else (h, w), 7, dtype=torch.uint8, device="cuda") for _ in range(n)]


def targets_420(w, h, n, nv12=False):
    def one():
        y = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
        if nv12:
            return (y, torch.full((h // 2, w // 2, 2), 7, dtype=torch.uint8, device="cuda"))
        return (y, torch.full((h // 2, w // 2), 7, dtype=torch.uint8, device="cuda"), torch.full((h // 2, w // 2), 7, dtype=torch.uint8, device="cuda"))
    return [one() for _ in range(n)]


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------ the reference decoder's frames

@pytest.mark.parametrize("name", sc.NAMES)
def test_every_frame_as_the_reference_decoder_hands_it_out(gpu, name):
    """every tuple of the fixture: (magnification, format, smoothing) x display frame, through decode_device / decode_420
    and decode_planes / decode_planes_420; a tuple the reference refuses is refused here too"""
    rec = FIX["streams"][name]
    s = fiasco_amd.Stream(gpu, sc.stream_bytes(name))
    colour, n = bool(s.info["color"]), s.n
    assert s.frame_types == rec["frame_types"] and n <= 5
    seen = 0
    for key, ent in sorted(rec["decoded"].items()):
        m, fmt, smoothing = sc.parse_key(key)
        if "refused" in ent:
            with pytest.raises(fiasco_amd.FiascoError):
                w, h = fiasco_amd.magnified_size(gpu, s.info["width"], s.info["height"], m)
                s.decode_device(targets_of(w, h, colour, n), magnify=m, smoothing=smoothing)
            continue
        w, h = ent["width"], ent["height"]
        assert (w, h) == tuple(fiasco_amd.magnified_size(gpu, s.info["width"], s.info["height"], m)) and max(w, h) <= 512
        if fmt == "444":
            tg = targets_of(w, h, colour, n)
            assert s.decode_device(tg, magnify=m, smoothing=smoothing) == n, (name, key, gpu.error_message())
            got = [md5(host(t)) for t in tg]
            assert got == [f["pixels_md5"] for f in ent["frames"]], (name, key)
            if smoothing == 0:
                assert [rc.planes_md5(s.decode_planes(d, magnify=m)) for d in range(n)] == [f["planes_md5"] for f in ent["frames"]], (name, key)
        else:
            tg = targets_420(w, h, n)
            assert s.decode_420(tg, magnify=m, smoothing=smoothing) == n, (name, key, gpu.error_message())
            got = [md5(np.concatenate([host(p).ravel() for p in t])) for t in tg]
            assert got == [f["pixels_md5"] for f in ent["frames"]], (name, key)
            if smoothing == 0:
                planes = [s.decode_planes_420(d, magnify=m) for d in range(n)]
                assert [md5(np.concatenate([p.ravel() for p in f])) for f in planes] == [f["planes_md5"] for f in ent["frames"]], (name, key)
        seen += 1
    assert seen, name
    s.free()


def test_nv12_and_a_window_of_frames(gpu):
    """NV12 targets give the I420 samples interleaved; a range that begins behind an I frame decodes its references on the way"""
    name = sc.IPBBP
    s = fiasco_amd.Stream(gpu, sc.stream_bytes(name))
    w, h, n = s.info["width"], s.info["height"], s.n
    full, nv = targets_420(w, h, n), targets_420(w, h, n, nv12=True)
    assert s.decode_420(full, smoothing=0) == n and s.decode_420(nv, smoothing=0) == n
    for a, b in zip(full, nv):
        assert np.array_equal(host(a[0]), host(b[0])) and np.array_equal(np.stack([host(a[1]), host(a[2])], -1), host(b[1]))
    whole, part = targets_of(w, h, True, n), targets_of(w, h, True, 2)
    assert s.decode_device(whole) == n and s.decode_device(part, first=n - 2) == 2
    assert [md5(host(t)) for t in part] == [md5(host(t)) for t in whole[n - 2:]]
    gap = [None] * n
    gap[n - 1] = targets_of(w, h, True, 1)[0]
    assert s.decode_device(gap) == 1 and md5(host(gap[n - 1])) == md5(host(whole[n - 1]))
    s.free()


# ------------------------------------------------------------------ the coder's reconstruction: no new fixture

@pytest.mark.parametrize("name", sc.RECONST_NAMES)
def test_decode_planes_are_the_reference_coders_reconstruction(gpu, manifest, inputs, name):
    """the stream the device codes is the reference's (RECONST.json), and read back, every frame decodes to the planes the
    reference CODER reconstructed: I, P and B frames at the default mantissas"""
    frames, args = rc.case_of(manifest, inputs, name)
    rec = rc.fixture()[name]
    q, o = options_from_args(gpu, args)
    seq = fiasco_amd.Sequence(gpu, frames, q, o)
    stream = seq.encode()
    seq.free(); o.delete()
    assert hashlib.md5(stream).hexdigest() == rec["stream_md5"]
    s = fiasco_amd.Stream(gpu, stream)
    assert s.rewrite() == stream
    assert s.frame_types == [f["type"] for f in rec["frames"]]
    assert [rc.planes_md5(s.decode_planes(f["display"])) for f in rec["frames"]] == [f["planes_md5"] for f in rec["frames"]]
    s.free()


# ------------------------------------------------------------------ ties to the coder side of the library

def _colour_video(n=5, w=64, h=64):
    """the frames of st_color_ipbbp_64 (tests/golden/make_decoded_streams.py): most small colour videos end in "Can't write
    more than n weights", in the reference and here alike; this one is coded at -q 40"""
    a = synth.synth(200, 160, 11).astype(np.int32)
    return [synth.ppm_bytes(np.clip(np.stack([a[10 + 2 * i:10 + h + 2 * i, 20 + 3 * i:20 + w + 3 * i] + d for d in (30, -20, 10)], -1), 0, 255).astype(np.uint8))
            for i in range(n)]


@pytest.mark.parametrize("kind", ["gray", "colour"])
def test_stream_of_a_sequence_decodes_to_the_sequences_outputs(gpu, kind):
    """Sequence.encode() of a small `ipbbp` with outputs set; the stream read back gives the same bytes for every frame"""
    frames = rc._shift(5) if kind == "gray" else _colour_video()
    w, h, nb = rc.geometry(frames)
    q, o = options_from_args(gpu, ["--pattern", "ipbbp"] + (["-q", "40"] if kind == "colour" else []))
    seq = fiasco_amd.Sequence(gpu, frames, q, o)
    want = targets_of(w, h, nb == 3, 5)
    seq.set_outputs(want, False)
    stream = seq.encode()
    seq.free(); o.delete()
    s = fiasco_amd.Stream(gpu, stream)
    assert s.frame_types == [0, 1, 2, 2, 1] and s.coding_order == [0, 1, 4, 2, 3]
    got = targets_of(w, h, nb == 3, 5)
    assert s.decode_device(got, smoothing=0) == 5, gpu.error_message()
    for d in range(5):
        assert np.array_equal(host(got[d]), host(want[d])), (kind, d)
    if kind == "colour":
        assert stream == sc.stream_bytes(sc.IPBBP)          # ... and is the reference's stream
    s.free()


@pytest.mark.parametrize("magnify", [-1, 0, 1])
def test_streams_of_a_batch_decode_as_the_batch_does(gpu, magnify):
    """all-intra: the streams of a Batch through Stream against Batch.decode_shown / decode_420 at the same options"""
    pnm = [synth.ppm_bytes(synth.synth_color_k(102, 66, 5, 0)), synth.ppm_bytes(synth.synth_color_k(64, 64, 6, 0))]
    o = gpu.cli_options()
    o.set_smoothing(70)
    b = fiasco_amd.Batch(gpu, pnm, 20.0, o)
    streams = b.encode()
    sizes = [fiasco_amd.magnified_size(gpu, *fiasco_amd._pnm_geometry(p)[:2], magnify) for p in pnm]
    for smoothing in (-1, 0, 35):
        want = [targets_of(w, h, True, 1)[0] for w, h in sizes]
        assert b.decode_shown(want, magnify=magnify, smoothing=smoothing) == 2
        want4 = [targets_420(w, h, 1)[0] for w, h in sizes]
        assert b.decode_420(want4, magnify=magnify, smoothing=smoothing) == 2
        for i, data in enumerate(streams):
            s = fiasco_amd.Stream(gpu, data)
            got, got4 = targets_of(*sizes[i], True, 1), targets_420(*sizes[i], 1)
            assert s.decode_device(got, magnify=magnify, smoothing=smoothing) == 1
            assert s.decode_420(got4, magnify=magnify, smoothing=smoothing) == 1
            assert np.array_equal(host(got[0]), host(want[i])), (i, magnify, smoothing)
            for p, r in zip(got4[0], want4[i]):
                assert np.array_equal(host(p), host(r)), (i, magnify, smoothing)
            s.free()
    b.free(); o.delete()


# ------------------------------------------------------------------ refusals on the device path

def test_refusals(gpu):
    s = fiasco_amd.Stream(gpu, sc.stream_bytes(sc.IPBBP))
    w, h, n = s.info["width"], s.info["height"], s.n
    with pytest.raises(fiasco_amd.FiascoError, match=r"<device target 1>: %d x %d pixels for a frame of %d x %d\." % (w + 2, h, w, h)):
        s.decode_device(targets_of(w, h, True, 1) + targets_of(w + 2, h, True, 1))
    with pytest.raises(fiasco_amd.FiascoError, match="at magnification 1"):
        s.decode_device(targets_of(w, h, True, n), magnify=1)
    with pytest.raises(fiasco_amd.FiascoError, match="layout contradicts"):
        s.decode_device(targets_of(w, h, False, n))
    with pytest.raises(fiasco_amd.FiascoError, match="smoothing out of range"):
        s.decode_device(targets_of(w, h, True, n), smoothing=101)
    with pytest.raises(fiasco_amd.FiascoError, match="no such frames"):
        s.decode_device(targets_of(w, h, True, 2), first=n - 1)
    with pytest.raises(fiasco_amd.FiascoError, match="Magnification factor `-2' is too small"):
        s.decode_planes(0, magnify=-2)
    s.free()
    g = fiasco_amd.Stream(gpu, open(os.path.join(GOLDEN, "seq2_gray_ip.fco"), "rb").read())
    with pytest.raises(fiasco_amd.FiascoError, match="a gray frame has no chroma bands"):
        g.decode_420(targets_420(g.info["width"], g.info["height"], 2))
    g.free()


def test_half_pixel_stream_is_read_and_not_decoded(gpu):
    """tests/golden/seq2_gray_ip_halfpel.fco is no half-pixel stream (cfiasco drops the option; its md5 is seq2_gray_ip_pred's).
    The stream here is seq2_gray_ip with the half-pixel bit of its header set: the reader validates it like any other"""
    data = sc.half_pixel_stream(gpu)
    s = fiasco_amd.Stream(gpu, data)
    assert s.info["half_pixel"] == 1 and s.frame_types == [0, 1] and s.rewrite() == data
    w, h = s.info["width"], s.info["height"]
    one = targets_of(w, h, False, 1)
    assert s.decode_device(one, smoothing=0) == 1            # the I frame alone needs no vector
    with pytest.raises(fiasco_amd.FiascoError, match="Half-pixel motion vectors are not supported"):
        s.decode_device(targets_of(w, h, False, 2))
    with pytest.raises(fiasco_amd.FiascoError, match="Half-pixel motion vectors are not supported"):
        s.decode_planes(1)
    s.free()


def test_a_frame_that_fails_takes_its_dependants_along(gpu):
    """`ibbi`-like: an I frame as the future reference drops the past one (codec/decoder.c:229-246), so the B frames hold
    forward vectors without a frame to take them from.  They fail with a message, the I frames are written"""
    data = sc.orphaned_b_stream()
    s = fiasco_amd.Stream(gpu, data)
    assert s.frame_types == [0, 2, 2, 0] and s.coding_order == [0, 3, 1, 2]
    w, h = s.info["width"], s.info["height"]
    tg = targets_of(w, h, False, 4)
    assert s.decode_device(tg, smoothing=0) == 2
    msg = gpu.error_message()
    assert "display frame 1" in msg and "motion vector without its reference frame" in msg, msg
    assert (host(tg[1]) == 7).all() and (host(tg[2]) == 7).all() and not (host(tg[0]) == 7).all() and not (host(tg[3]) == 7).all()
    # frame 2 is predicted from frame 1 (B_as_past_ref): asked for alone, its message names the frame that failed first
    with pytest.raises(fiasco_amd.FiascoError, match="display frame 2 is predicted from frame 1, which failed"):
        s.decode_device([tg[2]], first=2, smoothing=0)
    s.free()


def test_two_shares_the_stream_stays_on_one(gpu):
    """the device listed twice: every job of a stream carries one share key, so the references never change share and the
    bytes are those of one share.  (A target on ANOTHER device is refused with both device numbers, as the batch entries
    refuse it; one device cannot show that.)"""
    s = fiasco_amd.Stream(gpu, sc.stream_bytes(sc.IBBP_B0))
    w, h, n = s.info["width"], s.info["height"], s.n
    one = targets_of(w, h, True, n)
    assert s.decode_device(one, magnify=0) == n
    gpu.set_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        two = targets_of(w, h, True, n)
        assert s.decode_device(two, magnify=0) == n
        assert [md5(host(t)) for t in two] == [md5(host(t)) for t in one]
    finally:
        gpu.set_devices([0])
    s.free()
