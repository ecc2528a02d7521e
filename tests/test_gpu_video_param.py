"""fiasco_c_options_set_video_param and the coding orders of B frames on the device -- run on a real MI355X: -m gpu.

The pins of tests/test_video_param_pins.py (tests/golden/VIDEO_PARAM.json: the streams and reconstructed frames of the
REFERENCE LIBRARY, cases in tests/video_param_cases.py) through the device: a B frame's device-decoded planes kept as
the past of a P search (`ibpbp`), runs of B frames that share one past reference (B_as_past_ref = 0) or hand it on
(= 1), two B runs in one group of pictures, the device-memory video entries with outputs in these orders.
  * fiasco_coder(): stream md5, every frame's planes md5 and block counts; the launcher's own choice of kernel build
    and, for three cases, FIASCO_AMD_NO_WIDE=1;
  * Sequence.from_device + set_outputs + encode(): every output frame is pixels_ref.pixels_of_planes of the
    fixture-checked planes, its distortion integers are distortion_ref's, every `written` flag is set;
  * the device listed twice and a second call on the three-GOP cases;
  * the refused patterns;
  * random cases (seeds 5200 .. 5223, video_param_cases.random_case) against the CPU oracle as int16 arrays and, where
    oracle/_ref/libfiasco_ref_recon.so is there, against the live reference library in a child process.
Frames are at most 128 pixels wide and there are at most 9 of them."""
import hashlib
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch            # before the product library is loaded: one HIP runtime for both

import fiasco_amd
import reconst_cases as rc
import seq_device_cases as sd
import video_param_cases as vc
from distortion_ref import distortion_of_planes
from pixels_ref import pixels_of_planes

pytestmark = pytest.mark.gpu

_runs = {}
_fuzz = {}


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def device_run(gpu, tmp_path_factory, name):
    """one fiasco_coder() run on the device per pinned case and session -> (fixture record, stream, planes, counts)"""
    if name not in _runs:
        frames, args, vp = vc.case_of(name)
        rec = vc.fixture()["cases"][name]
        assert rc.inputs_md5(frames) == rec["inputs_md5"] and args == rec["args"] and list(vp) == rec["video_param"], "the inputs of %s changed" % name
        stream, planes, counts, msg = vc.run_library(gpu, frames, args, vp, tmp_path_factory.mktemp("vp_" + name))
        assert stream is not None, "%s: %s" % (name, msg)
        _runs[name] = (rec, stream, planes, counts)
    return _runs[name]


@pytest.mark.parametrize("name", vc.NAMES)
def test_device_meets_the_reference_librarys_stream_and_frames(gpu, tmp_path_factory, name):
    vc.check_case(name, *device_run(gpu, tmp_path_factory, name))


@pytest.mark.parametrize("name", vc.NO_WIDE)
def test_the_256_thread_build_meets_them_too(gpu, tmp_path, name):
    frames, args, vp = vc.case_of(name)
    stream, planes, counts, msg = vc.run_library(gpu, frames, args, vp, tmp_path, env={"FIASCO_AMD_NO_WIDE": "1"})
    assert stream is not None, msg
    vc.check_case(name, vc.fixture()["cases"][name], stream, planes, counts)


def test_the_pinned_set_is_not_hollow_on_the_device(gpu, tmp_path_factory):
    vc.check_not_hollow({n: device_run(gpu, tmp_path_factory, n)[1:] for n in vc.NAMES})


# ------------------------------------------------------------------ the device-memory video entries

def to_gpu(a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the PNM's bytes are not writable


def device_fed(gpu, name, encodes=1):
    """Sequence.from_device with targets and distortion -> per encode (stream, [pixels], sse, maxdiff, written)"""
    frames, args, vp = vc.case_of(name)
    w, h, nb = rc.geometry(frames)
    q, o = vc.open_options(gpu, args, vp)
    seq = fiasco_amd.Sequence.from_device(gpu, [to_gpu(sd.array_of_pnm(f)) for f in frames], q, o)
    targets = [torch.full((h, w, 3) if nb == 3 else (h, w), 7, dtype=torch.uint8, device="cuda") for _ in frames]
    seq.set_outputs(targets, True)
    out = []
    for _ in range(encodes):
        stream = seq.encode()
        sse, mx, written = seq.distortion()
        torch.cuda.synchronize()
        out.append((stream, [t.cpu().numpy().copy() for t in targets], sse, mx, written))
        for t in targets:
            t.fill_(7)
    seq.free(); o.delete()
    return out


@pytest.mark.parametrize("name", vc.DEVICE_FED)
def test_device_fed_video_delivers_the_reference_librarys_frames(gpu, tmp_path_factory, name):
    """the yardstick: the planes of the fiasco_coder() run once their md5s have been found to be the fixture's"""
    rec, _, planes, _ = device_run(gpu, tmp_path_factory, name)
    frames, _, _ = vc.case_of(name)
    (stream, pixels, sse, mx, written), again = device_fed(gpu, name, encodes=2)
    assert hashlib.md5(stream).hexdigest() == rec["stream_md5"] and len(stream) == rec["bytes"]
    assert written.tolist() == [1] * len(frames)
    for f in rec["frames"]:
        d = f["display"]
        t, p = planes[d]
        assert rc.planes_md5(p) == f["planes_md5"], (name, d)
        assert np.array_equal(pixels[d], pixels_of_planes(p if p.shape[0] == 3 else p[0])), (name, d, "IPB"[t])
        want_sse, want_mx = distortion_of_planes(sd.original_planes(sd.array_of_pnm(frames[d])), p)
        assert [int(v) for v in sse[d]] == want_sse and [int(v) for v in mx[d]] == want_mx, (name, d, "IPB"[t], sse[d], mx[d])
    assert again[0] == stream and again[4].tolist() == [1] * len(frames)
    assert all(np.array_equal(a, b) for a, b in zip(again[1], pixels))
    assert np.array_equal(again[2], sse) and np.array_equal(again[3], mx)


# ------------------------------------------------------------------ shares and repeats

@pytest.mark.parametrize("name", vc.THREE_GOPS)
def test_three_groups_on_two_shares_and_a_second_call(gpu, tmp_path_factory, tmp_path, name):
    """The device listed twice: the groups of pictures are dealt over two shares.  dec_add16 adds the blocks of a frame
    with atomics in whatever order the waves arrive: no share, no earlier call and no order may show."""
    rec, stream, planes, _ = device_run(gpu, tmp_path_factory, name)
    frames, args, vp = vc.case_of(name)
    try:
        gpu.set_devices([0, 0])
        assert gpu.device_count() == 2
        stream2, planes2, counts2, msg = vc.run_library(gpu, frames, args, vp, tmp_path / "two")
    finally:
        gpu.set_devices([])
    assert stream2 is not None, msg
    vc.check_case(name, rec, stream2, planes2, counts2)
    stream3, planes3, _, msg = vc.run_library(gpu, frames, args, vp, tmp_path / "again")
    assert stream3 is not None, msg
    for s, p, whose in ((stream2, planes2, "two shares"), (stream3, planes3, "a second call")):
        assert rc.compare_runs(name, s, p, stream, planes, "the first call") == "", whose


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("name", list(vc.REFUSED))
def test_refused_patterns(gpu, tmp_path, name):
    """0, the message, an existing output file as it was; the device-memory entry refuses with the same message; the
    library codes the next video"""
    vc.refusal_leaves_the_output(gpu, name, tmp_path / "coder")
    frames, args, vp = vc.case_of(name)
    q, o = vc.open_options(gpu, args, vp)
    seq = fiasco_amd.Sequence.from_device(gpu, [to_gpu(sd.array_of_pnm(f)) for f in frames], q, o)
    with pytest.raises(fiasco_amd.FiascoError, match="Motion search without a reference frame"):
        seq.encode()
    seq.free(); o.delete()
    ok = "ib_x2_fps25_cross1_b0"
    frames, args, vp = vc.case_of(ok)
    stream, _, _, msg = vc.run_library(gpu, frames, args, vp, tmp_path / "next")
    assert stream is not None and hashlib.md5(stream).hexdigest() == vc.fixture()["cases"][ok]["stream_md5"], msg


# ------------------------------------------------------------------ random cases

def fuzz(gpu, oracle, seed, tmp):
    if seed not in _fuzz:
        _fuzz[seed] = vc.fuzz_seed(gpu, seed, tmp, oracle)
        print("video param fuzz device seed %d: %s %s%s" % ((seed,) + _fuzz[seed][:2] + ("" if _fuzz[seed][2] else " [no reference stream]",)))
    return _fuzz[seed]


@pytest.mark.parametrize("seed", vc.FUZZ_SEEDS)
def test_device_fuzz_against_the_oracle_and_the_live_reference_library(gpu, oracle, tmp_path, seed):
    """The device's stream and int16 planes equal the oracle's (a mismatch names the frame, its type, the band and the
    bounding box) and libfiasco_ref_recon.so's where that file is there and codes the case."""
    verdict, text, _ = fuzz(gpu, oracle, seed, tmp_path)
    assert verdict != "MISMATCH", text


def test_device_fuzz_compares_enough_seeds(gpu, oracle, tmp_path):
    """At least 18 of the 24 seeds compare against the oracle.  On the CPU the reference library codes 20 of them, and
    the oracle equals it on all 20; on the other four (colour) both end with "Can't write more than n weights"."""
    res = [fuzz(gpu, oracle, s, tmp_path) for s in vc.FUZZ_SEEDS]
    n = sum(1 for verdict, _, _ in res if verdict == "compared")
    print("video param fuzz device: %d of %d seeds compared with the oracle, %d of them with the reference library too"
          % (n, len(res), sum(1 for v, _, coded in res if v == "compared" and coded)))
    assert n >= vc.FUZZ_MIN_COMPARED, n
