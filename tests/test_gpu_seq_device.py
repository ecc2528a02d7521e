"""Videos from device memory; reconstructed frames and their distortion back into device memory -- run on a real
MI355X: -m gpu.  (include/libfiasco_amd_video.h: fiasco_amd_seq_open_device, fiasco_amd_seq_set_outputs_device;
csrc/hip/input_convert.inc, enc_stage.inc, frame_decoder.inc, output_convert.inc, distortion.inc.)

The yardsticks are the reference's: the stream md5 of tests/golden/RECONST.json / MANIFEST.json, the planes md5 of
RECONST.json, and tests/golden/RECONST_PIXELS.json -- per display frame the md5 of the 8-bit pixels of the reference
CODER's reconstructed planes and the exact distortion integers (tests/golden/make_reconst_pixels.py).  Everything is
compared with ==.  Frames are at most 256 pixels wide; a case takes well under a second on the device."""
import hashlib
import json
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch            # before the product library is loaded: one HIP runtime for both

import fiasco_amd
import reconst_cases as rc
import seq_device_cases as sd
import synth
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
NAMES = sd.names(MANIFEST)
IN_PLACE = [n for n in NAMES if n.startswith("shift100x70_") or n.startswith("gops_")]
COLOUR = [n for n in NAMES if sd.fixture()[n]["geometry"][2] == 3]
_runs = {}


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def sources(name, frames, planar=False):
    """-> (the frames as GPU tensors, the tensors to overwrite once the sequence is open).  The shift100x70_* and gops_*
    cases are windows of ONE 160 x 120 tensor, read in place: pitch 160, rows at byte offsets 20 + 3 i (not on 16 bytes),
    a width of 100 (no multiple of 16: the byte-load path and the ragged row end)."""
    arrays = [sd.array_of_pnm(f) for f in frames]
    if name in IN_PLACE:
        big = to_gpu(synth.synth(160, 120, 7))
        views = [big[10 + 2 * i:80 + 2 * i, 20 + 3 * i:120 + 3 * i] for i in range(len(frames))]
        for v, a in zip(views, arrays):
            assert v.stride(0) == 160 and not v.is_contiguous() and np.array_equal(v.cpu().numpy(), a)
        assert [(v.data_ptr() - big.data_ptr()) % 160 for v in views] == [20 + 3 * i for i in range(len(frames))]
        return views, [big]
    t = [to_gpu(a.transpose(2, 0, 1) if planar and a.ndim == 3 else a) for a in arrays]
    return t, t


def new_targets(geom, n):
    w, h, nb = geom
    return [torch.full((h, w, 3) if nb == 3 else (h, w), 7, dtype=torch.uint8, device="cuda") for _ in range(n)]


def md5_of(t):
    torch.cuda.synchronize()
    return hashlib.md5(t.contiguous().cpu().numpy().tobytes()).hexdigest()


def run(gpu, manifest, inputs, name, fed="device", planar=False, targets=True, distortion=True, keep=False, encodes=1, cache=True):
    """one sequence through the device -> dict(stream, pixels=[md5], sse, maxdiff, written, planes, researched)"""
    key = (name, fed, planar, targets, distortion, keep, encodes)
    if cache and key in _runs:
        return _runs[key]
    frames, args, _ = sd.case_of(manifest, inputs, name)
    geom = rc.geometry(frames)
    q, o = sd.open_options(gpu, args)
    if fed == "device":
        src, wipe = sources(name, frames, planar)
        seq = fiasco_amd.Sequence.from_device(gpu, src, q, o)
        for t in wipe:
            t.zero_()               # right after open, in stream order: the planes were converted before
    else:
        seq = fiasco_amd.Sequence(gpu, frames, q, o)
    tg = new_targets(geom, len(frames)) if targets is True else targets
    if tg is not None or distortion:
        seq.set_outputs(tg, distortion)
    if keep:
        seq.keep_reconstructed()
    out = {"researched": False}
    for _ in range(encodes):
        guess = seq.probe()
        out["stream"] = seq.encode()
        left = [seq.gop_result(g)[0] for g in range(seq.gops)]
        # every GOP behind the first started from the probe's guess: one that follows a GOP which left another level was
        # searched a second time (fa_seq_encode_all)
        out["researched"] = out["researched"] or any(left[g - 1] != guess for g in range(1, seq.gops))
        if tg is not None or distortion:
            out["sse"], out["maxdiff"], out["written"] = seq.distortion()
        if tg is not None:
            out["pixels"] = [None if t is None else md5_of(t) for t in tg]
        if keep:
            out["planes"] = [seq.reconstructed_planes(d) for d in range(len(frames))]
        out.setdefault("first", dict(out))
    seq.free(); o.delete()
    out["targets"] = tg
    if cache:
        _runs[key] = out
    return out


def check_outputs(name, got, frames_wanted=None):
    rec = sd.fixture()[name]
    for f in rec["frames"]:
        d = f["display"]
        if frames_wanted is not None and d not in frames_wanted:
            continue
        if got.get("pixels") is not None and got["pixels"][d] is not None:
            assert got["pixels"][d] == f["pixels_md5"], (name, d, "IPB"[f["type"]])
        if got.get("sse") is not None:
            assert [int(v) for v in got["sse"][d]] == f["sse"], (name, d, "IPB"[f["type"]], got["sse"][d])
            assert [int(v) for v in got["maxdiff"][d]] == f["maxdiff"], (name, d, "IPB"[f["type"]], got["maxdiff"][d])


# ------------------------------------------------------------------ streams

@pytest.mark.parametrize("name", NAMES)
def test_device_fed_video_gives_the_references_stream_frames_and_distortion(gpu, manifest, inputs, name):
    """Fed from device memory (gray H x W, colour interleaved; the sources zeroed right after open), with targets,
    distortion and kept planes: the reference's stream; every display frame -- B frames, the last frame of every group,
    the frames of the all-intra pair -- as the fixture's pixels and integers; the planes of RECONST.json with no
    directory knob set."""
    assert "FIASCO_AMD_SEQ_RECONST_DIR" not in os.environ
    frames, _, md5 = sd.case_of(manifest, inputs, name)
    got = run(gpu, manifest, inputs, name, keep=True)
    assert hashlib.md5(got["stream"]).hexdigest() == md5
    assert got["written"].tolist() == [1] * len(frames)
    check_outputs(name, got)
    if name in rc.fixture():
        for f in rc.fixture()[name]["frames"]:
            p, t = got["planes"][f["display"]]
            assert t == f["type"] and rc.planes_md5(p) == f["planes_md5"], (name, f["display"])


@pytest.mark.parametrize("name", COLOUR)
def test_planar_colour_sources_give_the_same_stream(gpu, manifest, inputs, name):
    """every colour case a second time, as 3 x H x W planes"""
    frames, _, md5 = sd.case_of(manifest, inputs, name)
    assert rc.geometry(frames)[2] == 3
    got = run(gpu, manifest, inputs, name, planar=True, targets=None, distortion=False)
    assert hashlib.md5(got["stream"]).hexdigest() == md5


# ------------------------------------------------------------------ outputs

@pytest.mark.parametrize("name", NAMES)
def test_pnm_fed_video_delivers_the_same_outputs(gpu, manifest, inputs, name):
    """fiasco_amd_seq_open + set_outputs: the original is copied into the flight's arena from the step's parsed image"""
    frames, _, md5 = sd.case_of(manifest, inputs, name)
    got = run(gpu, manifest, inputs, name, fed="pnm")
    assert hashlib.md5(got["stream"]).hexdigest() == md5
    assert got["written"].tolist() == [1] * len(frames)
    check_outputs(name, got)


def test_the_frame_kinds_the_search_used_to_skip_are_covered():
    fx = sd.fixture()
    assert [f["type"] for f in fx["seq4_gray_ibbp"]["frames"]] == [0, 2, 2, 1]
    assert [f["type"] for f in fx["seq4_gray_ipbb"]["frames"]] == [0, 1, 2, 1]           # the last frame forced to P
    assert [f["type"] for f in fx["gops_ibpi"]["frames"]] == [0, 2, 1, 0, 0, 1]
    assert {"sat_q60_ibp", "blend_q60_ibp", "seed9018"} <= set(fx)
    assert all(f["type"] == 0 for n in sd.CARRY for f in fx[n]["frames"])


@pytest.mark.parametrize("name", sd.CARRY)
def test_a_group_searched_twice_leaves_the_outputs_of_the_final_stream(gpu, manifest, inputs, name):
    """The all-intra pair: three groups of pictures each.  A group whose speculated minimum level was wrong is searched
    again and overwrites its frames; what the arrays hold after the last search belongs to the stream that is written.
    With the probe's guess neither sequence needs a second search (measured with the CPU oracle: carry48 starts at 4, the
    probe says 4, the groups leave 4, 4, 4; carry74: 6, 6 and 6, 6, 6 -- the `carry' of their names is the y_column one),
    so the wrong speculation is made by hand, the way a driver meets it: the first sweep starts the groups 1 and 2 one
    level too high, the chain is verified from gop_result as fa_seq_encode_all and sharding.py verify it, and the groups
    behind the first wrong start are searched again."""
    frames, args, md5 = sd.case_of(manifest, inputs, name)
    fx = sd.fixture()[name]["frames"]
    q, o = sd.open_options(gpu, args)
    src, wipe = sources(name, frames)
    seq = fiasco_amd.Sequence.from_device(gpu, src, q, o)
    for t in wipe:
        t.zero_()
    tg = new_targets(rc.geometry(frames), 3)
    seq.set_outputs(tg, True)
    guess = seq.probe()
    carry, todo, searches = [seq.initial_level, guess + 1, guess + 1], [True] * 3, []
    for sweep in range(3):
        seq.search(carry, todo)
        searches.append(list(todo))
        sse, mx, wr = seq.distortion()
        assert wr.tolist() == [1, 1, 1]
        pix = [md5_of(t) for t in tg]
        if sweep == 0:
            first = pix
        t, first_invalid = seq.initial_level, 3
        for g in range(3):
            if carry[g] != t:
                first_invalid = g
                break
            left, failed, _ = seq.gop_result(g)
            assert not failed
            t = left
        if first_invalid == 3:
            break
        todo = [g >= first_invalid for g in range(3)]
        carry = [t if todo[g] else carry[g] for g in range(3)]
    assert searches == [[True, True, True], [False, True, True]], "a second search of the groups 1 and 2 was expected"
    assert first[0] == fx[0]["pixels_md5"] and first[1] != fx[1]["pixels_md5"] and first[2] != fx[2]["pixels_md5"]
    check_outputs(name, {"pixels": pix, "sse": sse, "maxdiff": mx})
    assert hashlib.md5(seq.encode()).hexdigest() == md5           # the stream these frames belong to
    got = {"pixels": [md5_of(t) for t in tg]}
    got["sse"], got["maxdiff"], wr = seq.distortion()
    assert wr.tolist() == [1, 1, 1]
    check_outputs(name, got)
    seq.free(); o.delete()


def test_target_and_output_variants(gpu, manifest, inputs):
    """targets with a pitch, cut out of a larger tensor; no target for some frames; targets alone; distortion alone"""
    name = "shift100x70_ibbp"
    frames, _, md5 = sd.case_of(manifest, inputs, name)
    fx = sd.fixture()[name]["frames"]
    big = torch.full((4, 90, 131), 9, dtype=torch.uint8, device="cuda")
    cut = [big[i, 3:73, 17:117] for i in range(4)]
    got = run(gpu, manifest, inputs, name, targets=cut, distortion=True, cache=False)
    assert hashlib.md5(got["stream"]).hexdigest() == md5 and got["written"].tolist() == [1, 1, 1, 1]
    check_outputs(name, got)
    frame = big.clone()
    frame[:, 3:73, 17:117] = 9
    assert torch.equal(frame, torch.full_like(big, 9)), "bytes outside the targets were written"
    some = new_targets((100, 70, 1), 4)
    some[0] = some[3] = None
    got = run(gpu, manifest, inputs, name, targets=some, distortion=False, cache=False)
    assert got["written"].tolist() == [0, 1, 1, 0] and got["sse"] is None
    assert got["pixels"][1] == fx[1]["pixels_md5"] and got["pixels"][2] == fx[2]["pixels_md5"]
    got = run(gpu, manifest, inputs, name, fed="pnm", targets=some, distortion=True, cache=False)
    assert got["written"].tolist() == [1, 1, 1, 1]          # measured, not written
    check_outputs(name, got)
    got = run(gpu, manifest, inputs, name, targets=None, distortion=True, cache=False)
    assert got["written"].tolist() == [1, 1, 1, 1] and "pixels" not in got
    check_outputs(name, got)


# ------------------------------------------------------------------ shares, ranks, a second call

@pytest.mark.parametrize("name", rc.MULTI_GOP)
def test_groups_of_pictures_on_two_shares_of_one_device(gpu, manifest, inputs, name):
    one = run(gpu, manifest, inputs, name, keep=True)
    try:
        gpu.set_devices([0, 0])
        assert gpu.device_count() == 2
        two = run(gpu, manifest, inputs, name, keep=True, cache=False)
    finally:
        gpu.set_devices([])
    assert two["stream"] == one["stream"] and two["pixels"] == one["pixels"]
    assert np.array_equal(two["sse"], one["sse"]) and np.array_equal(two["maxdiff"], one["maxdiff"])
    assert two["written"].tolist() == [1] * 6
    check_outputs(name, two)


def test_two_ranks_in_one_process_write_only_their_own_groups(gpu, manifest, inputs):
    name = "gops_ibpi"
    frames, args, md5 = sd.case_of(manifest, inputs, name)
    whole = run(gpu, manifest, inputs, name, keep=True)
    q, o = sd.open_options(gpu, args)
    parts, written, pieces = [], [], {}
    for rank in range(2):
        src, wipe = sources(name, frames)
        seq = fiasco_amd.Sequence.from_device(gpu, src, q, o, rank, 2)
        for t in wipe:
            t.zero_()
        tg = new_targets(rc.geometry(frames), len(frames))
        seq.set_outputs(tg, True)
        seq.search([seq.initial_level] * seq.gops, [True] * seq.gops)
        sse, mx, wr = seq.distortion()
        for k in range(seq.frames):
            if seq.gop_of(k) % 2 == rank:
                pieces[k] = seq.write(k)
        parts.append((sse, mx, [md5_of(t) for t in tg]))
        written.append(wr)
        seq.free()
    o.delete()
    assert hashlib.md5(b"".join(pieces[k] for k in sorted(pieces))).hexdigest() == md5 and len(pieces) == 6
    # display frames 0 1 2 | 3 | 4 5 are the groups 0 | 1 | 2: rank 0 has groups 0 and 2, rank 1 group 1
    assert written[0].tolist() == [1, 1, 1, 0, 1, 1] and written[1].tolist() == [0, 0, 0, 1, 0, 0]
    untouched = hashlib.md5(bytes([7]) * 7000).hexdigest()
    for d in range(6):
        r = 0 if written[0][d] else 1
        sse, mx, pix = parts[r]
        assert pix[d] == whole["pixels"][d] and parts[1 - r][2][d] == untouched
        assert np.array_equal(sse[d], whole["sse"][d]) and np.array_equal(mx[d], whole["maxdiff"][d])
        assert not parts[1 - r][0][d].any()


@pytest.mark.parametrize("name", ["sat_q60_ibp", "gops_ibpi"])
def test_a_second_encode_gives_identical_outputs(gpu, manifest, inputs, name):
    """dec_add16 adds in arrival order into fresh planes: nothing of the first call, and no order, may show"""
    got = run(gpu, manifest, inputs, name, keep=True, encodes=2, cache=False)
    first = got["first"]
    assert got["stream"] == first["stream"] and got["pixels"] == first["pixels"]
    assert np.array_equal(got["sse"], first["sse"]) and np.array_equal(got["maxdiff"], first["maxdiff"])
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(got["planes"], first["planes"]))
    check_outputs(name, got)


def test_host_planes_of_a_device_fed_frame_come_on_demand(gpu, manifest, inputs):
    """keep_reconstructed on a device-fed sequence alone (no outputs): the planes of RECONST.json"""
    name = "seq4_gray_ipbb"
    got = run(gpu, manifest, inputs, name, targets=None, distortion=False, keep=True)
    for f in rc.fixture()[name]["frames"]:
        p, t = got["planes"][f["display"]]
        assert t == f["type"] and rc.planes_md5(p) == f["planes_md5"]


# ------------------------------------------------------------------ refusals (all before any launch)

class HostArray:
    """host memory behind the interface of a GPU array"""
    def __init__(self, a):
        self.a = a
        self.__cuda_array_interface__ = {"shape": a.shape, "typestr": "|u1", "data": (a.ctypes.data, False), "version": 3, "strides": None}


def test_refusals_leave_everything_usable(gpu, manifest, inputs):
    name = "seq4_gray_ibbp"
    frames, args, md5 = sd.case_of(manifest, inputs, name)
    q, o = sd.open_options(gpu, args)
    good = [to_gpu(sd.array_of_pnm(f)) for f in frames]
    h, w = good[0].shape
    for bad, why in (([HostArray(np.zeros((h, w), np.uint8))] + good[1:], "not in device memory"),
                     (good[:2] + [good[2][:h - 2]] + good[3:], "have to be of the same size"),
                     (good[:3] + [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")], "color model"),
                     ([], "No frames")):
        with pytest.raises(fiasco_amd.FiascoError, match=why):
            fiasco_amd.Sequence.from_device(gpu, bad, q, o)
    seq = fiasco_amd.Sequence.from_device(gpu, good, q, o)
    ok = new_targets((w, h, 1), 4)
    for bad, why in ((ok[:3] + [torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")], "contradicts the colour model"),
                     (ok[:1] + [torch.zeros((h, w + 2), dtype=torch.uint8, device="cuda")] + ok[2:], "pixels for a frame of"),
                     (ok[:2] + [HostArray(np.zeros((h, w), np.uint8))] + ok[3:], "not in device memory")):
        with pytest.raises(fiasco_amd.FiascoError, match=why):
            seq.set_outputs(bad, True)
        with pytest.raises(fiasco_amd.FiascoError, match="no outputs are set"):
            seq.distortion()                        # nothing was set
    with pytest.raises(fiasco_amd.FiascoError, match="targets for a sequence"):
        seq.set_outputs(ok[:3])
    assert hashlib.md5(seq.encode()).hexdigest() == md5
    seq.set_outputs(ok, True)
    assert hashlib.md5(seq.encode()).hexdigest() == md5
    got = {"pixels": [md5_of(t) for t in ok]}
    got["sse"], got["maxdiff"], got["written"] = seq.distortion()
    assert got["written"].tolist() == [1, 1, 1, 1]
    check_outputs(name, got)
    seq.set_outputs()                               # none again
    assert hashlib.md5(seq.encode()).hexdigest() == md5
    seq.free(); o.delete()


def test_encode_sequence_device_of_the_sharding_module(gpu, manifest, inputs):
    """the driver of sharding.encode_sequence on a device-fed sequence (one rank)"""
    from fiasco_amd import sharding
    name = "seq3_color_ibp"
    frames, args, md5 = sd.case_of(manifest, inputs, name)
    q, o = sd.open_options(gpu, args)
    src, _ = sources(name, frames)
    tg = new_targets(rc.geometry(frames), len(frames))
    assert hashlib.md5(sharding.encode_sequence_device(gpu, src, q, o)).hexdigest() == md5
    data, (sse, mx, wr) = sharding.encode_sequence_device(gpu, src, q, o, targets=tg, distortion=True)
    o.delete()
    assert hashlib.md5(data).hexdigest() == md5 and wr.tolist() == [1, 1, 1]
    check_outputs(name, {"pixels": [md5_of(t) for t in tg], "sse": sse, "maxdiff": mx})
