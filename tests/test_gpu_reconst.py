"""The reconstructed frames of a video on the device -- run on a real MI355X: -m gpu.

The frame the next P or B frame is predicted from is decoded on the device (frame_decoder.inc: the level launches,
dec_assemble_kernel, then dec_mc_kernel with dec_add16 and dec_clip_chroma_kernel, the restatement of decode_image +
restore_mc, reference codec/coder.c:647-651).  Stream parity sees such a frame only through the frames predicted from
it: never a B frame, never the last frame of a group of pictures.  Here every frame is compared directly:
  * with the REFERENCE CODER's own planes, as md5 sums of tests/golden/RECONST.json (cases: tests/reconst_cases.py);
  * on random sequences with the CPU oracle's planes as int16 arrays, and with the live reference coder's where
    oracle/_ref/cfiasco_ref_recon is there;
  * with itself: the device listed twice, a second call.
Frames are at most 256 pixels wide; every case takes well under a second on the device.
"""
import json
import os

import numpy as np
import pytest

import reconst_cases as rc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

NAMES = rc.pinned_names(json.load(open(os.path.join(GOLDEN, "MANIFEST.json"))))
GROUPS = 4
_runs = {}
_tally = {}


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def device_run(gpu, manifest, inputs, tmp_path_factory, name):
    """one device run per pinned case and session -> (fixture record, stream, planes, counts)"""
    if name not in _runs:
        frames, args = rc.case_of(manifest, inputs, name)
        rec = rc.fixture()[name]
        assert rc.inputs_md5(frames) == rec["inputs_md5"] and args == rec["args"], "the inputs of %s changed" % name
        stream, planes, counts, msg = rc.run_library(gpu, frames, args, tmp_path_factory.mktemp("reconst_" + name))
        assert stream is not None, "%s: %s" % (name, msg)
        _runs[name] = (rec, stream, planes, counts)
    return _runs[name]


@pytest.mark.parametrize("name", NAMES)
def test_device_reconstructed_frames_equal_the_reference_coders(gpu, manifest, inputs, tmp_path_factory, name):
    """stream md5 and the md5 of every frame's planes, B frames and the last frame of every group included"""
    rc.check_against_fixture(name, *device_run(gpu, manifest, inputs, tmp_path_factory, name))


def test_the_pinned_set_is_not_hollow_on_the_device(gpu, manifest, inputs, tmp_path_factory):
    rc.check_not_hollow([device_run(gpu, manifest, inputs, tmp_path_factory, n) for n in NAMES])


def fuzz_group(gpu, oracle, group, tmp):
    if group not in _tally:
        per = len(rc.FUZZ_SEEDS) // GROUPS
        _tally[group] = rc.run_fuzz("device", gpu, tmp, rc.FUZZ_SEEDS[group * per:(group + 1) * per], yardstick=oracle)
    return _tally[group]


@pytest.mark.parametrize("group", range(GROUPS))
def test_device_fuzz_against_the_oracle_and_the_live_reference_coder(gpu, oracle, tmp_path, group):
    """Seeds 9000 .. 9023, six per case: the device's stream and planes equal the oracle's (int16 arrays; a mismatch
    names the frame, its type, the band and the bounding box) and cfiasco_ref_recon's where that binary is there."""
    fuzz_group(gpu, oracle, group, tmp_path)


def test_device_fuzz_compares_enough_seeds(gpu, oracle, tmp_path):
    n = sum(fuzz_group(gpu, oracle, g, tmp_path) for g in range(GROUPS))
    print("reconst fuzz device: %d of %d seeds compared" % (n, len(rc.FUZZ_SEEDS)))
    assert n >= rc.FUZZ_MIN_COMPARED, n


@pytest.mark.parametrize("name", rc.MULTI_GOP)
def test_groups_of_pictures_on_two_shares_of_one_device(gpu, manifest, inputs, tmp_path_factory, tmp_path, name):
    """The device listed twice: the groups of pictures are dealt over two shares, and a group's reference frames are
    decoded on the share that searches it.  Same stream, same planes."""
    rec, stream, planes, _ = device_run(gpu, manifest, inputs, tmp_path_factory, name)
    frames, args = rc.case_of(manifest, inputs, name)
    try:
        gpu.set_devices([0, 0])
        assert gpu.device_count() == 2
        stream2, planes2, counts2, msg = rc.run_library(gpu, frames, args, tmp_path)
    finally:
        gpu.set_devices([])
    assert stream2 is not None, msg
    rc.check_against_fixture(name, rec, stream2, planes2, counts2)
    assert rc.compare_runs(name, stream2, planes2, stream, planes, "one share") == ""


@pytest.mark.parametrize("name", ["shift100x70_ibbp_lv67", "sat_q60_ibp", "gops_ibpi"])
def test_a_second_call_gives_the_same_planes(gpu, manifest, inputs, tmp_path_factory, tmp_path, name):
    """dec_add16 adds the blocks of a frame with atomics in whatever order the waves arrive, into planes the call
    allocates: nothing of an earlier call, and no order, may show."""
    rec, stream, planes, _ = device_run(gpu, manifest, inputs, tmp_path_factory, name)
    frames, args = rc.case_of(manifest, inputs, name)
    stream2, planes2, counts2, msg = rc.run_library(gpu, frames, args, tmp_path)
    assert stream2 is not None, msg
    assert rc.compare_runs(name, stream2, planes2, stream, planes, "the first call") == ""
    assert all(np.array_equal(planes[d][1], planes2[d][1]) for d in planes)
