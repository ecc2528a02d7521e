"""The reconstructed frames of a video -- what the coder predicts the next P or B frame from (decode_image +
restore_mc, reference codec/coder.c:647-651) -- of the CPU oracle against the REFERENCE CODER's own frames.

tests/golden/RECONST.json holds, per case and frame, the md5 of the planes that cfiasco_ref_recon wrote (the reference
coder with one block added that writes reconst->pixels[], oracle/ref_build.sh; tests/golden/make_reconst.py).  The
oracle writes its planes through FIASCO_AMD_SEQ_RECONST_DIR of the sequence engine, the last frame of every group of
pictures included, which no later frame is predicted from and which stream parity therefore never sees, like every B
frame.  tests/reconst_cases.py has the cases and says why `dfiasco` is not the yardstick here.
tests/test_gpu_reconst.py runs the same pins on the device.
"""
import json
import os

import pytest

import reconst_cases as rc
from conftest import GOLDEN

NAMES = rc.pinned_names(json.load(open(os.path.join(GOLDEN, "MANIFEST.json"))))
_runs = {}


def oracle_run(oracle, manifest, inputs, tmp_path_factory, name):
    """one oracle run per pinned case and session -> (fixture record, stream, planes, counts)"""
    if name not in _runs:
        frames, args = rc.case_of(manifest, inputs, name)
        rec = rc.fixture()[name]
        assert rc.inputs_md5(frames) == rec["inputs_md5"] and args == rec["args"], "the inputs of %s changed" % name
        stream, planes, counts, msg = rc.run_library(oracle, frames, args, tmp_path_factory.mktemp("reconst_" + name))
        assert stream is not None, "%s: %s" % (name, msg)
        _runs[name] = (rec, stream, planes, counts)
    return _runs[name]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reconstructed_frames_equal_the_reference_coders(oracle, manifest, inputs, tmp_path_factory, name):
    rc.check_against_fixture(name, *oracle_run(oracle, manifest, inputs, tmp_path_factory, name))


def test_the_pinned_set_is_not_hollow(oracle, manifest, inputs, tmp_path_factory):
    rc.check_not_hollow([oracle_run(oracle, manifest, inputs, tmp_path_factory, n) for n in NAMES])


def test_the_fixture_records_where_the_reference_decoder_drifts():
    """dfiasco is not the yardstick of these frames.  The record, not a judgement of either program:
    it never differs on an I frame, it differs on P / B frames of five pinned seeds and dies on two."""
    fx = rc.fixture()
    assert sorted(fx) == sorted(NAMES)
    drift, dead = set(), set()
    for name, rec in fx.items():
        for f in rec["frames"]:
            if f["dfiasco_equal"] is None:
                dead.add(name)
            elif not f["dfiasco_equal"]:
                assert f["type"] != 0, (name, f)
                drift.add(name)
    assert drift == {"seed9003", "seed9004", "seed9007", "seed9009", "seed9011"} and dead == {"seed9018", "seed9022"}


def test_oracle_fuzz_against_the_live_reference_coder(oracle, tmp_path):
    """Streams equal, and every frame's planes equal, the last of each group of pictures included.  A seed is left
    out only where both coders fail or where the reference crashes or refuses."""
    if not os.path.exists(rc.CFIASCO_RECON):
        pytest.skip("cfiasco_ref_recon is not built (oracle/ref_build.sh needs the reference's sources)")
    n = rc.run_fuzz("oracle", oracle, tmp_path)
    print("reconst fuzz oracle: %d of %d seeds compared" % (n, len(rc.FUZZ_SEEDS)))
    assert n >= rc.FUZZ_MIN_COMPARED, n
