"""The level recursion of the <sub-block, state> tables works on items, not states (op_ipis_t in csrc/hip/fc_tables.inc,
FC_IPT builds; the mapping is csrc/hip/ipt_layout.h): where a level has 8 or more slots in the call's subtree, cnt / 4
neighbouring lanes serve one state, one group of four slots each, exchange their results inside the quad and store the
state's row of the level's table in 16-byte pieces.  Same sources, same additions in the same order: the streams must be
the reference's under the 256-thread, the 1024-thread and the triangular build, and every approximate_range record
the oracle's.

The host side of it (coverage, lane groups, alignment, the simulated exchange) is tests/test_ipis_items_host.py.

Cases: 32 x 32 and 64 x 32 (block levels below 8: one lane per state only, rows of 8 and 16 bytes), 100 x 70 (ragged
borders), 128 x 96 noise and 256 x 256 (whole blocks of level 10: 4 and 2 lanes per state; subtree calls after appends
with a first state above 0 and a non-zero address), 512 x 512 noise (1012 states: several items per lane, and a last
wave with part of its lane groups idle), a two-frame gray sequence, and the smallest colour golden (sparse chroma blocks
beside the new path)."""
import hashlib
import os

import pytest

BUILDS = {"narrow": {"FIASCO_AMD_NO_WIDE": "1", "FIASCO_AMD_SPEC": "0"}, "wide": {"FIASCO_AMD_SPEC": "0"},
          "wide_tri": {"FIASCO_AMD_FORCE_TRI": "1"}}
SLOT = {"narrow": 0, "wide": 1, "wide_tri": 4}      # frames_by_build: 256, 1024, big 256, big 512, 1024 triangular
SWITCHES = ("FIASCO_AMD_NO_WIDE", "FIASCO_AMD_SPEC", "FIASCO_AMD_FORCE_TRI")
CASES = ["g32x32_q20", "g64x32_q20", "g100x70_q20", "n128x96_q20", "g256_q20", "n512_q20", "seq2_gray_i", "c256_q20"]


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def _select(monkeypatch, build):
    monkeypatch.setenv("FIASCO_AMD_DEBUG", "1")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in BUILDS[build].items():
        monkeypatch.setenv(k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", CASES)
def test_reference_streams_build_by_build(gpu, manifest, inputs, tmp_path, monkeypatch, name, build):
    """bytes and md5 of the manifest, through the build that was asked for and no other"""
    from conftest import encode_case
    _select(monkeypatch, build)
    case = [c for c in manifest["cases"] if c["name"] == name][0]
    gpu.reset_stats()
    data = encode_case(gpu, case, inputs, tmp_path)
    assert data is not None, gpu.error_message()
    assert len(data) == case["bytes"] and hashlib.md5(data).hexdigest() == case["md5"]
    st = gpu.get_stats()
    by = list(st.frames_by_build)
    print("%s %s: frames_by_build %s, states_max %d" % (name, build, by, st.states_max))
    assert by[SLOT[build]] >= len(case["inputs"]) and sum(by) == by[SLOT[build]] and st.spec_frames == 0, (by, st.spec_frames)
    if name == "n512_q20":
        assert st.states_max > 256, st.states_max       # several items per lane, idle lane groups in the last wave


TRACE = [('seq', 'i4'), ('level', 'i4'), ('image', 'i4'), ('D', 'i4'), ('states', 'i4'), ('nedges', 'i4'), ('cost', 'f4'),
         ('err', 'f4'), ('mbits', 'f4'), ('wbits', 'f4'), ('into', 'i2', 6), ('w', 'f4', 5)]


@pytest.fixture(scope="module")
def traced_frame(oracle, tmp_path_factory):
    """one 128 x 128 frame (seed 77), the oracle's stream and its record of every approximate_range call"""
    import numpy as np
    import synth
    img = synth.pgm_bytes(synth.synth(128, 128, 77))
    path = str(tmp_path_factory.mktemp("ipis_items") / "ora.trace")
    old = os.environ.get("FIASCO_ORACLE_TRACE")
    os.environ["FIASCO_ORACLE_TRACE"] = path
    try:
        o = oracle.cli_options()
        exp = oracle.encode_batch([img], 20.0, o)[0]
        o.delete()
    finally:
        if old is None:
            del os.environ["FIASCO_ORACLE_TRACE"]
        else:
            os.environ["FIASCO_ORACLE_TRACE"] = old
    assert exp is not None
    return img, exp, np.fromfile(path, np.dtype(TRACE))


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
def test_every_call_of_a_small_frame_equals_the_oracles_record(gpu, traced_frame, tmp_path, monkeypatch, build):
    """costs, error, matrix and weight bits as raw floats, chosen states and quantised weights of every
    approximate_range call: bit for bit the oracle's"""
    import numpy as np
    img, exp, want = traced_frame
    _select(monkeypatch, build)
    tg = str(tmp_path / "gpu.trace")
    monkeypatch.setenv("FIASCO_AMD_TRACE", tg)
    gpu.reset_stats()
    o = gpu.cli_options()
    got = gpu.encode_batch([img], 20.0, o)[0]
    o.delete()
    assert got is not None, gpu.error_message()
    assert got == exp
    by = list(gpu.get_stats().frames_by_build)
    assert by[SLOT[build]] == 1 and sum(by) == 1, by
    a = np.fromfile(tg, np.dtype(TRACE))
    assert len(a) == len(want) > 100
    assert a.tobytes() == want.tobytes(), "first differing record: %d" % next(
        i for i in range(len(a)) if a[i].tobytes() != want[i].tobytes())
