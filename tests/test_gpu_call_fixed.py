"""The part of a matching-pursuit call that does not depend on its candidates: the log2 tables of the rate models
(mp_tables, csrc/hip/mp_device.inc) are written by ONE path for every role -- the role of a lane is a chain of selects
(csrc/hip/mp_roles.h), every operand is read whatever the role, one division, one logarithm, destinations chosen by
select.  No value changes: the streams must be the reference's, build by build, and every approximate_range record the
oracle's.

Host (no GPU): the select chain against the nested-if mapping it replaces (tests/mp_roles_check.cpp).
GPU: goldens through the 256-thread, 1024-thread, triangular-table and speculating builds; model sizes that move the
single roles (sy = 64: they start at lane 128, in the third wave; sy = 8, dcs = 8 and 16: the smallest); one traced frame.

The recorded streams of the model-size cases come from "cases" and "oracle_cases" of the manifest (both written by the
real reference): its "option_cases" hold mantissas 6 .. 8 only, which run the FC_HM form of mp_tables, not this one."""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"narrow": {"FIASCO_AMD_NO_WIDE": "1", "FIASCO_AMD_SPEC": "0"}, "wide": {"FIASCO_AMD_SPEC": "0"},
          "wide_tri": {"FIASCO_AMD_FORCE_TRI": "1"}, "spec": {}}
SWITCHES = ("FIASCO_AMD_NO_WIDE", "FIASCO_AMD_SPEC", "FIASCO_AMD_FORCE_TRI")


def test_role_selects_equal_the_nested_if_mapping(tmp_path):
    """(tid, dcs, sy, ctx, band, half_nd, half_dc) -> (kind, ci, ti, destination): every tid < 256, dcs and sy 1 .. 64,
    ctx 0 .. 4, both values of band, default and big role set."""
    exe = str(tmp_path / "mp_roles_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "fiasco_amd", "csrc", "hip"),
                        "-o", exe, os.path.join(ROOT, "tests", "mp_roles_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "mp_roles_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


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


def _case(manifest, name):
    return [c for c in manifest["cases"] + manifest["oracle_cases"] if c["name"] == name][0]


@pytest.mark.gpu
@pytest.mark.parametrize("build", list(BUILDS))
@pytest.mark.parametrize("name", ["g256_q20", "c256_q20"])
def test_goldens_build_by_build(gpu, manifest, inputs, tmp_path, monkeypatch, name, build):
    """g256_q20 and the smallest colour golden (256 x 192; its chroma bands keep the set-up of a call on lane 0 and have
    no placeholder-price roles) through each build of the default geometry: the reference's streams."""
    from conftest import encode_case
    _select(monkeypatch, build)
    case = _case(manifest, name)
    gpu.reset_stats()
    data = encode_case(gpu, case, inputs, tmp_path)
    assert data is not None, gpu.error_message()
    assert len(data) == case["bytes"] and hashlib.md5(data).hexdigest() == case["md5"]
    st = gpu.get_stats()
    by = list(st.frames_by_build)               # 256, 1024, big 256, big 512, 1024 triangular
    assert by[2] + by[3] == 0, by               # a build of the default geometry
    if build == "spec":
        assert st.spec_frames >= 1
    else:
        assert by[{"narrow": 0, "wide": 1, "wide_tri": 4}[build]] >= 1, by


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["narrow", "wide"])
@pytest.mark.parametrize("name", ["g256_rpf", "o_g256_m5", "o_g256_m2", "o_g256_dm3", "seq3_color_carry74"])
def test_model_sizes_that_move_the_single_roles(gpu, manifest, inputs, tmp_path, monkeypatch, name, build):
    """256 x 256 gray at --rpf-mantissa 4 (g256_rpf: sy = 32, the largest the 256-thread build takes; single roles from
    lane 96), 5 (sy = 64: single roles from lane 128 on, the roles end in the third wave; 5 x 64 + 64 counters are the big
    build's), 2 (sy = 8, the smallest), --dc-rpf-mantissa 3 (dcs = 16) and a colour sequence at --dc-rpf-mantissa 2
    (dcs = 8, the smallest): the streams the reference wrote."""
    from conftest import encode_case
    _select(monkeypatch, build)
    case = _case(manifest, name)
    data = encode_case(gpu, case, inputs, tmp_path)
    assert data is not None, gpu.error_message()
    assert len(data) == case["bytes"] and hashlib.md5(data).hexdigest() == case["md5"]


TRACE = [('seq', 'i4'), ('level', 'i4'), ('image', 'i4'), ('D', 'i4'), ('states', 'i4'), ('nedges', 'i4'), ('cost', 'f4'),
         ('err', 'f4'), ('mbits', 'f4'), ('wbits', 'f4'), ('into', 'i2', 6), ('w', 'f4', 5)]


@pytest.fixture(scope="module")
def traced_frame(oracle, tmp_path_factory):
    """one 128 x 128 frame, the oracle's stream and its record of every approximate_range call"""
    import numpy as np
    import synth
    img = synth.pgm_bytes(synth.synth(128, 128, 77))
    path = str(tmp_path_factory.mktemp("call_fixed") / "ora.trace")
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
@pytest.mark.parametrize("build", ["narrow", "wide", "spec"])
def test_every_call_of_a_small_frame_equals_the_oracles_record(gpu, traced_frame, tmp_path, monkeypatch, build):
    """costs, error, matrix and weight bits as raw floats, chosen states and quantised weights of every
    approximate_range call: bit for bit the oracle's"""
    import numpy as np
    img, exp, want = traced_frame
    _select(monkeypatch, build)
    tg = str(tmp_path / "gpu.trace")
    monkeypatch.setenv("FIASCO_AMD_TRACE", tg)
    o = gpu.cli_options()
    got = gpu.encode_batch([img], 20.0, o)[0]
    o.delete()
    assert got is not None, gpu.error_message()
    assert got == exp
    a = np.fromfile(tg, np.dtype(TRACE))
    assert len(a) == len(want) > 100
    assert a.tobytes() == want.tobytes(), "first differing record: %d" % next(
        i for i in range(len(a)) if a[i].tobytes() != want[i].tobytes())
