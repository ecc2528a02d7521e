"""Videos from device memory, their reconstructed frames and distortion (fiasco_amd_seq_open_device,
fiasco_amd_seq_set_outputs_device, fiasco_amd_seq_encode / _keep_reconstructed / _reconstructed_planes): what can be
checked without a GPU.  The device side is tests/test_gpu_seq_device.py (-m gpu).

The three host outlets work in the CPU oracle too, so the oracle pins them here: Sequence.encode() against
fiasco_coder(), the kept planes against the reference coder's (tests/golden/RECONST.json), and through them
tests/golden/RECONST_PIXELS.json, the fixture of the device outputs."""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import fiasco_amd
import reconst_cases as rc
import seq_device_cases as sd
from conftest import GOLDEN, encode_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["fiasco_amd_seq_encode", "fiasco_amd_seq_keep_reconstructed", "fiasco_amd_seq_reconstructed_planes"]
DEVICE = ["fiasco_amd_seq_open_device", "fiasco_amd_seq_set_outputs_device"]
MANIFEST = json.load(open(os.path.join(GOLDEN, "MANIFEST.json")))
PINNED = rc.pinned_names(MANIFEST)
_runs = {}


def _decls(path):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", path)).read(), flags=re.S)


def test_headers_symbol_list_and_export_map_hold_the_new_names(product):
    """the five entries live in a header of their own, include/libfiasco_amd_video.h, and in a symbol list of their own,
    fiasco_amd.VIDEO_SYMBOLS: the two older headers and EXPORTED_SYMBOLS are pinned as they are by tests/test_host_api.py"""
    host, hip = _decls("libfiasco_amd.h"), _decls("libfiasco_amd_video.h")
    declared = set(re.findall(r"\b(fiasco_\w*)\s*\(", hip))
    assert declared == set(HOST + DEVICE) and fiasco_amd.VIDEO_SYMBOLS == HOST + DEVICE
    for name, (restype, argtypes) in fiasco_amd._VIDEO_SIGNATURES.items():
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, hip).group(1)
        assert params.count(",") + 1 == len(argtypes), name
        assert not re.search(r"\b%s\b" % name, host) and name not in fiasco_amd.EXPORTED_SYMBOLS, name
        assert hasattr(product.L, name), name
    assert fiasco_amd._VIDEO_SIGNATURES["fiasco_amd_seq_open_device"][0] is ctypes.c_void_p
    # exported through the version script: the dynamic symbol table of the product holds every name
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    for name in HOST + DEVICE:
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
    pat = open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read()
    assert "fiasco_*;" in pat
    m = re.search(r"typedef struct fiasco_amd_seq_outputs \{(.*?)\} fiasco_amd_seq_outputs;", hip, flags=re.S)
    assert m, "struct fiasco_amd_seq_outputs"
    fields = re.findall(r"(\w+)\s*;", m.group(1))
    assert fields == ["targets", "sse", "maxdiff", "written", "stream"]
    assert fields == [f[0] for f in fiasco_amd.SeqOutputs._fields_]
    assert ctypes.sizeof(fiasco_amd.SeqOutputs) == 5 * ctypes.sizeof(ctypes.c_void_p)
    assert "device_frame" not in open(os.path.join(ROOT, "include", "libfiasco_amd.h")).read()


def test_the_oracle_library_has_the_host_outlets_and_none_of_the_device_entries(oracle):
    assert oracle.core_name() == "oracle-cpu"
    for name in HOST:
        assert hasattr(oracle.L, name), name
    for name in DEVICE:
        assert not hasattr(oracle.L, name), name


def test_import_does_not_import_torch():
    code = ("import sys; sys.path.insert(0, %r); import fiasco_amd; fiasco_amd.Sequence.from_device; "
            "fiasco_amd.Sequence.set_outputs; assert 'torch' not in sys.modules" % ROOT)
    subprocess.check_call([sys.executable, "-c", code])


@pytest.mark.parametrize("name", ["seq4_gray_ibbp", "seq3_color_ibp", "gops_ibpi", "seq3_color_carry48"])
def test_encode_gives_the_bytes_fiasco_coder_writes(oracle, manifest, inputs, tmp_path, name):
    frames, args, md5 = sd.case_of(manifest, inputs, name)
    names = rc.write_inputs(frames, tmp_path)
    q, o = sd.open_options(oracle, args)
    out = os.path.join(str(tmp_path), "coder.fco")
    assert oracle.fiasco_coder(names, out, q, o) == 1, oracle.error_message()
    seq = fiasco_amd.Sequence(oracle, frames, q, o)
    got = seq.encode()
    again = seq.encode()
    seq.free(); o.delete()
    assert got == open(out, "rb").read() and again == got
    assert hashlib.md5(got).hexdigest() == md5


def test_encode_needs_the_whole_stream_in_one_process(oracle, manifest, inputs):
    frames, args, _ = sd.case_of(manifest, inputs, "gops_ibpi")
    q, o = sd.open_options(oracle, args)
    seq = fiasco_amd.Sequence(oracle, frames, q, o, rank=1, world=2)
    with pytest.raises(fiasco_amd.FiascoError, match="world == 1"):
        seq.encode()
    seq.free(); o.delete()


def kept_run(oracle, manifest, inputs, name):
    """one oracle run per case and session with keep_reconstructed -> (stream, {display: (type, planes)})"""
    if name not in _runs:
        frames, args, _ = sd.case_of(manifest, inputs, name)
        q, o = sd.open_options(oracle, args)
        seq = fiasco_amd.Sequence(oracle, frames, q, o)
        seq.keep_reconstructed()
        stream = seq.encode()
        planes = {}
        for d in range(len(frames)):
            p, t = seq.reconstructed_planes(d)
            planes[d] = (t, p)
        seq.free(); o.delete()
        _runs[name] = (stream, planes)
    return _runs[name]


@pytest.mark.parametrize("name", PINNED)
def test_kept_planes_of_the_oracle_are_the_reference_coders(oracle, manifest, inputs, name):
    """every frame of every pinned case, B frames and the last frame of every group included, no directory knob"""
    assert "FIASCO_AMD_SEQ_RECONST_DIR" not in os.environ
    rec = rc.fixture()[name]
    stream, planes = kept_run(oracle, manifest, inputs, name)
    assert hashlib.md5(stream).hexdigest() == rec["stream_md5"]
    assert sorted(planes) == [f["display"] for f in rec["frames"]]
    for f in rec["frames"]:
        t, p = planes[f["display"]]
        assert t == f["type"] and rc.planes_md5(p) == f["planes_md5"], (name, f["display"])


@pytest.mark.parametrize("name", sd.names(MANIFEST))
def test_the_pixel_fixture_is_what_the_oracles_planes_give(oracle, manifest, inputs, name):
    """pixels_of_planes and distortion_of_planes of the oracle's kept planes: the fixture of the device outputs is pinned
    to the oracle as well as to the reference coder that made it (all-intra sequences included: keep decodes them too)"""
    frames, _, md5 = sd.case_of(manifest, inputs, name)
    rec = sd.fixture()[name]
    stream, planes = kept_run(oracle, manifest, inputs, name)
    assert hashlib.md5(stream).hexdigest() == md5 == rec["stream_md5"]
    assert [f["display"] for f in rec["frames"]] == list(range(len(frames)))
    for f in rec["frames"]:
        t, p = planes[f["display"]]
        got = sd.record_of_planes(frames[f["display"]], p)
        assert t == f["type"] and got == {k: f[k] for k in ("pixels_md5", "sse", "maxdiff")}, (name, f["display"], got)


def test_the_fixture_holds_results_only_and_is_small():
    assert os.path.getsize(sd.FIXTURE) < 100 * 1024
    fx = sd.fixture()
    assert sorted(fx) == sorted(sd.names(MANIFEST))
    assert sum(1 for c in fx.values() for f in c["frames"] if f["type"] == 2) >= 10       # B frames
    assert all(max(f["maxdiff"]) <= 255 and len(f["sse"]) == 3 for c in fx.values() for f in c["frames"])


def test_reconstructed_planes_without_keep_fail_with_a_message(oracle, manifest, inputs):
    frames, args, _ = sd.case_of(manifest, inputs, "seq2_gray_ip")
    q, o = sd.open_options(oracle, args)
    seq = fiasco_amd.Sequence(oracle, frames, q, o)
    seq.encode()
    with pytest.raises(fiasco_amd.FiascoError, match="not kept"):
        seq.reconstructed_planes(0)
    seq.keep_reconstructed()
    with pytest.raises(fiasco_amd.FiascoError, match="has not been reconstructed"):
        seq.reconstructed_planes(1)                 # kept from now on: the search before did not keep it
    with pytest.raises(fiasco_amd.FiascoError, match="no frame 2"):
        seq.reconstructed_planes(2)
    seq.encode()
    assert seq.reconstructed_planes(1)[1] == 1
    seq.keep_reconstructed(False)
    with pytest.raises(fiasco_amd.FiascoError, match="not kept"):
        seq.reconstructed_planes(1)
    seq.free(); o.delete()


class FakeArray:
    def __init__(self, shape, strides=None, ptr=0x1000):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "|u1", "data": (ptr, False), "version": 3, "strides": strides}


class Recorder:
    """stands in for a library: records what Sequence.from_device hands to fiasco_amd_seq_open_device and refuses"""
    path = "<recorder>"

    def __init__(self):
        self.L = self
        self.seen = None

    def fiasco_amd_seq_open_device(self, n, arr, stream, quality, options, rank, world):
        self.seen = (n, [(d.layout, d.width, d.height, d.pitch, d.plane_stride, d.data) for d in arr[:n]], rank, world)
        return None

    def error_message(self):
        return "refused by the recorder"


def test_strides_become_pitch_and_plane_stride_for_sequence_frames():
    r = Recorder()
    frames = [FakeArray((70, 100), (160, 1), 0x1000 + 20 + 3 * i) for i in range(3)]
    with pytest.raises(fiasco_amd.FiascoError, match="recorder"):
        fiasco_amd.Sequence.from_device(r, frames, 20.0, None, 1, 2)
    assert r.seen == (3, [(0, 100, 70, 160, 0, 0x1000 + 20 + 3 * i) for i in range(3)], 1, 2)
    with pytest.raises(fiasco_amd.FiascoError):
        fiasco_amd.Sequence.from_device(r, [FakeArray((3, 70, 100), (20000, 160, 1)), FakeArray((70, 100), (1, 70))])
    with pytest.raises(fiasco_amd.FiascoError, match="HIP library"):
        fiasco_amd.Sequence.from_device(fiasco_amd.Library(os.path.join(ROOT, "oracle", "liboracle_fiasco.so")), frames)


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_device_entries_fail_loudly_without_gpu(product, manifest, inputs):
    """No HIP device: a message, no crash (no pointer is looked at); the sequence stays usable"""
    o = product.cli_options()
    with pytest.raises(fiasco_amd.FiascoError, match="no HIP device available"):
        fiasco_amd.Sequence.from_device(product, [FakeArray((64, 96))] * 2, 20.0, o)
    with pytest.raises(fiasco_amd.FiascoError, match="No frames"):
        fiasco_amd.Sequence.from_device(product, [], 20.0, o)
    frames, _, _ = sd.case_of(manifest, inputs, "seq2_gray_ip")
    seq = fiasco_amd.Sequence(product, frames, 20.0, o)
    with pytest.raises(fiasco_amd.FiascoError, match="no HIP device available"):
        seq.set_outputs(distortion=True)
    with pytest.raises(fiasco_amd.FiascoError, match="no outputs are set"):
        seq.distortion()
    seq.set_outputs()                                # none again: nothing to refuse
    assert seq.gops == 1 and seq.frames == 2
    seq.free(); o.delete()
