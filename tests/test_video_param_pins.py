"""fiasco_c_options_set_video_param and the coding orders of B frames: the CPU oracle against the REFERENCE LIBRARY.

tests/golden/VIDEO_PARAM.json holds, per case, the md5 of the stream libfiasco_ref_recon.so wrote with the case's
(fps, cross_B_search, B_as_past_ref) and per frame the md5 of the planes it reconstructed
(tests/golden/make_video_param.py; the reference's command-line tool cannot set these parameters, so the library is
driven through ctypes).  tests/video_param_cases.py has the cases and says which coding orders they reach: B_as_past_ref = 0
(a B frame behind a B frame keeps the old past reference), a P frame coded right after a B frame, runs of three and four
B frames, two B runs in one group of pictures, trailing B runs, uppercase patterns.  tests/test_gpu_video_param.py runs the
same pins on the device.
"""
import os

import pytest

import reconst_cases as rc
import video_param_cases as vc

_runs = {}


def oracle_run(oracle, tmp_path_factory, name):
    """one oracle run per pinned case and session -> (fixture record, stream, planes, counts)"""
    if name not in _runs:
        frames, args, vp = vc.case_of(name)
        rec = vc.fixture()["cases"][name]
        assert rc.inputs_md5(frames) == rec["inputs_md5"] and args == rec["args"] and list(vp) == rec["video_param"], "the inputs of %s changed" % name
        stream, planes, counts, msg = vc.run_library(oracle, frames, args, vp, tmp_path_factory.mktemp("vp_" + name))
        assert stream is not None, "%s: %s" % (name, msg)
        _runs[name] = (rec, stream, planes, counts)
    return _runs[name]


@pytest.mark.parametrize("name", vc.NAMES)
def test_oracle_meets_the_reference_librarys_stream_and_frames(oracle, tmp_path_factory, name):
    vc.check_case(name, *oracle_run(oracle, tmp_path_factory, name))


def test_the_fixture_holds_the_pinned_set():
    fx = vc.fixture()
    assert sorted(fx["cases"]) == sorted(vc.NAMES) and sorted(fx["refusals"]) == sorted(vc.REFUSED)
    types = {n: "".join("IPB"[f["type"]] for f in rec["frames"]) for n, rec in fx["cases"].items()}
    # display order; a trailing B frame is coded as a P frame (codec/coder.c:553-557)
    assert types["ibpbp_x5_fps25_cross1_b0"] == "IBPBP" and types["ibbbbp_x6_fps25_cross1_b0"] == "IBBBBP"
    assert types["ibbpbbp_x7_pred_fps25_cross1_b0"] == "IBBPBBP" and types["ipbbpbbp_x8_fps25_cross1_b0"] == "IPBBPBBP"
    assert types["ipbpb_x5_fps25_cross1_b0"] == "IPBPP" and types["ibb_x3_fps25_cross1_b0"] == "IBP" and types["ib_x2_fps25_cross1_b0"] == "IP"
    assert types["ibbp_x9_fps25_cross1_b0"] == "IBBPIBBPI"
    assert sum(1 for rec in fx["cases"].values() if rec["geometry"][2] == 3) == 2
    # the default parameters are what the command-line tool's streams carry
    assert all((rec["stream_md5"] == rec["cli_stream_md5"]) == (rec["video_param"][0] == 25 and rec["video_param"][2] == 1)
               for rec in fx["cases"].values())


def test_cross_b_search_changes_nothing_and_case_of_the_pattern_neither(oracle, tmp_path_factory):
    """codec/coder.c:359 overwrites cross_B_search with half_pixel; pattern2type lowers the letter"""
    a, b = (oracle_run(oracle, tmp_path_factory, n) for n in vc.CROSS_TWIN)
    assert a[1] == b[1] and a[0]["stream_md5"] == b[0]["stream_md5"]
    for upper, lower in vc.LOWERCASE_TWIN.items():
        a, b = oracle_run(oracle, tmp_path_factory, upper), oracle_run(oracle, tmp_path_factory, lower)
        assert a[1] == b[1] and a[0]["stream_md5"] == b[0]["stream_md5"]


class Bits:
    """the reference's bit reader on a stream: most significant bit first; Rice code with parameter 8 (unary quotient
    of ones, a zero, 8 bits)"""

    def __init__(self, data):
        self.data, self.at = data, 0

    def bit(self):
        v = (self.data[self.at >> 3] >> (7 - (self.at & 7))) & 1
        self.at += 1
        return v

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = 2 * v + self.bit()
        return v

    def rice(self):
        q = 0
        while self.bit():
            q += 1
        return (q << 8) + self.bits(8)

    def string(self):
        s = b""
        while True:
            c = self.bits(8)
            if not c:
                return s
            s += bytes([c])


def video_header(stream):
    """the header as read_basic_file_header reads it (reference input/read.c:95-214) -> dict"""
    assert stream[:7] == b"FIASCO\n"
    b = Bits(stream[7:])
    h = {"basis": b.string(), "release": b.rice()}
    while True:
        t = b.rice()
        if t == 0:
            break
        h[{1: "title", 2: "comment"}[t]] = b.string()
    h["max_states"], h["color"], h["width"], h["height"] = b.rice(), b.bit(), b.rice(), b.rice()
    if h["color"]:
        h["chroma_max_states"] = b.rice()
    h["p_min_level"], h["p_max_level"], h["frames"], h["smoothing"] = b.rice(), b.rice(), b.rice(), b.rice()
    b.bits(5)
    for _ in range(3):
        if b.bit():
            b.bits(5)
    assert h["frames"] > 1
    h["fps"], h["search_range"], h["half_pixel"], h["B_as_past_ref"] = b.rice(), b.rice(), b.bit(), b.bit()
    h["header_bytes"] = 7 + (b.at + 7) // 8
    return h


@pytest.mark.parametrize("name", vc.NAMES)
def test_fps_and_the_flag_decode_back_from_the_header(oracle, tmp_path_factory, name):
    rec, stream, _, _ = oracle_run(oracle, tmp_path_factory, name)
    frames, _, vp = vc.case_of(name)
    h = video_header(stream)
    w, hh, nb = rc.geometry(frames)
    assert (h["width"], h["height"], h["color"], h["frames"]) == (w, hh, int(nb == 3), len(frames)), h
    assert (h["fps"], h["half_pixel"], h["B_as_past_ref"], h["search_range"]) == (vp[0], 0, vp[2], 16), h


def test_the_fps_values_of_the_pinned_set(oracle, tmp_path_factory):
    """0, 25, 30 and 100000: the last one's quotient is 390 ones, 49 bytes more than the 507 of fps 25"""
    got = {vc.case_of(n)[2][0]: len(oracle_run(oracle, tmp_path_factory, n)[1]) for n in vc.FPS_CASES}
    assert sorted(got) == [0, 25, 30, 100000]
    assert got[100000] - got[25] == (100000 >> 8) // 8 + 1 == 49 and got[0] == got[25]


@pytest.mark.parametrize("name", list(vc.REFUSED))
def test_refused_patterns(oracle, tmp_path, name):
    """an I frame between a B frame and its future reference: the reference dies, the library returns 0 with the
    message and leaves an existing output file as it was"""
    assert vc.fixture()["refusals"][name]["reference"].startswith(("signal", "exit"))
    vc.refusal_leaves_the_output(oracle, name, tmp_path)


def test_the_pinned_set_is_not_hollow(oracle, tmp_path_factory):
    """the flag changes the stream and a B frame wherever two B frames follow each other; the P frame coded right after
    a B frame is predicted: it has forward blocks, on the moving windows of reconst_cases._shift as they are"""
    vc.check_not_hollow({n: oracle_run(oracle, tmp_path_factory, n)[1:] for n in vc.NAMES})


def test_the_reference_library_alive_gives_the_fixture(tmp_path):
    """where oracle/_ref is built: the driver of the generator, run again on two cases, one per flag value"""
    if not os.path.exists(vc.REF_LIB):
        pytest.skip("libfiasco_ref_recon.so is not built (oracle/ref_build.sh needs the reference's sources)")
    for name in ("ibbbp_x5_fps25_cross1_b0", "ibbpbp_x6_fps25_cross1_b1"):
        frames, args, vp = vc.case_of(name)
        err, stream, planes = vc.run_reference_library(frames, args, vp, tmp_path / name)
        assert err is None, err
        rec = vc.fixture()["cases"][name]
        assert [rc.planes_md5(planes[f["display"]][1]) for f in rec["frames"]] == [f["planes_md5"] for f in rec["frames"]]
        assert len(stream) == rec["bytes"]


def test_oracle_fuzz_against_the_live_reference_library(oracle, tmp_path):
    """Seeds 5200 .. 5223 of video_param_cases.random_case through the oracle and the reference library: streams and
    planes equal wherever the reference writes a stream.  The reference codes 20 of the 24: 5200, 5204, 5222 and 5223
    are colour frames on which it, and the oracle alike, ends with "Can't write more than n weights"."""
    if not os.path.exists(vc.REF_LIB):
        pytest.skip("libfiasco_ref_recon.so is not built (oracle/ref_build.sh needs the reference's sources)")
    res = [(s,) + vc.fuzz_seed(oracle, s, tmp_path) for s in vc.FUZZ_SEEDS]
    for s, verdict, text, coded in res:
        print("video param fuzz oracle seed %d: %s %s%s" % (s, verdict, text, "" if coded else " [no reference stream]"))
    assert not [t for _, v, t, _ in res if v == "MISMATCH"], "\n".join(t for _, v, t, _ in res if v == "MISMATCH")
    n = sum(1 for _, v, _, coded in res if v == "compared" and coded)
    print("video param fuzz oracle: %d of %d seeds compared with the reference" % (n, len(res)))
    assert n >= 20, n
