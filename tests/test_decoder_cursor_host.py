"""The cursor under fa_stream_walk on the host under the sanitizers: tests/decoder_cursor_check.c, a program with its own
main, built here with -fsanitize=address,undefined (the leak check on) from the product's reader and stream object and a run
callback that decodes nothing.  It plays every golden video, the orphaned-B stream and `gops_ibpi' coded by the oracle
display frame by display frame at read-ahead 1, 2, 3 and 32 and checks what the header of the program lists: every coded
frame reaches the decoder once, its references are alive and unsmoothed, the flights are the walk's, a failed frame is
consumed and named by its dependants, and nothing is held behind the last frame or an early close.  No device."""
import os
import subprocess

import pytest

import reconst_cases as rc
import stream_cases as sc
from conftest import GOLDEN, ROOT

HOST = os.path.join(ROOT, "fiasco_amd", "csrc", "host")
SOURCES = [os.path.join(ROOT, "tests", "decoder_cursor_check.c")] + [os.path.join(HOST, f) for f in (
    "fa_reader.c", "fa_stream.c", "fa_bitio.c", "fa_wfa.c", "fa_writer.c", "fa_rpf.c", "fa_error.c")]
VIDEOS = sc.VIDEOS + sc.NEW


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("cursor_check")), "decoder_cursor_check")
    subprocess.check_call(["gcc", "-std=gnu99", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
                           "-Wno-unused-parameter", "-I" + os.path.join(ROOT, "include"), "-I" + HOST, "-o", out] + SOURCES + ["-lm"])
    return out


def run(exe, *paths):
    """{name: (frames, decoded, {display: cause})}; a report of the program or of the sanitizers ends it with a status that is not 0"""
    r = subprocess.run([exe] + [str(p) for p in paths], capture_output=True, env=dict(os.environ, FIASCO_DATA=GOLDEN, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-400:], r.stderr.decode()[-2000:])
    got = {}
    for line in r.stdout.decode().strip().split("\n"):
        name, n, ok, failed = line.split(" ", 3)
        causes = dict((int(e.split(":", 1)[0]), e.split(":", 1)[1]) for e in failed[len("failed="):].split(";") if e)
        got[name] = (int(n), int(ok[len("ok="):]), causes)
    return got


def test_every_golden_video_plays_frame_by_frame(exe):
    got = run(exe, *[sc.stream_path(n) for n in VIDEOS])
    fx = sc.fixture()["streams"]
    assert sorted(got) == sorted(VIDEOS)
    for name in VIDEOS:
        n = len(fx[name]["frame_types"])
        assert got[name] == (n, n, {}), name
    assert any(fx[n]["frame_types"].count(2) >= 2 for n in VIDEOS) and any(fx[n]["frame_types"][1:].count(0) for n in VIDEOS)


def test_a_failed_frame_is_consumed_and_named_by_its_dependants(exe):
    n, ok, causes = run(exe, sc.stream_path(sc.ORPHAN))[sc.ORPHAN]
    assert (n, ok) == (4, 2) and sorted(causes) == [1, 2]
    assert "motion vector without its reference frame" in causes[1]
    assert causes[2].startswith("display frame 2 is predicted from frame 1, which failed")


def test_two_groups_of_pictures_coded_by_the_oracle(exe, oracle, manifest, inputs, tmp_path):
    frames, args = rc.case_of(manifest, inputs, "gops_ibpi")
    stream, _, _, msg = rc.run_library(oracle, frames, args, tmp_path)
    assert stream is not None, msg
    path = tmp_path / "gops_ibpi.fco"
    path.write_bytes(stream)
    assert run(exe, path)["gops_ibpi"] == (len(frames), len(frames), {})
