"""bin/dfiasco beside the reference's dfiasco -- run on a real MI355X: -m gpu.  Both front ends run on the same stream with
the same arguments into two temporary directories; the names of the files they write and their bytes are compared with ==.
The reference binary is oracle/_ref/dfiasco_ref (oracle/ref_build.sh); where it did not travel the tests skip.  Children run
one after another, each in a fresh process with a time limit; the test stops at the first one that ends abnormally."""
import os
import shutil
import subprocess

import pytest

import fiasco_amd
import stream_cases as sc
from conftest import GOLDEN, REF_SHARE, ROOT

pytestmark = pytest.mark.gpu

OURS = os.path.join(os.path.dirname(fiasco_amd.LIB_PATH), "bin", "dfiasco")
THEIRS = os.path.join(ROOT, "oracle", "_ref", "dfiasco_ref")
ENV = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
ENV.pop("FIASCO_IMAGES", None)
ARGS = [["-o", "out"], ["-m", "-1"], ["-m", "1", "-s", "35"], ["-s", "0"]]


def run(exe, args, stream, cwd):
    """(exit status, stderr, {file name: bytes}) of one front end in its own directory; the stream is copied there, so a
    name made from the input's is the same for both"""
    os.makedirs(cwd)
    shutil.copy(sc.stream_path(stream), os.path.join(cwd, "in.fco"))
    r = subprocess.run([exe] + args + ["in.fco"], cwd=cwd, env=ENV, capture_output=True, timeout=60)
    assert r.returncode >= 0 and r.returncode not in (124, 134, 137, 139), (exe, args, stream, r.returncode, r.stderr.decode("latin-1")[-400:])
    files = {n: open(os.path.join(cwd, n), "rb").read() for n in sorted(os.listdir(cwd)) if n != "in.fco"}
    if r.stdout:
        files["<stdout>"] = r.stdout
    return r.returncode, r.stderr.decode("latin-1"), files


@pytest.mark.parametrize("stream", ["g100x70_q20", "seq4_gray_ibbp", sc.IPBBP])
def test_same_files_and_bytes_as_the_references_dfiasco(stream, tmp_path):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    if not os.path.exists(THEIRS):
        pytest.skip("oracle/_ref/dfiasco_ref is not here (oracle/ref_build.sh builds it from the reference tree)")
    for k, args in enumerate(ARGS):
        want = run(THEIRS, args, stream, str(tmp_path / ("ref%d" % k)))
        got = run(OURS, args, stream, str(tmp_path / ("amd%d" % k)))
        assert want[0] == 0 and got[0] == 0, (stream, args, want[1][-300:], got[1][-300:])
        assert sorted(got[2]) == sorted(want[2]) and got[2], (stream, args, sorted(got[2]), sorted(want[2]))
        assert got[2] == want[2], (stream, args)
        decoding = lambda text: [ln for ln in text.split("\n") if ln.startswith("Decoding frame")]
        assert decoding(got[1]) == decoding(want[1]), (stream, args)


def test_a_refused_magnification_ends_both_with_the_same_sentence(tmp_path):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    if not os.path.exists(THEIRS):
        pytest.skip("oracle/_ref/dfiasco_ref is not here (oracle/ref_build.sh builds it from the reference tree)")
    want = run(THEIRS, ["-m", "-3"], "g100x70_q20", str(tmp_path / "ref"))
    got = run(OURS, ["-m", "-3"], "g100x70_q20", str(tmp_path / "amd"))
    sentence = "Magnifaction factor `-3' is too small. Minimum value is -1."
    assert want[0] != 0 and got[0] != 0 and sentence in want[1] and sentence in got[1] and not want[2] and not got[2]
