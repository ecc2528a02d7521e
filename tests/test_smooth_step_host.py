"""The smoothing step of the device decoder (csrc/hip/smooth.inc) replayed on the CPU: tests/smooth_step_check.cpp holds
the step's checks, its packing and the kernel's per-item function as plain C++ and is built here with AddressSanitizer
and UBSan -- tables in heap blocks of exactly the size the flight carves, planes of exactly W x H values, flights of 1
to 32 frames of which some drop out, a 1280 x 720 list with 25 passes and more, items in a scattered order, the result
against the sequential loop; malformed lists refused.  A program of its own, linked with the sanitizers itself: nothing
is loaded into this process.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_smoothing_step_replayed_under_sanitizers(tmp_path):
    exe = str(tmp_path / "smooth_step_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "fiasco_amd", "csrc", "hip"), "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "smooth_step_check.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("no address,undefined sanitizer runtime on this machine")
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    if "unexpected memory mapping" in out.stderr:          # the runtime cannot place its shadow memory in this address space
        pytest.skip("the address,undefined sanitizer runtime does not start on this machine")
    assert out.returncode == 0 and "smooth_step_check: ok" in out.stdout and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
