"""The conversion kernel of YCbCr frames in device memory (csrc/hip/input_convert_ycbcr.inc, icy_convert_kernel) replayed on
the CPU: tests/ycbcr_in_step_check.cpp holds the kernel's per-item function and its load and store helpers as plain C++ and is
built here with AddressSanitizer and UBSan -- widths 32, 34, 38 and 50, heights 32 and 34, 4:2:0 and 4:4:4, c_step 1 and 2 in
both orders, pitches larger than the row, source bases one byte off alignment, planes at 4-, 8- and 16-byte alignment, guard
bytes around the planes, source blocks that end with their last sample, the result against a per-sample loop.  A program of
its own, linked with the sanitizers itself: nothing is loaded into this process.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
INC = ["-I" + os.path.join(ROOT, "fiasco_amd", "csrc", "hip"), "-I" + os.path.join(ROOT, "include")]


def test_ycbcr_kernel_items_replayed_under_sanitizers(tmp_path):
    exe = str(tmp_path / "ycbcr_in_step_check")
    r = subprocess.run(["g++", "-std=c++17", "-Wno-unknown-pragmas"] + SAN + INC + ["-o", exe, os.path.join(ROOT, "tests", "ycbcr_in_step_check.cpp")],
                       capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("no address,undefined sanitizer runtime on this machine")
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    if "unexpected memory mapping" in out.stderr:          # the runtime cannot place its shadow memory in this address space
        pytest.skip("the address,undefined sanitizer runtime does not start on this machine")
    assert out.returncode == 0 and "ycbcr_in_step_check: ok" in out.stdout and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
