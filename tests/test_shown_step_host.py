"""The fused smoothing kernel of the device decoder (csrc/hip/smooth.inc, sm_frame_kernel) replayed on the CPU:
tests/shown_step_check.cpp holds the kernel's body between two barriers, the per-item function, the checks and the packing
as plain C++ and is built here with AddressSanitizer and UBSan -- the border lists of magnified frames (the sizes of
tests/golden/DECODED_SHOWN.json at every magnification from -3 to 2, the clipped borders of 50 x 36 and 66 x 34 among them),
planes of exactly W x H values, tables in one heap block of exactly the carved size, passes in order and the threads of a
pass scrambled, fused and per-pass planes in one flight, the result against the sequential loop in state order.  A program
of its own, linked with the sanitizers itself: nothing is loaded into this process.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_smoothing_kernel_replayed_under_sanitizers(tmp_path):
    exe = str(tmp_path / "shown_step_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I" + os.path.join(ROOT, "fiasco_amd", "csrc", "hip"), "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "shown_step_check.cpp")], capture_output=True, text=True)
    if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
        pytest.skip("no address,undefined sanitizer runtime on this machine")
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    if "unexpected memory mapping" in out.stderr:          # the runtime cannot place its shadow memory in this address space
        pytest.skip("the address,undefined sanitizer runtime does not start on this machine")
    assert out.returncode == 0 and "shown_step_check: ok" in out.stdout and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
