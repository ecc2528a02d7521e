"""The 4:2:0 rendering kernel of the device decoder (csrc/hip/render_420.inc, rd420_render_kernel) replayed on the CPU:
tests/render_420_step_check.cpp holds the kernel's per-item functions, render.inc's pixel arithmetic, stores and the
exchange inside a wave (with 64, 63 and 1 live lanes) as plain C++ and is built here with AddressSanitizer and UBSan -- planes
of exactly W x H and (W / 2) x (H / 2) values, surfaces of exactly the bytes their rows span, widths 2, 4, 14, 16, 18, 30, 32, 34,
36 and 66 with heights 2, 4 and 6, surfaces that begin one pixel (at 24 bpp also one byte) into their block, pitches above the
row, all twelve renderers, the result against a per-pixel loop and against the plain host loop csrc/host/fa_render.c.  A
program of its own, linked with the sanitizers itself: nothing is loaded into this process.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-Wall", "-Wextra", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
INC = ["-I" + os.path.join(ROOT, "fiasco_amd", "csrc", "hip"), "-I" + os.path.join(ROOT, "fiasco_amd", "csrc", "host"), "-I" + os.path.join(ROOT, "include")]


def test_render_420_kernel_items_replayed_under_sanitizers(tmp_path):
    exe, host = str(tmp_path / "render_420_step_check"), str(tmp_path / "fa_render.o")
    steps = [["gcc", "-std=gnu99"] + SAN + INC + ["-c", os.path.join(ROOT, "fiasco_amd", "csrc", "host", "fa_render.c"), "-o", host],
             ["g++", "-std=c++17", "-Wno-unknown-pragmas"] + SAN + INC + ["-o", exe, os.path.join(ROOT, "tests", "render_420_step_check.cpp"), host]]
    for cmd in steps:
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0 and ("cannot find" in r.stderr or "unrecognized" in r.stderr):
            pytest.skip("no address,undefined sanitizer runtime on this machine")
        assert r.returncode == 0 and not r.stderr, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    if "unexpected memory mapping" in out.stderr:          # the runtime cannot place its shadow memory in this address space
        pytest.skip("the address,undefined sanitizer runtime does not start on this machine")
    assert out.returncode == 0 and "render_420_step_check: ok" in out.stdout and not out.stderr, out.stdout[-2000:] + out.stderr[-4000:]
