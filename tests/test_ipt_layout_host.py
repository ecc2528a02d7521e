"""The state-major copy of the level recursion's sources (DevFrame.ipt, csrc/hip/ipt_layout.h; FC_IPT builds of the frame
kernel): where an entry lies, what op_ipis_t loads and stores there, and the room the slab layout gives it.  Host only:
tests/ipt_layout_check.cpp includes the kernel's own offset arithmetic and the launcher's make_layout()."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fiasco_amd", "csrc")


def test_ipt_layout_and_the_kernels_accesses(tmp_path):
    """lc_max - images_level 1 .. 5: distinct entries inside the buffer, sources one level down, every vector access of
    every subtree aligned to its width; the slab grows by NA * P * 4 bytes rounded to 256, and 256 slabs of a 4K frame still fit."""
    exe = str(tmp_path / "ipt_layout_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-parameter",
                        "-I" + os.path.join(CSRC, "hip"), "-I" + os.path.join(CSRC, "host"), "-I" + os.path.join(ROOT, "include"),
                        "-o", exe, os.path.join(ROOT, "tests", "ipt_layout_check.cpp")], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ipt_layout_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
