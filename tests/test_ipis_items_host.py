"""The work items of the level recursion (csrc/hip/ipt_layout.h: lanes per state, item -> (state, slot group), which
lane's pair goes into which stored 16 bytes; op_ipis_t in csrc/hip/fc_tables.inc, FC_IPT builds of the frame kernel).
Host only: tests/ipis_items_check.cpp includes the kernel's own mapping and walks it lane by lane."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fiasco_amd", "csrc")


def test_items_cover_the_call_and_whole_rows_land_where_the_layout_says(tmp_path):
    """lc_max - images_level 1 .. 5, every subtree, first state 0 and 37, 1 .. 70 states and one count above the
    workgroup, 256 and 1024 lanes: every (state, slot) once, a state's lanes one aligned group of a wave, every access
    aligned and inside its table, a group's loads contiguous, and the simulated exchange and stores leave exactly the
    entries ipt_row + ipt_col define."""
    exe = str(tmp_path / "ipis_items_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Wno-unused-function", "-Wno-unused-parameter",
                        "-I" + os.path.join(CSRC, "hip"), "-o", exe, os.path.join(ROOT, "tests", "ipis_items_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "ipis_items_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
