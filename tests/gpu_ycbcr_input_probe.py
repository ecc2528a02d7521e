#!/usr/bin/env python3
"""Developer probe (not part of the suite): what the conversion of YCbCr frames in device memory costs beside the conversion of
RGB frames, whose kernel (ic_convert_kernel on RGB8_INTERLEAVED) is the yardstick: it is timed in the same run.

For 32 colour frames of 1080p, resident in device memory as NV12, I420, planar 4:4:4 and interleaved RGB, the hand-over of
replacement frames is timed with HIP events on the caller's stream.  The host side of a hand-over (the binding, the checks of
every plane, two passes over the shares) takes longer than the kernel, so it must not fall between the events: before the
first event the caller's stream is given `--ahead` fills of a 1 GiB buffer, several milliseconds of work, and the host has
long returned from the call when the device reaches the first event.  That is checked, not assumed: a repetition counts only
if the first event had NOT happened yet when the call returned (`late` counts the others).  What lies between the events then
is what the device does for the hand-over: the upload stream's wait for the caller's, the copy of the descriptor table (a few
KiB), the ONE conversion launch of the share, and the caller's stream's wait for it.  Nothing is submitted or encoded.

Method: the kinds take turns inside every repetition, two warm-up rounds first (allocations, code objects, clocks), then
`--reps` repetitions; the median is the figure, min and max are kept.  Achieved bytes per second: the bytes the conversion has
to move -- 1.5 + 6 per pixel for 4:2:0, 3 + 6 for 4:4:4 and RGB -- over the median time; it understates the kernel's own rate by
the two stream waits and the table copy.  `--kinds a,b` restricts the run (under `rocprofv3 --kernel-trace`, in a run of its
own, the trace then holds the durations of the launches of those kinds alone).  Writes profiles/ycbcr_input.json."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fiasco_amd  # noqa: E402
import synth  # noqa: E402
import ycbcr_ref as yr  # noqa: E402

W, H = 1920, 1080
BYTES_PER_PIXEL = {"rgb8_interleaved": 3 + 6, "nv12": 1.5 + 6, "i420": 1.5 + 6, "444": 3 + 6}


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def sources(n):
    """n frames of one synthetic picture at different offsets, in the four kinds, on the device"""
    base = synth.synth_color_k(W + 64, H + 64, 21)
    cut = lambda a, i: a[i % 64:i % 64 + H, i % 32:i % 32 + W]            # H x W ( x 3) out of (H + 64) x (W + 64) ( x 3)
    rgb = np.stack([cut(base, i) for i in range(n)])
    planes = yr.bytes_of(yr.pnm_planes(base))                                                  # [3][H + 64][W + 64]
    p = [np.stack([cut(planes[k], i) for i in range(n)]) for k in range(3)]                    # [3][n][H][W]
    y, cb, cr = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in p)
    cb2, cr2 = cb[:, ::2, ::2].contiguous(), cr[:, ::2, ::2].contiguous()
    pairs = torch.stack([cb2, cr2], dim=-1).contiguous()
    return {
        "rgb8_interleaved": list(torch.from_numpy(rgb).cuda()),
        "nv12": [(y[i], pairs[i]) for i in range(n)],
        "i420": [(y[i], cb2[i], cr2[i]) for i in range(n)],
        "444": [(y[i], cb[i], cr[i]) for i in range(n)],
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ahead", type=int, default=24, help="fills of 1 GiB in front of every timed hand-over")
    ap.add_argument("--kinds", default="", help="comma separated; default all four")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ycbcr_input.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    lib.set_limits(30000, 26)                       # 1080p colour at the CLI defaults: the declared limits extension
    o = lib.cli_options()
    src = sources(a.frames)
    torch.cuda.synchronize()
    b = fiasco_amd.Batch.from_device(lib, src["rgb8_interleaved"], 20.0, o)
    feed = {k: (b.upload_device if k == "rgb8_interleaved" else b.upload_device_ycbcr) for k in src}
    kinds = [k for k in src if k in a.kinds.split(",")] if a.kinds else list(src)
    ms, late = {k: [] for k in kinds}, {k: 0 for k in kinds}
    ahead = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    for r in range(a.reps + 2):                     # rounds 0 and 1 warm up
        for k in kinds:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            for _ in range(a.ahead):
                ahead.fill_(r & 255)                # work in front of the first event: the host gets ahead of the device
            e0.record()
            feed[k](src[k])
            in_time = not e0.query()                # the call is back and the device has not reached the first event
            e1.record()
            torch.cuda.synchronize()
            if r >= 2 and in_time:
                ms[k].append(e0.elapsed_time(e1))
            elif r >= 2:
                late[k] += 1
    res = {"device": torch.cuda.get_device_name(0), "frames": a.frames, "width": W, "height": H, "reps": a.reps,
           "ahead_fills_of_1GiB": a.ahead,
           "timed": "HIP events on the caller's stream around upload_device / upload_device_ycbcr, the host's part of the call over "
                    "before the device reaches the first event: two stream waits + table copy + one launch", "kinds": {}}
    for k in kinds:
        assert ms[k], "%s: the host never got ahead of the device (raise --ahead)" % k
        t = stat(ms[k])
        moved = BYTES_PER_PIXEL[k] * W * H * a.frames
        res["kinds"][k] = {"ms": t, "bytes_moved": moved, "bytes_per_pixel": BYTES_PER_PIXEL[k],
                           "gbytes_per_s": moved / (t["median"] * 1e-3) / 1e9, "late_repetitions_dropped": late[k]}
    if "rgb8_interleaved" in kinds:
        base = res["kinds"]["rgb8_interleaved"]["ms"]["median"]
        for k in kinds:
            res["kinds"][k]["time_over_rgb"] = res["kinds"][k]["ms"]["median"] / base
    b.free(); o.delete()
    lib.set_limits(6000, 22)
    lib.L.fiasco_amd_release_memory()
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
