#!/usr/bin/env python3
"""Developer probe (not part of the suite): what feeding a staged batch from device memory buys.

For a batch of 1080p frames, gray and colour, two things are timed, PNM path against device path, in ONE process
and one run (the yardstick is the PNM path of the same build):
  upload  Batch.upload() of host PNM bytes (host parse + convert, pinned memory, H2D copy) against
          Batch.upload_device() of resident uint8 tensors (one conversion kernel per share), each from the call
          until the device has the planes: wall clock around call + torch.cuda.synchronize(), and for the device
          path also HIP events on the caller's stream, which the library makes wait for the conversion
  loop    submit / upload / collect(resubmit) over `--passes` passes, frames per second

Method: one warm-up round of everything first (allocations, the slab pool, clocks), then `--reps` repetitions; the
median is the figure, min and max are kept.  Writes profiles/device_input_upload.json.  Under
`rocprofv3 --kernel-trace --stats -- python tests/gpu_device_input_probe.py --frames 64 --reps 2` the trace must
show one ic_convert_kernel call per upload_device / from_device and share: the sum of "device_conversions" over the
cases of the JSON it writes."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fiasco_amd  # noqa: E402
import synth  # noqa: E402

W, H = 1920, 1080


def frames_of(n, color, seed):
    """n frames cut from one larger synthetic picture at different offsets: [n, H, W] or [n, H, W, 3] uint8"""
    base = synth.synth_color_k(W + 64, H + 64, seed) if color else synth.synth(W + 64, H + 64, seed)
    out = np.empty((n, H, W, 3) if color else (n, H, W), dtype=np.uint8)
    for i in range(n):
        out[i] = base[i % 64:i % 64 + H, (i // 64) * 4 % 64:(i // 64) * 4 % 64 + W]
    return out


def pnm_of(frames, color):
    hdr = b"P%d\n%d %d\n255\n" % (6 if color else 5, W, H)
    return [hdr + f.tobytes() for f in frames]


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def probe(lib, n, color, reps, passes):
    o = lib.cli_options()
    host = [frames_of(n, color, 21 + k) for k in range(2)]
    pnm = [pnm_of(h, color) for h in host]
    dev = [torch.from_numpy(h).cuda() for h in host]
    torch.cuda.synchronize()
    if color:                                       # 1080p colour at the CLI defaults needs > 6000 states per frame:
        lib.L.fiasco_amd_release_memory()           # the declared limits extension, as bench.py config3_pass
        lib.set_limits(30000, 26)
    b = fiasco_amd.Batch.from_device(lib, dev[0], 20.0, o)
    conversions = [1]                               # from_device and every upload_device: one kernel call per share
    upload_device = b.upload_device

    def counted(frames, stream=None):
        conversions[0] += 1
        return upload_device(frames, stream)
    b.upload_device = counted
    first = b.encode()
    assert None not in first, lib.error_message()
    res = {"frames": n, "color": bool(color), "width": W, "height": H}
    up_pnm, up_dev, up_dev_ev = [], [], []
    for r in range(reps + 1):                       # round 0 warms up
        k = r & 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b.upload(pnm[k])
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t2 = time.perf_counter()
        e0.record()
        b.upload_device(dev[k])
        e1.record()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if r:
            up_pnm.append((t1 - t0) * 1e3); up_dev.append((t3 - t2) * 1e3); up_dev_ev.append(e0.elapsed_time(e1))
    res["upload_ms_pnm"] = stat(up_pnm)
    res["upload_ms_device"] = stat(up_dev)
    res["upload_ms_device_hip_events"] = stat(up_dev_ev)
    res["upload_ratio_pnm_over_device"] = res["upload_ms_pnm"]["median"] / res["upload_ms_device"]["median"]
    for name, feed in (("pnm", lambda k: b.upload(pnm[k])), ("device", lambda k: b.upload_device(dev[k]))):
        fps = []
        for r in range(reps + 1):
            feed(0)
            b.submit()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for p in range(passes):
                feed((p + 1) & 1)
                out = b.collect(resubmit=True)
                assert None not in out, lib.error_message()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            b.collect()
            if r:
                fps.append(n * passes / (t1 - t0))
        res["loop_fps_" + name] = stat(fps)
    res["device_conversions"] = conversions[0]
    res["loop_ratio_device_over_pnm"] = res["loop_fps_device"]["median"] / res["loop_fps_pnm"]["median"]
    b.free(); o.delete()
    if color:
        lib.set_limits(6000, 22)
        lib.L.fiasco_amd_release_memory()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--color-frames", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_input_upload.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "passes": a.passes, "cases": []}
    for color, n in ((0, a.frames), (1, a.color_frames if a.color_frames is not None else a.frames)):
        if n:
            res["cases"].append(probe(lib, n, color, a.reps, a.passes))
            print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
