#!/usr/bin/env python3
"""Developer probe (not part of the suite): what decoding in 4:2:0 costs on the device beside the 4:4:4 path.  Its JSON lines
belong in profiles/yuv420_device.json; no run of it is recorded yet.

Flights -- `--case colour720` or `--case colour320`, one case per process: ONE flight of 32 device-fed colour frames
(replicas of a frame, staged with Batch.from_device) is coded once; then the routes alternate call by call, 1 warm-up round
and `--reps` rounds, and the decoder's own device time of every call (fiasco_amd_stats.decoder_us: HIP events around the
uploads and the kernels of the flight) is kept: median, min, max in microseconds.  Routes, each at smoothing 0 and -1:
  rgb          fiasco_amd_batch_decode_device_shown() into planar RGB, the 4:4:4 path that existed before: the baseline
  nv12, i420   fiasco_amd_batch_decode_device_420() into packed NV12 and I420 buffers
The kernels alone -- `--kernels`, to be run under `rocprofv3 --kernel-trace --stats -d DIR -o kt --`: colour planes of
4096 x 4096 through fiasco_amd_planes_to_pixels_device() (oc_convert_kernel, planar RGB) and 4:2:0 planes of 8192 x 4096
through fiasco_amd_planes_to_420_device() (oc420_convert_kernel, NV12 and I420), 1 warm-up and 5 timed launches each, in an
order the probe writes to `--order FILE`; `--summarise DB --order FILE` then reads the dispatches of the two kernels from the
rocpd database in that order and prints per launch kind the median kernel time and the bytes moved per second (the bytes the
algorithm needs: 2 per value read, 1 per byte written).
Every step under a time limit of its own, stopping at the first that fails:
  timeout -k 10 400 python tests/gpu_420_probe.py --case colour720 && \\
  timeout -k 10 300 python tests/gpu_420_probe.py --case colour320 && \\
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tests/gpu_420_probe.py --kernels --order DIR/order.json && \\
  python tests/gpu_420_probe.py --summarise DIR/*/*_results.db --order DIR/order.json
Prints one JSON line per step."""
import argparse
import json
import os
import sqlite3
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"colour720": (1280, 720), "colour320": (320, 200)}
FRAMES = 32
WARM, TIMED = 1, 5


def flights(a):
    import torch
    import fiasco_amd
    import synth
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.Library()
    lib.set_verbosity(0)
    w, h = CASES[a.case]
    src = torch.from_numpy(synth.synth_color_k(w, h, 1234)).cuda()
    o = lib.cli_options()
    b = fiasco_amd.Batch.from_device(lib, [src] * FRAMES, 20.0, o)
    assert None not in b.encode(), lib.error_message()
    rgb = list(torch.zeros((FRAMES, 3, h, w), dtype=torch.uint8, device="cuda"))
    ys = list(torch.zeros((FRAMES, h, w), dtype=torch.uint8, device="cuda"))
    pairs = list(torch.zeros((FRAMES, h // 2, w // 2, 2), dtype=torch.uint8, device="cuda"))
    cbs = list(torch.zeros((FRAMES, h // 2, w // 2), dtype=torch.uint8, device="cuda"))
    crs = list(torch.zeros((FRAMES, h // 2, w // 2), dtype=torch.uint8, device="cuda"))
    calls = {}
    for s in (0, -1):
        calls["rgb_s%d" % s] = (lambda s=s: b.decode_shown(rgb, smoothing=s))
        calls["nv12_s%d" % s] = (lambda s=s: b.decode_420(list(zip(ys, pairs)), smoothing=s))
        calls["i420_s%d" % s] = (lambda s=s: b.decode_420(list(zip(ys, cbs, crs)), smoothing=s))
    us = {n: [] for n in calls}
    for rep in range(a.reps + 1):
        for route, call in calls.items():
            lib.reset_stats()
            good = call()
            torch.cuda.synchronize()                                # a failure surfaces here, under its route's name
            st = lib.get_stats()
            assert good == FRAMES and st.decoder_frames == FRAMES, (route, good, lib.error_message())
            if rep:
                us[route].append(int(st.decoder_us))
    res = {"case": a.case, "frames": FRAMES, "width": w, "height": h, "reps": a.reps, "device": torch.cuda.get_device_name(0), "decoder_us": {},
           "bytes_written_per_flight": {"rgb": FRAMES * w * h * 3, "nv12": FRAMES * w * h * 3 // 2, "i420": FRAMES * w * h * 3 // 2}}
    for n, v in us.items():
        res["decoder_us"][n] = {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
    print(json.dumps(res), flush=True)
    b.free(); o.delete()


def kernels(a):
    import numpy as np
    import torch
    import fiasco_amd
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.Library()
    lib.set_verbosity(0)
    order = []
    rng = np.random.RandomState(3)
    w, h = 4096, 4096
    planes = torch.from_numpy(rng.randint(-2200, 2200, size=(3, h, w)).astype(np.int16)).cuda()
    target = torch.zeros((3, h, w), dtype=torch.uint8, device="cuda")
    for rep in range(WARM + TIMED):
        fiasco_amd.planes_to_pixels_device(lib, planes, target)
        order.append({"kernel": "oc_convert_kernel", "route": "rgb_planar", "timed": rep >= WARM, "bytes": 3 * w * h * 3})
    del planes, target
    w, h = 8192, 4096
    y = torch.from_numpy(rng.randint(-2200, 2200, size=(h, w)).astype(np.int16)).cuda()
    cb = torch.from_numpy(rng.randint(-2200, 2200, size=(h // 2, w // 2)).astype(np.int16)).cuda()
    cr = torch.from_numpy(rng.randint(-2200, 2200, size=(h // 2, w // 2)).astype(np.int16)).cuda()
    ty = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    tp = torch.zeros((h // 2, w // 2, 2), dtype=torch.uint8, device="cuda")
    tb, tr = torch.zeros((h // 2, w // 2), dtype=torch.uint8, device="cuda"), torch.zeros((h // 2, w // 2), dtype=torch.uint8, device="cuda")
    for route, target in (("nv12", (ty, tp)), ("i420", (ty, tb, tr))):
        for rep in range(WARM + TIMED):
            fiasco_amd.planes_to_420_device(lib, y, cb, cr, target)
            order.append({"kernel": "oc420_convert_kernel", "route": route, "timed": rep >= WARM, "bytes": 3 * (w * h * 3 // 2)})
    torch.cuda.synchronize()
    json.dump(order, open(a.order, "w"))
    print(json.dumps({"kernels": "launched", "dispatches": len(order)}), flush=True)


def summarise(a):
    order = json.load(open(a.order))
    con = sqlite3.connect(a.summarise)
    rows = [(name, end - start) for name, start, end in con.execute("select name, start, end from kernels order by start")
            if "oc_convert_kernel" in name or "oc420_convert_kernel" in name]
    assert len(rows) == len(order), (len(rows), len(order))
    got = {}
    for (name, ns), want in zip(rows, order):
        assert want["kernel"] in name, (name, want)
        if want["timed"]:
            got.setdefault((want["kernel"], want["route"]), {"bytes": want["bytes"], "ns": []})["ns"].append(ns)
    res = {"kernels": {}}
    for (kernel, route), v in got.items():
        med = statistics.median(v["ns"])
        res["kernels"][route] = {"kernel": kernel, "bytes": v["bytes"], "median_us": med / 1e3, "min_us": min(v["ns"]) / 1e3, "max_us": max(v["ns"]) / 1e3,
                                 "n": len(v["ns"]), "GB_per_s": round(v["bytes"] / med, 1)}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--order", default="yuv420_order.json")
    ap.add_argument("--summarise")
    a = ap.parse_args()
    if a.summarise:
        summarise(a)
    elif a.kernels:
        kernels(a)
    else:
        assert a.case, "--case, --kernels or --summarise"
        flights(a)


if __name__ == "__main__":
    main()
