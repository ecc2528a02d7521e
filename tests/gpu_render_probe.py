#!/usr/bin/env python3
"""Developer probe (not part of the suite): what rendering into display surfaces costs on the device
(profiles/render_device.json).

Flights -- `--case gray1080` or `--case colour720`, one case per process: ONE flight of 32 device-fed frames (replicas of a
frame, staged with Batch.from_device) is coded once; then the routes alternate call by call, 1 warm-up round and `--reps`
rounds, and the decoder's own device time of every call (fiasco_amd_stats.decoder_us: HIP events around the uploads and the
kernels of the flight) is kept: median, min, max in microseconds.  Routes:
  shown        fiasco_amd_batch_decode_device_shown(b, 0, -1, ...), the path that existed before: the baseline of the run
  r16 r24 r32  fiasco_amd_batch_decode_device_rendered() at that depth (565, R G B bytes, XRGB8888), smoothing -1
  r16x2 ..     the same with every pixel doubled
The kernels alone -- `--kernels`, to be run under `rocprofv3 --kernel-trace --stats -d DIR -o kt --`: planes of 8192 x 4096
(gray) and 4096 x 4096 (colour) through fiasco_amd_planes_to_pixels_device() (oc_convert_kernel) and
fiasco_amd_planes_render_device() (rd_render_kernel) at the six formats, 1 warm-up and 5 timed launches each, in an order
the probe writes to `--order FILE`; `--summarise DB --order FILE` then reads the dispatches of the two kernels from the rocpd
database in that order and prints per launch kind the median kernel time and the bytes moved per second (the bytes the
algorithm needs: 2 per value read, the pixel bytes written, times four when doubled).
Every step under a time limit of its own, stopping at the first that fails:
  timeout -k 10 300 python tests/gpu_render_probe.py --case gray1080 && \\
  timeout -k 10 300 python tests/gpu_render_probe.py --case colour720 && \\
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tests/gpu_render_probe.py --kernels --order DIR/order.json && \\
  python tests/gpu_render_probe.py --summarise DIR/*/*_results.db --order DIR/order.json
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

CASES = {"gray1080": (1920, 1080, False), "colour720": (1280, 720, True)}
FORMATS = {"r16": (16, 0xf800, 0x07e0, 0x001f), "r24": (24, 0xff0000, 0x00ff00, 0x0000ff), "r32": (32, 0xff0000, 0x00ff00, 0x0000ff)}
FRAMES = 32
KERNEL_SHAPES = {"gray": (8192, 4096, False), "colour": (4096, 4096, True)}
WARM, TIMED = 1, 5


def renderers(fiasco_amd, lib):
    out = {}
    for n, (bpp, r, g, b) in FORMATS.items():
        out[n] = fiasco_amd.Renderer(lib, r, g, b, bpp, False)
        out[n + "x2"] = fiasco_amd.Renderer(lib, r, g, b, bpp, True)
    return out


def flights(a):
    import torch
    import fiasco_amd
    import synth
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.Library()
    lib.set_verbosity(0)
    w, h, colour = CASES[a.case]
    frame = synth.synth_color_k(w, h, 1234) if colour else synth.synth(w, h, 1234)
    src = torch.from_numpy(frame).cuda()
    o = lib.cli_options()
    b = fiasco_amd.Batch.from_device(lib, [src] * FRAMES, 20.0, o)
    assert None not in b.encode(), lib.error_message()
    rs = renderers(fiasco_amd, lib)
    full = list(torch.zeros((FRAMES, h, w, 3) if colour else (FRAMES, h, w), dtype=torch.uint8, device="cuda"))
    surf = {n: list(torch.zeros((FRAMES,) + r.surface_size(w, h, colour)[1::-1] + (r.bpp // 8,), dtype=torch.uint8, device="cuda")) for n, r in rs.items()}
    calls = {"shown": lambda: b.decode_shown(full)}
    for n, r in rs.items():
        calls[n] = (lambda n=n, r=r: b.decode_rendered(r, surf[n]))
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
    vals = w * h * (3 if colour else 1)
    res = {"case": a.case, "frames": FRAMES, "width": w, "height": h, "reps": a.reps, "device": torch.cuda.get_device_name(0), "decoder_us": {},
           "pixel_bytes_written_per_flight": {"shown": FRAMES * vals}}
    for n, v in us.items():
        res["decoder_us"][n] = {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}
    for n, r in rs.items():
        res["pixel_bytes_written_per_flight"][n] = FRAMES * w * h * (r.bpp // 8) * (4 if r.double_resolution else 1)
    print(json.dumps(res), flush=True)
    b.free(); o.delete()


def kernels(a):
    import numpy as np
    import torch
    import fiasco_amd
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.Library()
    lib.set_verbosity(0)
    rs = renderers(fiasco_amd, lib)
    order = []
    for kind, (w, h, colour) in KERNEL_SHAPES.items():
        rng = np.random.RandomState(3)
        planes = torch.from_numpy(rng.randint(-2200, 2200, size=(3, h, w) if colour else (h, w)).astype(np.int16)).cuda()
        vals = w * h * (3 if colour else 1)
        target = torch.zeros((h, w, 3) if colour else (h, w), dtype=torch.uint8, device="cuda")
        for rep in range(WARM + TIMED):
            fiasco_amd.planes_to_pixels_device(lib, planes, target)
            order.append({"kernel": "oc_convert_kernel", "kind": kind, "route": "pixels8", "timed": rep >= WARM, "bytes": 2 * vals + vals})
        del target
        for n, r in rs.items():
            sw, sh, row = r.surface_size(w, h, colour)
            s = torch.zeros((sh, sw, r.bpp // 8), dtype=torch.uint8, device="cuda")
            for rep in range(WARM + TIMED):
                fiasco_amd.render_planes_device(lib, r, planes, s)
                order.append({"kernel": "rd_render_kernel", "kind": kind, "route": n, "timed": rep >= WARM, "bytes": 2 * vals + sh * row})
            del s
        torch.cuda.synchronize()
    json.dump(order, open(a.order, "w"))
    print(json.dumps({"kernels": "launched", "dispatches": len(order)}), flush=True)


def summarise(a):
    order = json.load(open(a.order))
    con = sqlite3.connect(a.summarise)
    rows = [(name, end - start) for name, start, end in con.execute("select name, start, end from kernels order by start")
            if "oc_convert_kernel" in name or "rd_render_kernel" in name]
    assert len(rows) == len(order), (len(rows), len(order))
    got = {}
    for (name, ns), want in zip(rows, order):
        assert want["kernel"] in name, (name, want)
        if want["timed"]:
            got.setdefault((want["kind"], want["route"]), {"bytes": want["bytes"], "ns": []})["ns"].append(ns)
    res = {"kernels": {}}
    for (kind, route), v in got.items():
        med = statistics.median(v["ns"])
        res["kernels"].setdefault(kind, {})[route] = {"bytes": v["bytes"], "median_us": med / 1e3, "min_us": min(v["ns"]) / 1e3, "max_us": max(v["ns"]) / 1e3,
                                                     "n": len(v["ns"]), "GB_per_s": round(v["bytes"] / med, 1)}
    res["shapes"] = {k: {"width": w, "height": h, "colour": c} for k, (w, h, c) in KERNEL_SHAPES.items()}
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--order", default="render_order.json")
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
