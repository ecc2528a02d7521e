#!/usr/bin/env python3
"""Developer probe (not part of the suite): what decoding in 4:2:0 into display surfaces costs on the device beside the paths
that existed before.  Its JSON lines belong in profiles/render_420_device.json; no run of it is recorded yet.

Flights -- `--case colour720` or `--case colour1080`, one case per process: ONE flight of 32 device-fed colour frames
(replicas of a frame, staged with Batch.from_device) is coded once; then the routes take turns call by call, 1 warm-up round
and `--reps` rounds (default 20).  Every call is timed twice: with HIP events on the caller's stream around the call (what a
caller waits for: the decoder's work, the table uploads and the rendering), and by the decoder's own device time
(fiasco_amd_stats.decoder_us).  Median, min, max in microseconds.  Routes, all at smoothing -1:
  r32_444            fiasco_amd_batch_decode_device_rendered() at 32 bpp: the 4:4:4 path into surfaces
  i420               fiasco_amd_batch_decode_device_420() into packed I420 buffers: the 4:2:0 path into bytes
  r16 r24 r32        fiasco_amd_batch_decode_device_rendered_420() at that depth (565, R G B bytes, XRGB8888)
  r16x2 r24x2 r32x2  the same with every pixel doubled
The kernels alone -- `--kernels`, to be run under `rocprofv3 --kernel-trace --stats -d DIR -o kt --`: colour planes of 4096 x
4096 through fiasco_amd_planes_render_device() (rd_render_kernel) and the same Y plane with chroma planes of 2048 x 2048
through fiasco_amd_planes_render_device_420() (rd420_render_kernel) into the same surfaces at the six formats, 1 warm-up and 5
timed launches each, the whole sequence twice (repeat 0 and 1: their difference is the spread of the measurement), in an
order the probe writes to `--order FILE`; `--summarise DB --order FILE` then reads the dispatches of the two kernels from the
rocpd database in that order and prints per kernel, format and repeat the median kernel time and the bytes moved per second
(the bytes the algorithm needs: 6 per pixel read at 4:4:4, 3 at 4:2:0, the pixel bytes written, times four when doubled).
Every step under a time limit of its own, stopping at the first that fails:
  timeout -k 10 300 python tests/gpu_render_420_probe.py --case colour720 && \\
  timeout -k 10 400 python tests/gpu_render_420_probe.py --case colour1080 && \\
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d DIR -o kt -- python tests/gpu_render_420_probe.py --kernels --order DIR/order.json && \\
  python tests/gpu_render_420_probe.py --summarise DIR/*/*_results.db --order DIR/order.json
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

CASES = {"colour720": (1280, 720), "colour1080": (1920, 1080)}
FORMATS = {"r16": (16, 0xf800, 0x07e0, 0x001f), "r24": (24, 0xff0000, 0x00ff00, 0x0000ff), "r32": (32, 0xff0000, 0x00ff00, 0x0000ff)}
FRAMES = 32
KERNEL_SHAPE = (4096, 4096)
WARM, TIMED, REPEATS = 1, 5, 2


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
    w, h = CASES[a.case]
    src = torch.from_numpy(synth.synth_color_k(w, h, 1234)).cuda()
    o = lib.cli_options()
    b = fiasco_amd.Batch.from_device(lib, [src] * FRAMES, 20.0, o)
    assert None not in b.encode(), lib.error_message()
    rs = renderers(fiasco_amd, lib)
    surf = {n: list(torch.zeros((FRAMES,) + r.surface_size_420(w, h)[1::-1] + (r.bpp // 8,), dtype=torch.uint8, device="cuda")) for n, r in rs.items()}
    ys = list(torch.zeros((FRAMES, h, w), dtype=torch.uint8, device="cuda"))
    cbs = list(torch.zeros((FRAMES, h // 2, w // 2), dtype=torch.uint8, device="cuda"))
    crs = list(torch.zeros((FRAMES, h // 2, w // 2), dtype=torch.uint8, device="cuda"))
    calls = {"r32_444": lambda: b.decode_rendered(rs["r32"], surf["r32"]), "i420": lambda: b.decode_420(list(zip(ys, cbs, crs)))}
    for n, r in rs.items():
        calls[n] = (lambda n=n, r=r: b.decode_rendered_420(r, surf[n]))
    ev_us, dec_us = {n: [] for n in calls}, {n: [] for n in calls}
    for rep in range(a.reps + 1):
        for route, call in calls.items():
            lib.reset_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            good = call()
            e1.record()
            torch.cuda.synchronize()                                # a failure surfaces here, under its route's name
            st = lib.get_stats()
            assert good == FRAMES and st.decoder_frames == FRAMES, (route, good, lib.error_message())
            if rep:
                ev_us[route].append(e0.elapsed_time(e1) * 1e3)
                dec_us[route].append(int(st.decoder_us))

    def stats(v):
        return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1), "n": len(v)}
    res = {"case": a.case, "frames": FRAMES, "width": w, "height": h, "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "stream_event_us": {n: stats(v) for n, v in ev_us.items()}, "decoder_us": {n: stats(v) for n, v in dec_us.items()},
           "bytes_written_per_flight": {"r32_444": FRAMES * w * h * 4, "i420": FRAMES * w * h * 3 // 2}}
    for n, r in rs.items():
        res["bytes_written_per_flight"][n] = FRAMES * w * h * (r.bpp // 8) * (4 if r.double_resolution else 1)
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
    w, h = KERNEL_SHAPE
    rng = np.random.RandomState(3)
    planes = torch.from_numpy(rng.randint(-2200, 2200, size=(3, h, w)).astype(np.int16)).cuda()
    cb = torch.from_numpy(rng.randint(-2200, 2200, size=(h // 2, w // 2)).astype(np.int16)).cuda()
    cr = torch.from_numpy(rng.randint(-2200, 2200, size=(h // 2, w // 2)).astype(np.int16)).cuda()
    for repeat in range(REPEATS):
        for n, r in rs.items():
            sw, sh, row = r.surface_size_420(w, h)
            s = torch.zeros((sh, sw, r.bpp // 8), dtype=torch.uint8, device="cuda")
            for rep in range(WARM + TIMED):
                fiasco_amd.render_planes_device(lib, r, planes, s)
                order.append({"kernel": "rd_render_kernel", "route": n, "repeat": repeat, "timed": rep >= WARM, "bytes": 6 * w * h + sh * row})
            for rep in range(WARM + TIMED):
                fiasco_amd.render_planes_device_420(lib, r, planes[0], cb, cr, s)
                order.append({"kernel": "rd420_render_kernel", "route": n, "repeat": repeat, "timed": rep >= WARM, "bytes": 3 * w * h + sh * row})
            del s
        torch.cuda.synchronize()
    json.dump(order, open(a.order, "w"))
    print(json.dumps({"kernels": "launched", "dispatches": len(order)}), flush=True)


def summarise(a):
    order = json.load(open(a.order))
    con = sqlite3.connect(a.summarise)
    rows = [(name, end - start) for name, start, end in con.execute("select name, start, end from kernels order by start")
            if "rd420_render_kernel" in name or "rd_render_kernel" in name]
    assert len(rows) == len(order), (len(rows), len(order))
    got = {}
    for (name, ns), want in zip(rows, order):
        assert want["kernel"] in name, (name, want)
        if want["timed"]:
            got.setdefault((want["kernel"], want["route"], want["repeat"]), {"bytes": want["bytes"], "ns": []})["ns"].append(ns)
    res = {"kernels": {}, "shape": {"width": KERNEL_SHAPE[0], "height": KERNEL_SHAPE[1]}}
    for (kernel, route, repeat), v in got.items():
        med = statistics.median(v["ns"])
        res["kernels"].setdefault(route, {}).setdefault(kernel, []).append(
            {"repeat": repeat, "bytes": v["bytes"], "median_us": med / 1e3, "min_us": min(v["ns"]) / 1e3, "max_us": max(v["ns"]) / 1e3, "n": len(v["ns"]),
             "GB_per_s": round(v["bytes"] / med, 1)})
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--order", default="render_420_order.json")
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
