#!/usr/bin/env python3
"""Developer probe (not part of the suite): what the magnified decodes cost on the device.

One case per process -- `--case gray1080` or `--case colour720` --: ONE flight of 32 device-fed frames (replicas of a
frame, staged with Batch.from_device) is coded once, then every route is called 1 + `--reps` times (the first call warms
up) and the decoder's own device time of the call (fiasco_amd_stats.decoder_us: HIP events around the uploads and kernels
of the flight) is kept: median, min, max in microseconds.  Routes:
  old         fiasco_amd_batch_decode_device(), the entry that existed before
  mag0        fiasco_amd_batch_decode_device_magnified(b, 0, ...): must cost what `old' costs
  mag-1 mag-2 thumbnails alone: the level launches stop 2 k levels early
  thumbs2     fiasco_amd_batch_decode_device_thumbnails(b, targets, 2, thumbs): the full frames AND the thumbnails of
              mag-2 from one decode; against `old' this is the price of the gather and the second conversion launch
Enlargements are kept out: they multiply the level images by 4^M.  After every route the device is
synchronised and the error state read, so a failure names its route.  `--lib` takes another build of the library (the
parent commit's, which has `old' only: `--routes old').  Run the cases one after the other, each under a time limit of
its own, and stop at the first that fails:
  timeout -k 10 240 python tests/gpu_magnify_probe.py --case gray1080 && \\
  timeout -k 10 240 python tests/gpu_magnify_probe.py --case colour720
Prints one JSON line per case."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fiasco_amd  # noqa: E402
import synth  # noqa: E402

CASES = {"gray1080": (1920, 1080, False), "colour720": (1280, 720, True)}
ROUTES = ["old", "mag0", "mag-1", "mag-2", "thumbs2"]
FRAMES = 32


def shown(w, h, m):
    """the size at magnification m, without the library (the parent's has no fiasco_amd_magnified_size)"""
    if m >= 0:
        return w << m, h << m
    w, h = w >> -m, h >> -m
    return w + (w & 1), h + (h & 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=sorted(CASES), required=True)
    ap.add_argument("--routes", default=",".join(ROUTES))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--lib", default=fiasco_amd.LIB_PATH)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.Library(a.lib)
    assert lib.core_name() == "hip-gfx950"
    lib.set_verbosity(0)
    w, h, colour = CASES[a.case]
    frame = synth.synth_color_k(w, h, 1234) if colour else synth.synth(w, h, 1234)
    src = torch.from_numpy(frame).cuda()
    o = lib.cli_options()
    b = fiasco_amd.Batch.from_device(lib, [src] * FRAMES, 20.0, o)
    assert None not in b.encode(), lib.error_message()

    def tensors(m):
        tw, th = shown(w, h, m)
        return list(torch.zeros((FRAMES, th, tw, 3) if colour else (FRAMES, th, tw), dtype=torch.uint8, device="cuda"))

    full = tensors(0)
    small = {m: tensors(m) for m in (-1, -2)}
    c = ctypes
    if "mag0" in a.routes.split(","):
        fm = lib.L.fiasco_amd_batch_decode_device_magnified
        fm.argtypes = [c.c_void_p, c.c_int, c.POINTER(fiasco_amd.DeviceTarget), c.c_void_p]
        fm.restype = c.c_int
        full_arr = fiasco_amd._device_targets(full)
    calls = {
        "old": lambda: b.decode_device(full),
        "mag0": lambda: fm(b.handle, 0, full_arr, None),
        "mag-1": lambda: b.decode_device(small[-1], magnify=-1),
        "mag-2": lambda: b.decode_device(small[-2], magnify=-2),
        "thumbs2": lambda: b.decode_thumbnails(full, 2, small[-2]),
    }
    res = {"case": a.case, "frames": FRAMES, "width": w, "height": h, "reps": a.reps, "lib": os.path.relpath(a.lib, ROOT), "decoder_us": {}}
    for route in a.routes.split(","):
        us = []
        for r in range(a.reps + 1):
            lib.reset_stats()
            good = calls[route]()
            torch.cuda.synchronize()                                # a failure surfaces here, under its route's name
            st = lib.get_stats()
            assert good == FRAMES and st.decoder_frames == FRAMES, (route, good, lib.error_message())
            if r:
                us.append(int(st.decoder_us))
        res["decoder_us"][route] = {"median": statistics.median(us), "min": min(us), "max": max(us)}
        print("%s %s: %s" % (a.case, route, res["decoder_us"][route]), file=sys.stderr, flush=True)
    print(json.dumps(res), flush=True)
    b.free(); o.delete()


if __name__ == "__main__":
    main()
