#!/usr/bin/env python3
"""Developer probe (not part of the suite): what decoding a staged batch into device memory costs.

For a batch of replicas of one 1080p frame (1024 gray, 256 colour) two routes from the finished automata to pixels
are timed in ONE process and one run, on the same batch:
  device  Batch.decode_device() into one packed uint8 tensor: decoder flights + one oc_convert_kernel launch per
          flight, nothing copied to the host
  host    Batch.decode_psnr_all(): the same flights, then one blocking device-to-host copy per band and the PSNR
          sums on the host (the route that existed before; the comparison point)
For both: wall clock around the call + torch.cuda.synchronize(), and the decoder's own device time per frame
(fiasco_amd_stats.decoder_us / decoder_frames, HIP events around the flights).  profiles/bench_r06.json holds the
device time bench.py measured for the host route before this outlet existed ("config.decoder").

Method: one warm-up round of both first, then `--reps` repetitions, alternating; the median is the figure, min and
max are kept.  Writes profiles/decode_device.json."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fiasco_amd  # noqa: E402
import synth  # noqa: E402

W, H = 1920, 1080


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def probe(lib, n, color, reps):
    o = lib.cli_options()
    frame = synth.synth_color_k(W, H, 1234) if color else synth.synth(W, H, 1234)
    pnm = b"P%d\n%d %d\n255\n" % (6 if color else 5, W, H) + frame.tobytes()
    if color:                                       # 1080p colour at the CLI defaults needs > 6000 states per frame:
        lib.L.fiasco_amd_release_memory()           # the declared limits extension, as bench.py config3_pass
        lib.set_limits(30000, 26)
    b = fiasco_amd.Batch(lib, [pnm] * n, 20.0, o)
    assert None not in b.encode(), lib.error_message()
    out = torch.zeros((n, H, W, 3) if color else (n, H, W), dtype=torch.uint8, device="cuda")
    targets = list(out)
    res = {"frames": n, "color": bool(color), "width": W, "height": H}
    wall = {"device": [], "host": []}
    us = {"device": [], "host": []}
    for r in range(reps + 1):                       # round 0 warms up
        for route in ("device", "host"):
            lib.reset_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            good = b.decode_device(targets) if route == "device" else b.decode_psnr_all()[0]
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            st = lib.get_stats()
            assert good == n and st.decoder_frames == n, (route, good, lib.error_message())
            if r:
                wall[route].append((t1 - t0) * 1e3)
                us[route].append(st.decoder_us / st.decoder_frames)
    assert bool((out == out[0]).all()), "replicas of one frame decode to one picture"
    for route in ("device", "host"):
        res["wall_ms_" + route] = stat(wall[route])
        res["decoder_us_per_frame_" + route] = stat(us[route])
    res["wall_ratio_host_over_device"] = res["wall_ms_host"]["median"] / res["wall_ms_device"]["median"]
    b.free(); o.delete()
    if color:
        lib.set_limits(6000, 22)
        lib.L.fiasco_amd_release_memory()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--color-frames", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_device.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    parent = json.load(open(os.path.join(ROOT, "profiles", "bench_r06.json")))["config"]["decoder"]
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "bench_r06_decoder_us_per_frame": 1e6 * parent["device_seconds"] / parent["frames"], "cases": []}
    for color, n in ((0, a.frames), (1, a.color_frames)):
        if n:
            res["cases"].append(probe(lib, n, color, a.reps))
            print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
