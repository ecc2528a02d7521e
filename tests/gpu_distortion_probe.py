#!/usr/bin/env python3
"""Developer probe (not part of the suite): what measuring the decoded distortion of a staged batch costs.

For a batch of replicas of one 1080p frame (1024 gray, 256 colour), staged from PNM and staged from device memory, two
routes from the finished automata to "how good is it" are timed in ONE process and one run, on the same batch:
  device  Batch.decode_distortion_device(): decoder flights + one ds_distortion_kernel launch per flight; 12 bytes per
          band come back.  PNM-fed frames: the original planes go up into the flight's arena first
  legacy  Batch.decode_psnr_all(): the same flights, then one blocking device-to-host copy per band and the float sums
          on host threads (the route that existed before; the comparison point).  A device-fed frame's original planes
          are fetched to the host by the first call and kept: that call is reported on its own ("first")
For both: wall clock around the call + torch.cuda.synchronize(), and the decoder's own device time per frame
(fiasco_amd_stats.decoder_us / decoder_frames, HIP events around the flights: uploads, kernels, the measuring launch).

Method: one first round of both (reported as "first": it warms up, and holds the legacy route's fetch), then `--reps`
repetitions, alternating; the median is the figure, min and max are kept.  Writes profiles/decode_distortion.json."""
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


def probe(lib, n, color, fed, reps):
    o = lib.cli_options()
    frame = synth.synth_color_k(W, H, 1234) if color else synth.synth(W, H, 1234)
    if color:                                       # 1080p colour at the CLI defaults needs > 6000 states per frame:
        lib.L.fiasco_amd_release_memory()           # the declared limits extension, as bench.py config3_pass
        lib.set_limits(30000, 26)
    if fed == "device":
        src = torch.from_numpy(frame).cuda().unsqueeze(0).repeat(n, *([1] * frame.ndim))
        b = fiasco_amd.Batch.from_device(lib, list(src), 20.0, o)
    else:
        pnm = b"P%d\n%d %d\n255\n" % (6 if color else 5, W, H) + frame.tobytes()
        b = fiasco_amd.Batch(lib, [pnm] * n, 20.0, o)
    assert None not in b.encode(), lib.error_message()
    res = {"frames": n, "color": bool(color), "fed": fed, "width": W, "height": H}
    wall = {"device": [], "legacy": []}
    us = {"device": [], "legacy": []}
    got = {}
    for r in range(reps + 1):                       # round 0: the first calls
        for route in ("device", "legacy"):
            lib.reset_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = b.decode_distortion_device() if route == "device" else b.decode_psnr_all()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            st = lib.get_stats()
            assert out[0] == n and st.decoder_frames == n, (route, out[0], lib.error_message())
            if r:
                wall[route].append((t1 - t0) * 1e3)
                us[route].append(st.decoder_us / st.decoder_frames)
            else:
                res["wall_ms_%s_first" % route] = (t1 - t0) * 1e3
            assert got.setdefault(route, out) == out, "two runs of one route give the same numbers"
    sse, mse = got["device"][1], got["legacy"][2]
    assert all(s == sse[0] for s in sse), "replicas of one frame have one distortion"
    res["sse"], res["maxdiff"], res["psnr_db"] = sse[0], got["device"][2][0], got["device"][3][0]
    res["legacy_mse"], res["exact_mse"] = mse[0], [s / (W * H) for s in sse[0]]
    for route in ("device", "legacy"):
        res["wall_ms_" + route] = stat(wall[route])
        res["decoder_us_per_frame_" + route] = stat(us[route])
    res["wall_ratio_legacy_over_device"] = res["wall_ms_legacy"]["median"] / res["wall_ms_device"]["median"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode_distortion.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "cases": []}
    for color, n in ((0, a.frames), (1, a.color_frames)):
        for fed in ("device", "pnm"):
            if n:
                res["cases"].append(probe(lib, n, color, fed, a.reps))
                print(json.dumps(res["cases"][-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
