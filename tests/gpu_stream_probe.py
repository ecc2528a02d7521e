#!/usr/bin/env python3
"""Measured, not gated: what decoding a stream costs on the device -> profiles/stream_decode.json.  Run on an MI355X:
    python tests/gpu_stream_probe.py            the timings
    python tests/gpu_stream_probe.py --once     one decode of each stream and nothing else: the program of a
                                                `rocprofv3 --kernel-trace --stats -- python tests/gpu_stream_probe.py --once` run,
                                                whose launches per frame go into the file by hand

  intra    an all-intra stream of 32 gray 1080p frames through Stream.decode_device(smoothing=0), and the same frames
           through Batch.decode_shown(smoothing=0) of the batch that coded them: the flights are the same, the two should
           agree within the spread
  chain    a 30-frame 720p `ippppppppp' stream through Stream.decode_device: one frame per flight
HIP events around the call on the caller's stream, the median of 20 after 3 warm-up calls; the spread is (max - min) / median."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fiasco_amd  # noqa: E402
import synth  # noqa: E402

REPEATS, WARMUP = 20, 3


def timed(call):
    ms = []
    for k in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        if k >= WARMUP:
            ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return {"median_ms": round(med, 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "spread": round((max(ms) - min(ms)) / med, 3)}


def main():
    once = "--once" in sys.argv
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    lib.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "warmup": WARMUP}
    # all-intra: 32 gray 1080p frames
    o = lib.cli_options()
    frames = [synth.pgm_bytes(synth.synth(1920, 1080, 100 + i)) for i in range(32)]
    b = fiasco_amd.Batch(lib, frames, 20.0, o)
    streams = b.encode()
    seq = fiasco_amd.Sequence(lib, frames, 20.0, lib.cli_options(pattern="i"))
    s = fiasco_amd.Stream(lib, seq.encode())
    seq.free()
    tg = [torch.empty((1080, 1920), dtype=torch.uint8, device="cuda") for _ in range(32)]
    tb = [torch.empty((1080, 1920), dtype=torch.uint8, device="cuda") for _ in range(32)]
    assert s.decode_device(tg, smoothing=0) == 32 and b.decode_shown(tb, smoothing=0) == 32
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(tg, tb)) and None not in streams
    if not once:
        out["intra_1080p_x32"] = {"stream_decode_device": timed(lambda: s.decode_device(tg, smoothing=0)),
                                  "batch_decode_shown": timed(lambda: b.decode_shown(tb, smoothing=0))}
    s.free(); b.free()
    # a chain of P frames: 30 frames of 720p, a window that moves by (3, 2) pixels per frame
    big = synth.synth(1280 + 100, 720 + 70, 7)
    video = [synth.pgm_bytes(np.ascontiguousarray(big[2 * i:720 + 2 * i, 3 * i:1280 + 3 * i])) for i in range(30)]
    seq = fiasco_amd.Sequence(lib, video, 20.0, lib.cli_options(pattern="ippppppppp"))
    v = fiasco_amd.Stream(lib, seq.encode())
    seq.free()
    assert v.frame_types == [0 if d % 10 == 0 else 1 for d in range(30)]
    tv = [torch.empty((720, 1280), dtype=torch.uint8, device="cuda") for _ in range(30)]
    assert v.decode_device(tv, smoothing=0) == 30
    if not once:
        t = timed(lambda: v.decode_device(tv, smoothing=0))
        out["chain_720p_x30"] = dict(t, per_frame_ms=round(t["median_ms"] / 30, 3), flights=30)
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        path = os.path.join(ROOT, "profiles", "stream_decode.json")
        old = json.load(open(path)) if os.path.exists(path) else {}
        out["launches_per_frame"] = old.get("launches_per_frame")          # from the --once run under rocprofv3
        json.dump(out, open(path, "w"), indent=1)
        print(json.dumps(out))
    v.free()


if __name__ == "__main__":
    main()
