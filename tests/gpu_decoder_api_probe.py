#!/usr/bin/env python3
"""Measured, not gated: what playing a stream through fiasco_decoder_get_frame costs beside Stream.decode_device over the
same stream in the same run -> profiles/decoder_api.json (or the file named behind --out).  Run on an MI355X:
    python tests/gpu_decoder_api_probe.py

The streams are those of tests/gpu_stream_probe.py: 32 gray 1080p intra frames, and a 30-frame 720p `ippppppppp'.  Per stream:
  stream_decode_device   Stream.decode_device(smoothing=0) into 8-bit targets: the path that was there before
  get_frame_ahead_32     a new Decoder, one get_frame per display frame, every image deleted; read-ahead 32
  get_frame_ahead_1      the same at read-ahead 1: one device call per display frame
  get_frame_render       the read-ahead 32 loop with fiasco_renderer_render of every image into a host XImage (32 bpp)
Every figure is for the whole stream, parsing included for the Decoder loops (fiasco_amd_decoder_new_memory is inside the
interval: a decoder plays once).  HIP events on the current stream AND the wall clock around the call, the median of 20 after
3 warm-up calls; the spread is (max - min) / median of the wall clock."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import fiasco_amd  # noqa: E402
import synth  # noqa: E402

REPEATS, WARMUP = 20, 3


def timed(call, frames):
    ev, wall = [], []
    for k in range(WARMUP + REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= WARMUP:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1000.0)
    med = statistics.median(wall)
    return {"wall_median_ms": round(med, 3), "wall_min_ms": round(min(wall), 3), "wall_max_ms": round(max(wall), 3),
            "spread": round((max(wall) - min(wall)) / med, 3), "events_median_ms": round(statistics.median(ev), 3),
            "per_frame_ms": round(med / frames, 3)}


def play(lib, data, ahead, renderer=None):
    d = fiasco_amd.Decoder(lib, data, smoothing=0, read_ahead=ahead)
    n = 0
    for image in d:
        if renderer is not None:
            image.render(renderer)
        image.delete()
        n += 1
    d.delete()
    return n


def measure(lib, data, targets, renderer):
    s = fiasco_amd.Stream(lib, data)
    n = s.n
    assert s.decode_device(targets, smoothing=0) == n and play(lib, data, 32) == n
    out = {"frames": n, "parse_ms": timed(lambda: fiasco_amd.Stream(lib, data).free(), n)["wall_median_ms"],
           "stream_decode_device": timed(lambda: s.decode_device(targets, smoothing=0), n),
           "get_frame_ahead_32": timed(lambda: play(lib, data, 32), n),
           "get_frame_ahead_1": timed(lambda: play(lib, data, 1), n),
           "get_frame_render": timed(lambda: play(lib, data, 32, renderer), n)}
    s.free()
    return out


def main():
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "decoder_api.json")
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    lib.set_device(0)
    out = {"device": torch.cuda.get_device_name(0), "repeats": REPEATS, "warmup": WARMUP}
    renderer = fiasco_amd.Renderer(lib, 0xff0000, 0x00ff00, 0x0000ff, 32)
    frames = [synth.pgm_bytes(synth.synth(1920, 1080, 100 + i)) for i in range(32)]
    seq = fiasco_amd.Sequence(lib, frames, 20.0, lib.cli_options(pattern="i"))
    data = seq.encode()
    seq.free()
    out["intra_1080p_x32"] = measure(lib, data, [torch.empty((1080, 1920), dtype=torch.uint8, device="cuda") for _ in range(32)], renderer)
    big = synth.synth(1280 + 100, 720 + 70, 7)
    video = [synth.pgm_bytes(np.ascontiguousarray(big[2 * i:720 + 2 * i, 3 * i:1280 + 3 * i])) for i in range(30)]
    seq = fiasco_amd.Sequence(lib, video, 20.0, lib.cli_options(pattern="ippppppppp"))
    data = seq.encode()
    seq.free()
    out["chain_720p_x30"] = measure(lib, data, [torch.empty((720, 1280), dtype=torch.uint8, device="cuda") for _ in range(30)], renderer)
    renderer.delete()
    os.makedirs(os.path.dirname(path), exist_ok=True)
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
