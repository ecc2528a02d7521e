"""A flight of mixed sizes decoded as `dfiasco' shows it, in a process of its own: tests/test_gpu_shown.py starts this file
twice, once with the developer switch FIASCO_AMD_SMOOTH_FUSED=0 (every smoothed plane through the per-pass launches) and
once with =1 (every one through the fused kernel), and compares what the two print -- one JSON line: the md5 of every
output of the calls below.  The switch is read when a flight is prepared, so it has to be in the environment of the
process; FIASCO_AMD_DEBUG=1 makes the library honour it.  Not a test file."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch                                       # before the product library: one HIP runtime for both

import fiasco_amd
import synth

MAGS = (-1, 0, 1)


def frames():
    """34 gray frames -- two flights -- of four sizes, the ragged ones included"""
    sizes = [(64, 64), (100, 70), (130, 66), (256, 256)]
    return [synth.synth(w, h, 900 + i) if i % 7 else synth.noise(w, h, 900 + i) for i, (w, h) in ((i, sizes[i % 4]) for i in range(34))]


def md5(t):
    return hashlib.md5(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


def main():
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    o = lib.cli_options()
    arrs = frames()
    b = fiasco_amd.Batch(lib, [synth.pgm_bytes(a) for a in arrs], 20.0, o)
    assert None not in b.encode(), lib.error_message()
    out = {"switch": os.environ.get("FIASCO_AMD_SMOOTH_FUSED"), "shown": {}, "thumbs": {}, "pairs": []}
    for m in MAGS:
        sizes = [fiasco_amd.magnified_size(lib, w, h, m) for w, h, _ in b._geom]
        ts = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for w, h in sizes]
        assert b.decode_shown(ts, magnify=m, smoothing=70) == len(arrs), lib.error_message()
        out["shown"][str(m)] = [md5(t) for t in ts]
    sizes = [fiasco_amd.magnified_size(lib, w, h, -1) for w, h, _ in b._geom]
    full = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for w, h, _ in b._geom]
    small = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for w, h in sizes]
    assert b.decode_thumbnails(full, 1, small, smoothing=70) == len(arrs), lib.error_message()
    out["thumbs"] = {"full": [md5(t) for t in full], "small": [md5(t) for t in small]}
    for i in range(4):
        for m in MAGS:
            borders = b.smoothing_borders(i, magnify=m)
            out["pairs"].append(sum(x[2] for x in borders))
    b.free(); o.delete()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
