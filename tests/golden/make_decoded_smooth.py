#!/usr/bin/env python3
"""Smoothed decoded frames of the REAL reference: for the stills below `cfiasco_ref <args> --smooth S' codes the input
and `dfiasco_ref -s N -o' decodes the stream for N in -1, 0, 1, 35, 70, 100; the md5 of the pixel bytes of every
decode goes into tests/golden/DECODED_SMOOTH.json.  N = -1 takes the percentage from the stream header (S, 70 unless
a case says otherwise); N > 0 smooths the frame along the partition borders (smooth_image, codec/decoder.c:674-768).
The numpy restatement (tests/smooth_ref.py) applied to the library's border list
(fiasco_amd_batch_smoothing_borders) must give them from the oracle's decoded planes (tests/test_smoothing_api.py).
tests/conftest.py options_from_args() does not know --smooth: a case carries the value on its own and the tests call
set_smoothing() after options_from_args().  Build container only (oracle/_ref from oracle/ref_build.sh)."""
import hashlib
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
from conftest import GOLDEN, REF_SHARE  # noqa: E402

# (name, input, MANIFEST case whose arguments are used, smoothing written into the stream header)
# carry48_a / carry74_a: colour, and the two frames on which the order of the Y and the Cb borders shows in the bytes;
# g100x70: gray, ragged (borders clipped at the frame); g64x32: gray, the smallest; c256: colour, as DECODED_RGB.json;
# g100x70 once more with 35 in the header, so that -1 is not 70; a second frame of 64 x 32 (input "synth:W:H:SEED":
# synth.synth(W, H, SEED) as a PGM), so that a flight can hold frames that differ
CASES = [
    ("carry48_a", "carry48_a", "seq3_color_carry48", 70),
    ("carry74_a", "carry74_a", "seq3_color_carry74", 70),
    ("g100x70", "g100x70", "g100x70_q20", 70),
    ("g64x32", "g64x32", "g64x32_q20", 70),
    ("c256", "c256", "c256_q20", 70),
    ("g100x70_s35", "g100x70", "g100x70_q20", 35),
    ("g64x32_b", "synth:64:32:17", "g64x32_q20", 70),
]
LEVELS = [-1, 0, 1, 35, 70, 100]
REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_smooth"
TOOLS = "cfiasco_ref <args> --smooth S -o ref.fco in; dfiasco_ref -s N -o dec ref.fco; decoded_md5[N] = md5 of dec's pixel bytes"


def input_of(inp):
    if inp.startswith("synth:"):
        import synth
        w, h, seed = (int(v) for v in inp.split(":")[1:])
        return synth.pgm_bytes(synth.synth(w, h, seed)), "pgm"
    return make_golden.make_input(inp)


def main():
    os.makedirs(TMP, exist_ok=True)
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    cases = {c["name"]: c for c in man["cases"]}
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    out = {}
    for name, inp, of, smooth in CASES:
        args = cases[of]["args"]
        data, ext = input_of(inp)
        src = os.path.join(TMP, name + "." + ext)
        open(src, "wb").write(data)
        fco = os.path.join(TMP, name + ".fco")
        subprocess.check_call([os.path.join(REFDIR, "cfiasco_ref"), "--progress-meter", "0"] + args
                              + ["--smooth", str(smooth), "-o", fco, src], env=env, stderr=subprocess.DEVNULL)
        stream = open(fco, "rb").read()
        md5s = {}
        w = h = None
        for n in LEVELS:
            dec = os.path.join(TMP, "%s.s%d.%s" % (name, n, ext))
            subprocess.check_call([os.path.join(REFDIR, "dfiasco_ref"), "-s", str(n), "-o", dec, fco], env=env, stderr=subprocess.DEVNULL)
            raw = open(dec, "rb").read()
            assert raw[:2] == (b"P6" if ext == "ppm" else b"P5"), name
            w, h = [int(v) for v in raw.split(b"\n", 2)[1].split()]
            md5s[str(n)] = hashlib.md5(raw[len(raw) - (3 if ext == "ppm" else 1) * w * h:]).hexdigest()
        # conditions the tests rely on
        for n in LEVELS:
            assert n <= 0 or md5s[str(n)] != md5s["0"], "%s: -s %d changes nothing; take another case" % (name, n)
        assert md5s["-1"] == md5s[str(smooth)], name
        if smooth != 70:
            assert md5s["-1"] != md5s["70"], name
        out[name] = {"input": inp, "args": args, "smoothing": smooth, "stream_md5": hashlib.md5(stream).hexdigest(),
                     "width": w, "height": h, "color": ext == "ppm", "decoded_md5": md5s, "tools": TOOLS}
        print("%-12s %4d x %-4d %s" % (name, w, h, " ".join("%d:%s" % (n, md5s[str(n)][:8]) for n in LEVELS)))
    with open(os.path.join(HERE, "DECODED_SMOOTH.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_decoded_smooth.py", "cases": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
