#!/usr/bin/env python3
"""Frames as the REAL reference's decoder SHOWS them at every magnification: for the stills below `cfiasco_ref <args>
--smooth S' codes the input and `dfiasco_ref -s N -m M -o' decodes the stream for M in -3 .. 3 and N in -1, 0, 35, 70
(get_next_frame, codec/decoder.c:317-377: enlarge_image, the decode, smooth_image on the shifted automaton).  Per M
tests/golden/DECODED_SHOWN.json records the width, the height and per N the md5 of the pixel bytes, or that the reference
refused M and the limit its message names (codec/dfiasco.c:104-137).  N = 0 is there for the generator's own assertions
and for the tests that tell a smoothed frame from an unsmoothed one.  The device decoder must give the same bytes
(tests/test_gpu_shown.py) and the library's border lists must be the coded lists shifted (tests/test_shown_api.py).
M = 3 only where a case says so (one gray, one colour): the frames stay small.
Build container only (oracle/_ref from oracle/ref_build.sh)."""
import hashlib
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402
import shown_ref  # noqa: E402
from conftest import GOLDEN, REF_SHARE  # noqa: E402

# (name, input, MANIFEST case whose arguments are used, further arguments, smoothing in the stream header, largest M)
# g256: gray, states from level 7 down to 1 at -3; c256sq: colour, 256 x 256, the only colour case that reaches -3 (Cb
# phase); c256: colour, 256 x 192, down to -2; g100x70 / g130x66: ragged, 50 x 36 and 66 x 34 at -1 (borders clipped at a
# size rounded up to even); carry74_a: colour, the frame on which the order of the Y and the Cb passes shows; noise256: a
# border on nearly every block; g256_z1_q300: states of level 5, which fall to level -1 at -3 -- the library refuses that
# one, the reference decodes it; g100x70_s35: 35 in the header, so that -1 is not 70
CASES = [
    ("g256", "g256", "g256_q20", [], 70, 2),
    ("g256_q60", "g256", "g256_q60", [], 70, 2),
    ("c256sq", "synthrgb:256:256:47:48:49", "c256_q20", [], 70, 2),
    ("c256", "c256", "c256_q20", [], 70, 2),
    ("g100x70", "g100x70", "g100x70_q20", [], 70, 3),
    ("g130x66", "synth:130:66:19", "g100x70_q20", [], 70, 2),
    ("carry74_a", "carry74_a", "seq3_color_carry74", [], 70, 3),
    ("noise256", "noise:256:256:11", "g256_q20", ["-q", "100"], 70, 2),
    ("g256_z1_q300", "g256", "g256_z1", ["-q", "300"], 70, 2),
    ("g100x70_s35", "g100x70", "g100x70_q20", [], 35, 2),
]
LEVELS = [-1, 0, 35, 70]
REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_shown"
TOOLS = ("cfiasco_ref <args> --smooth S -o ref.fco in; dfiasco_ref -s N -m M -o dec ref.fco; shown[M] = width, height and "
         "md5[N] of dec's pixel bytes, or refused + the limit the message names")


def main():
    os.makedirs(TMP, exist_ok=True)
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    cases = {c["name"]: c for c in man["cases"]}
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    out = {}
    for name, inp, of, more, smooth, top in CASES:
        args = cases[of]["args"] + more
        data, ext = shown_ref.synth_input(inp) or make_golden.make_input(inp)
        src = os.path.join(TMP, name + "." + ext)
        open(src, "wb").write(data)
        fco = os.path.join(TMP, name + ".fco")
        subprocess.check_call([os.path.join(REFDIR, "cfiasco_ref"), "--progress-meter", "0"] + args
                              + ["--smooth", str(smooth), "-o", fco, src], env=env, stderr=subprocess.DEVNULL)
        stream = open(fco, "rb").read()
        recs = {}
        for m in range(-3, top + 1):
            md5s, size, limit = {}, None, None
            for n in LEVELS:
                dec = os.path.join(TMP, "%s.m%d.s%d.%s" % (name, m, n, ext))
                if os.path.exists(dec):
                    os.remove(dec)
                r = subprocess.run([os.path.join(REFDIR, "dfiasco_ref"), "-s", str(n), "-m", str(m), "-o", dec, fco], env=env,
                                   stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
                said = r.stdout.decode("latin-1")
                lim = re.search(r"(Minimum|Maximium) value is (-?\d+)", said)
                if lim:
                    assert not os.path.exists(dec), (name, m)
                    limit = {"refused": "minimum" if lim.group(1) == "Minimum" else "maximum", "limit": int(lim.group(2))}
                    continue
                assert r.returncode == 0 and limit is None, (name, m, n, said)
                raw = open(dec, "rb").read()
                assert raw[:2] == (b"P6" if ext == "ppm" else b"P5"), name
                w, h = [int(v) for v in raw.split(b"\n", 2)[1].split()]
                assert size in (None, (w, h)), (name, m)
                size = (w, h)
                md5s[str(n)] = hashlib.md5(raw[len(raw) - (3 if ext == "ppm" else 1) * w * h:]).hexdigest()
            if limit:
                assert not md5s, (name, m)
                recs[str(m)] = limit
                continue
            # conditions the tests rely on
            for n in LEVELS:
                assert n == 0 or md5s[str(n)] != md5s["0"], "%s: -s %d changes nothing at -m %d; take another case" % (name, n, m)
            assert md5s["-1"] == md5s[str(smooth)], (name, m)
            if smooth != 70:
                assert md5s["-1"] != md5s["70"], (name, m)
            recs[str(m)] = {"width": size[0], "height": size[1], "md5": md5s}
        assert "md5" in recs["0"], name
        out[name] = {"input": inp, "args": args, "smoothing": smooth, "stream_md5": hashlib.md5(stream).hexdigest(),
                     "width": recs["0"]["width"], "height": recs["0"]["height"], "color": ext == "ppm", "shown": recs, "tools": TOOLS}
        print("%-13s %s" % (name, " ".join("%d:%s" % (int(m), "%dx%d:%s" % (r["width"], r["height"], r["md5"]["-1"][:6]) if "md5" in r
                                                       else "%s %d" % (r["refused"][:3], r["limit"])) for m, r in recs.items())))
    with open(os.path.join(HERE, "DECODED_SHOWN.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_decoded_shown.py", "cases": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
