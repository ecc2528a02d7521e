#!/usr/bin/env python3
"""Magnified decoded frames of the REAL reference: for the stills below `cfiasco_ref <args>' codes the input and
`dfiasco_ref -s 0 -m M -o' decodes the stream for M in -3 .. 3 (enlarge_image, codec/decoder.c:776-840: thumbnails for
M < 0, enlargements for M > 0).  Per M tests/golden/DECODED_MAGNIFIED.json records the width, the height and the md5 of
the pixel bytes, or that the reference refused and the smallest / largest value its message names
(codec/dfiasco.c:104-137).  fiasco_amd_magnified_size() must give the same sizes and limits
(tests/test_magnify_api.py) and the device decoder the same bytes (tests/test_gpu_magnify.py).
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
import magnify_ref  # noqa: E402
from conftest import GOLDEN, REF_SHARE  # noqa: E402

# (name, input, MANIFEST case whose arguments are used)
# g64x32: no reduction allowed, enlarged up to 512 x 256; g100x70: ragged, 35 rows round to 36; g130x66: both sides round
# (65 -> 66, 33 -> 34); c256: colour, 256 x 192, -2 .. 3; c100x70: colour and ragged; c192x144: colour, -2 allowed, -3 not;
# c256sq: colour, 256 x 256, the one case that reaches -3; g64x64_a / _b: two small frames that differ, for the flights
CASES = [
    ("g64x32", "g64x32", "g64x32_q20"),
    ("g100x70", "g100x70", "g100x70_q20"),
    ("g130x66", "synth:130:66:19", "g100x70_q20"),
    ("c256", "c256", "c256_q20"),
    ("c100x70", "synthrgb:100:70:41:42:43", "c256_q20"),
    ("c192x144", "synthrgb:192:144:44:45:46", "c256_q20"),
    ("c256sq", "synthrgb:256:256:47:48:49", "c256_q20"),
    ("g64x64_a", "synth:64:64:17", "g64x32_q20"),
    ("g64x64_b", "synth:64:64:18", "g64x32_q20"),
]
REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_magnified"
TOOLS = ("cfiasco_ref <args> -o ref.fco in; dfiasco_ref -s 0 -m M -o dec ref.fco; magnified[M] = width, height and md5 of dec's "
         "pixel bytes, or refused + the limit the message names")


def main():
    os.makedirs(TMP, exist_ok=True)
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    cases = {c["name"]: c for c in man["cases"]}
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    out = {}
    for name, inp, of in CASES:
        args = cases[of]["args"]
        data, ext = magnify_ref.synth_input(inp) or make_golden.make_input(inp)
        src = os.path.join(TMP, name + "." + ext)
        open(src, "wb").write(data)
        fco = os.path.join(TMP, name + ".fco")
        subprocess.check_call([os.path.join(REFDIR, "cfiasco_ref"), "--progress-meter", "0"] + args + ["-o", fco, src],
                              env=env, stderr=subprocess.DEVNULL)
        stream = open(fco, "rb").read()
        recs = {}
        for m in magnify_ref.MAGS:
            dec = os.path.join(TMP, "%s.m%d.%s" % (name, m, ext))
            if os.path.exists(dec):
                os.remove(dec)
            r = subprocess.run([os.path.join(REFDIR, "dfiasco_ref"), "-s", "0", "-m", str(m), "-o", dec, fco], env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
            said = r.stdout.decode("latin-1")
            lim = re.search(r"(Minimum|Maximium) value is (-?\d+)", said)
            if lim:
                assert not os.path.exists(dec), (name, m)
                recs[str(m)] = {"refused": "minimum" if lim.group(1) == "Minimum" else "maximum", "limit": int(lim.group(2))}
                continue
            assert r.returncode == 0, (name, m, said)
            raw = open(dec, "rb").read()
            assert raw[:2] == (b"P6" if ext == "ppm" else b"P5"), name
            w, h = [int(v) for v in raw.split(b"\n", 2)[1].split()]
            recs[str(m)] = {"width": w, "height": h, "md5": hashlib.md5(raw[len(raw) - (3 if ext == "ppm" else 1) * w * h:]).hexdigest()}
        # conditions the tests rely on
        assert "md5" in recs["0"], name
        for m in magnify_ref.MAGS:
            assert m == 0 or "md5" not in recs[str(m)] or recs[str(m)]["md5"] != recs["0"]["md5"], "%s: -m %d changes nothing" % (name, m)
        assert "md5" in recs["3"] or any("refused" in r for r in recs.values()), name
        out[name] = {"input": inp, "args": args, "stream_md5": hashlib.md5(stream).hexdigest(), "width": recs["0"]["width"],
                     "height": recs["0"]["height"], "color": ext == "ppm", "magnified": recs, "tools": TOOLS}
        print("%-10s %s" % (name, " ".join("%d:%s" % (m, "%dx%d:%s" % (recs[str(m)]["width"], recs[str(m)]["height"], recs[str(m)]["md5"][:6])
                                                       if "md5" in recs[str(m)] else "%s %d" % (recs[str(m)]["refused"][:3], recs[str(m)]["limit"]))
                                        for m in magnify_ref.MAGS)))
    with open(os.path.join(HERE, "DECODED_MAGNIFIED.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_decoded_magnified.py", "cases": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
