#!/usr/bin/env python3
"""Decoded colour frames of the REAL reference: for the colour still cases below, `dfiasco_ref -s 0 -o` decodes the
reference's own stream and writes a PPM; the md5 of its pixel bytes goes into tests/golden/DECODED_RGB.json.
fiasco_amd_batch_decode_device() must write the same bytes into device memory (tests/test_gpu_device_output.py), and
the numpy restatement of write_image (tests/pixels_ref.py) must give them from the oracle's decoded bands
(tests/test_device_output_api.py).  That second check recovers Y from the byte decode_plane() returns, so every
recorded case must have a decoded Y band without a byte 0 or 255 (the per-band clip then lost nothing): asserted
here.  MANIFEST.json is read, not rewritten.  Build container only (oracle/_ref from oracle/ref_build.sh)."""
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
import fiasco_amd  # noqa: E402
from conftest import GOLDEN, ORACLE_LIB, REF_SHARE, options_from_args  # noqa: E402

# The first choice was c00_q20, c00_z1, c256_q20, c256_z2, c256_chroma, check64_q20.  check64_q20 is a gray checker
# board of 0 and 255 (a PGM, and its decoded band is full of clipped bytes: it fails the assertion below): replaced
# by c256_z1, the remaining small colour still of MANIFEST.json.
CASES = ["c00_q20", "c00_z1", "c256_q20", "c256_z2", "c256_chroma", "c256_z1"]
REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_rgb"
TOOLS = "cfiasco_ref <args> -o ref.fco in.ppm; dfiasco_ref -s 0 -o dec.ppm ref.fco; decoded_md5 = md5 of dec.ppm's pixel bytes"


def main():
    os.makedirs(TMP, exist_ok=True)
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    cases = {c["name"]: c for c in man["cases"]}
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    oracle = fiasco_amd.Library(ORACLE_LIB)
    oracle.set_verbosity(0)
    out = {}
    for name in CASES:
        c = cases[name]
        assert len(c["inputs"]) == 1
        data, ext = make_golden.make_input(c["inputs"][0])
        assert ext == "ppm", name
        src = os.path.join(TMP, name + "." + ext)
        open(src, "wb").write(data)
        fco = os.path.join(TMP, name + ".fco")
        subprocess.check_call([os.path.join(REFDIR, "cfiasco_ref"), "--progress-meter", "0"] + c["args"] + ["-o", fco, src],
                              env=env, stderr=subprocess.DEVNULL)
        assert hashlib.md5(open(fco, "rb").read()).hexdigest() == c["md5"], name
        dec = os.path.join(TMP, name + ".dec.ppm")
        subprocess.check_call([os.path.join(REFDIR, "dfiasco_ref"), "-s", "0", "-o", dec, fco], env=env, stderr=subprocess.DEVNULL)
        raw = open(dec, "rb").read()
        assert raw[:2] == b"P6", name
        w, h = [int(v) for v in raw.split(b"\n", 2)[1].split()]
        # the oracle's decoded Y band holds no clipped byte
        q, o = options_from_args(oracle, c["args"])
        b = fiasco_amd.Batch(oracle, [data], q, o)
        assert hashlib.md5(b.encode()[0]).hexdigest() == c["md5"], name
        yband = b.decode_plane(0, 0, w, h)
        b.free(); o.delete()
        assert 0 not in yband and 255 not in yband, "%s: the decoded Y band is clipped; take another case" % name
        out[name] = {"width": w, "height": h, "decoded_md5": hashlib.md5(raw[len(raw) - 3 * w * h:]).hexdigest(), "tools": TOOLS}
        print("%-14s %d x %d %s" % (name, w, h, out[name]["decoded_md5"]))
    with open(os.path.join(HERE, "DECODED_RGB.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_decoded_rgb.py", "cases": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
