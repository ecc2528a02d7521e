#!/usr/bin/env python3
"""Decoded frames of the REAL reference over the option space: for every single-frame case of MANIFEST.json's
"option_cases", "model_cases" and "z3_cases", the pred_* stills and a few option stills of "cases" / "video_cases"
(tests/decoder_cases.py lists them; the two 1280 x 720 gray cases are left out), the reference's coder writes its
stream (md5 asserted against the manifest), `dfiasco_ref -s 0 -o` decodes it, and width, height, bands and the md5 of
the pixel bytes go into tests/golden/DECODED_OPTIONS.json.  Three synthetic edge inputs the manifest lacks -- a flat
gray frame, a flat colour frame, a colour frame with textured Y and constant chroma (decoder_cases.SYNTH_INPUTS) --
are recorded with the default options and with --prediction, stream md5 included.

The CPU check (tests/test_decoder_pins.py) recovers Y of a colour frame from the clipped byte decode_plane() returns,
as make_decoded_rgb.py explains; "y_clipped" says that the oracle's decoded Y band holds a byte 0 or 255, and that
check then leaves the case to the device test (tests/test_gpu_decoder_options.py), which compares RGB bytes in full.
MANIFEST.json is read, not rewritten.  Build container only (oracle/_ref from oracle/ref_build.sh)."""
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
import make_options  # noqa: E402,F401  (adds c01 / c02 to make_golden.INPUTS)
import fiasco_amd  # noqa: E402
import decoder_cases  # noqa: E402
from conftest import GOLDEN, ORACLE_LIB, REF_SHARE  # noqa: E402

REFDIR = os.path.join(ROOT, "oracle", "_ref")
TMP = "/tmp/fiasco_golden_decoded_options"
TOOLS = ("cfiasco_ref[_<model variant> | _z3] <args> -o ref.fco in.pnm; dfiasco_ref -s 0 -o dec.pnm ref.fco; "
         "decoded_md5 = md5 of dec.pnm's pixel bytes")
# the reference binary that wrote a list's streams (make_models.py, make_z3.py)
MODEL_VARIANT = {tuple(v): k for k, v in
                 {"adaptive": ("adaptive", "adaptive", "adaptive", "adaptive"), "uniform": ("uniform", "uniform", "uniform", "uniform"),
                  "basis": ("basis", "rle", "adaptive", "uniform"), "nochroma": ("rle-no-chroma", "rle", "adaptive", "adaptive"),
                  "rleuni": ("rle", "adaptive", "uniform", "adaptive")}.items()}


def coder_of(key, case):
    if key == "model_cases":
        return "cfiasco_ref_" + MODEL_VARIANT[tuple(case["models"])]
    return "cfiasco_ref_z3" if key == "z3_cases" else "cfiasco_ref"


def record(oracle, env, name, exe, data, args, models, want_md5):
    ext = "ppm" if data[:2] == b"P6" else "pgm"
    src, fco, dec = (os.path.join(TMP, name + e) for e in ("." + ext, ".fco", ".dec.pnm"))
    open(src, "wb").write(data)
    r = subprocess.run([os.path.join(REFDIR, exe), "--progress-meter", "0"] + args + ["-o", fco, src], env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    assert r.returncode == 0, "%s: the reference's coder does not finish: %s" % (name, r.stderr.decode("latin-1").strip().split("\n")[-1])
    stream = open(fco, "rb").read()
    md5 = hashlib.md5(stream).hexdigest()
    assert want_md5 is None or md5 == want_md5, name
    subprocess.check_call([os.path.join(REFDIR, "dfiasco_ref"), "-s", "0", "-o", dec, fco], env=env, stderr=subprocess.DEVNULL)
    raw = open(dec, "rb").read()
    w, h = [int(v) for v in raw.split(b"\n", 2)[1].split()]
    bands = 3 if raw[:2] == b"P6" else 1
    assert raw[:2] == (b"P6" if ext == "ppm" else b"P5") and (w, h, bands) == fiasco_amd._pnm_geometry(data), name
    rec = {"width": w, "height": h, "bands": bands, "decoded_md5": hashlib.md5(raw[len(raw) - bands * w * h:]).hexdigest()}
    if bands == 3:
        # the oracle writes the reference's stream; does its decoded Y band hold a clipped byte?
        b, o = decoder_cases.staged(oracle, data, args, models)
        assert hashlib.md5(b.encode()[0]).hexdigest() == md5, name
        yband = b.decode_plane(0, 0, w, h)
        b.free(); o.delete()
        rec["y_clipped"] = 0 in yband or 255 in yband
    return rec, md5


def main():
    os.makedirs(TMP, exist_ok=True)
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    oracle = fiasco_amd.Library(ORACLE_LIB)
    oracle.set_verbosity(0)
    out = {}
    for c, key in decoder_cases.manifest_cases(man):
        data, _ = make_golden.make_input(c["inputs"][0])
        assert c["name"] not in out
        out[c["name"]], _ = record(oracle, env, c["name"], coder_of(key, c), data, c["args"], c.get("models"), c["md5"])
        print("%-26s %s" % (c["name"], out[c["name"]]))
    for name, inp, args in decoder_cases.SYNTH_CASES:
        data = decoder_cases.SYNTH_INPUTS[inp]()
        rec, md5 = record(oracle, env, name, "cfiasco_ref", data, args, None, None)
        rec.update({"input": inp, "input_md5": hashlib.md5(data).hexdigest(), "args": args, "stream_md5": md5})
        out[name] = rec
        print("%-26s %s" % (name, rec))
    with open(os.path.join(HERE, "DECODED_OPTIONS.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_decoded_options.py", "tools": TOOLS, "cases": out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
