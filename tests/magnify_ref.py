"""What the magnification tests share (tests/test_magnify_api.py, tests/test_gpu_magnify.py, the generator
tests/golden/make_decoded_magnified.py): the fixture tests/golden/DECODED_MAGNIFIED.json and the inputs of its cases."""
import json
import os

import numpy as np

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MAGS = list(range(-3, 4))


def fixture_cases():
    return json.load(open(os.path.join(GOLDEN, "DECODED_MAGNIFIED.json")))["cases"]


def synth_input(spec):
    """synth:W:H:SEED -> a PGM of synth.synth(W, H, SEED); synthrgb:W:H:R:G:B -> a PPM whose planes are
    synth.synth(W, H, R), (W, H, G), (W, H, B).  (bytes, extension), or None for any other name"""
    part = spec.split(":")
    if part[0] == "synth":
        w, h, seed = (int(v) for v in part[1:])
        return synth.pgm_bytes(synth.synth(w, h, seed)), "pgm"
    if part[0] == "synthrgb":
        w, h = int(part[1]), int(part[2])
        return synth.ppm_bytes(np.stack([synth.synth(w, h, int(s)) for s in part[3:6]], -1)), "ppm"
    return None


def case_input(inputs, ent):
    """the PNM bytes of a fixture case: synthesised, or a golden input by name"""
    made = synth_input(ent["input"])
    return made[0] if made else inputs.data(ent["input"])


def accepted(ent):
    """[(M, record)] of the magnifications the reference decodes the case at"""
    return [(m, ent["magnified"][str(m)]) for m in MAGS if "md5" in ent["magnified"][str(m)]]


def refused(ent):
    return [(m, ent["magnified"][str(m)]) for m in MAGS if "md5" not in ent["magnified"][str(m)]]
