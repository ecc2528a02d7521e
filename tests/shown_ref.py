"""What the tests of the shown frames share (tests/test_shown_api.py, tests/test_gpu_shown.py, the generator
tests/golden/make_decoded_shown.py): the fixture tests/golden/DECODED_SHOWN.json, the inputs of its cases, and the border
list of a magnified frame derived in numpy from the CODED list -- `dfiasco -m M' smooths along the coded borders with x
and y shifted by M, the level raised by 2 M and the length the side of that level, clipped at the size shown
(enlarge_image + smooth_image, reference codec/decoder.c:776-840, :674-768)."""
import json
import os

import numpy as np

import magnify_ref
import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEVELS = (-1, 35, 70)
# (case, M) the reference decodes but the library refuses to smooth: a smoothed state falls below level 1 there
LIBRARY_REFUSES = {("g256_z1_q300", -3)}


def fixture_cases():
    return json.load(open(os.path.join(GOLDEN, "DECODED_SHOWN.json")))["cases"]


def synth_input(spec):
    """noise:W:H:SEED -> a PGM of synth.noise(W, H, SEED); else magnify_ref.synth_input"""
    part = spec.split(":")
    if part[0] == "noise":
        w, h, seed = (int(v) for v in part[1:])
        return synth.pgm_bytes(synth.noise(w, h, seed)), "pgm"
    return magnify_ref.synth_input(spec)


def case_input(inputs, ent):
    made = synth_input(ent["input"])
    return made[0] if made else inputs.data(ent["input"])


def staged(lib, inputs, ent):
    """a fixture case as a batch of one frame, not yet encoded -> (batch, options)"""
    import fiasco_amd
    from conftest import options_from_args
    q, o = options_from_args(lib, ent["args"])
    o.set_smoothing(ent["smoothing"])
    return fiasco_amd.Batch(lib, [case_input(inputs, ent)], q, o), o


def accepted(ent):
    """[(M, record)] of the magnifications the reference decodes the case at"""
    return [(int(m), r) for m, r in sorted(ent["shown"].items(), key=lambda kv: int(kv[0])) if "md5" in r]


def refused(ent):
    return [(int(m), r) for m, r in sorted(ent["shown"].items(), key=lambda kv: int(kv[0])) if "md5" not in r]


def side(level):
    """the unclipped length of a border of `level': the width of the level for a horizontal one, the height else"""
    return 1 << (level >> 1) if level & 1 else 1 << ((level + 1) >> 1)


def magnified_borders(coded, m, width, height):
    """the list at magnification m from the coded list [(x, y, len, level, pass)]; width x height: the size shown.
    None: a border falls below level 1.  Passes that lose all their borders close up."""
    out, renumber = [], {}
    for x, y, _, level, p in coded:
        x, y = (x << m, y << m) if m >= 0 else (x >> -m, y >> -m)
        level += 2 * m
        if x >= width or y >= height:
            continue
        if level < 1:
            return None
        room = width - x if level & 1 else height - y
        out.append((x, y, min(side(level), room), level, renumber.setdefault(p, len(renumber))))
    return out


def pixels_touched(borders, width, height):
    """per pass: a boolean plane of the pixels its borders touch, asserting that no two borders of the pass share one"""
    planes = {}
    for x, y, n, level, p in borders:
        seen = planes.setdefault(p, np.zeros((height, width), dtype=bool))
        region = seen[y - 1:y + 1, x:x + n] if level & 1 else seen[y:y + n, x - 1:x + 1]
        assert region.shape == ((2, n) if level & 1 else (n, 2)) and not region.any(), (p, x, y, n, level)
        region[:] = True
    return planes
