"""The reference's border smoothing restated in numpy (smooth_image, reference codec/decoder.c:674-768).
tests/test_smoothing_api.py pins it, and the border list it is fed (fiasco_amd_batch_smoothing_borders), to the bytes
`dfiasco_ref -s N' writes (tests/golden/DECODED_SMOOTH.json) without a GPU.

The borders are applied SEQUENTIALLY in list order and in place, as the reference's loop over the states does: borders
that cross share pixels, so the order is part of the result."""
import numpy as np


def factors(sf):
    """(is, inegs) of a smoothing percentage with the reference's types: real_t is float, the products are float, the
    additions of .5 double, the conversions to int truncate.  None: the reference smooths nothing."""
    s = np.float32(1.0 - sf / 200.0)
    if s < 0.5 or s >= 1:
        return None
    i_s = int(np.float64(s * np.float32(512)) + .5)
    inegs = int(np.float64((np.float32(1) - s) * np.float32(512)) + .5)
    return i_s, inegs


def blend(a, b, i_s, inegs):
    """the pair update on int64 arrays of int16 values: arithmetic shifts, the result stored as int16"""
    one = (((i_s * a) >> 10) << 1) + (((inegs * b) >> 10) << 1)
    two = (((i_s * b) >> 10) << 1) + (((inegs * a) >> 10) << 1)
    return one.astype(np.int16), two.astype(np.int16)


def smooth(y_plane, borders, sf):
    """y_plane: int16 [H, W]; borders: (x, y, len, level, pass) tuples -> a smoothed copy"""
    p = np.array(y_plane, dtype=np.int16)
    assert p.ndim == 2
    f = factors(sf)
    if f is None:
        return p
    for x, y, n, level, _ in borders:
        if level & 1:                       # horizontal: rows y - 1 and y
            one, two = p[y - 1, x:x + n], p[y, x:x + n]
        else:                               # vertical: columns x - 1 and x
            one, two = p[y:y + n, x - 1], p[y:y + n, x]
        assert y >= (level & 1) and x >= 1 - (level & 1) and one.shape == (n,) and two.shape == (n,), (x, y, n, level)
        a, b = one.astype(np.int64), two.astype(np.int64)
        one[:], two[:] = blend(a, b, *f)
    return p


def smooth_planes(planes, borders, sf):
    """int16 [bands, H, W]: band 0 smoothed, the others as they are"""
    out = np.array(planes, dtype=np.int16)
    out[0] = smooth(out[0], borders, sf)
    return out


def case_input(inputs, ent):
    """the PNM bytes of a case of tests/golden/DECODED_SMOOTH.json: a golden input by name, or synth:W:H:SEED"""
    if ent["input"].startswith("synth:"):
        import synth
        w, h, seed = (int(v) for v in ent["input"].split(":")[1:])
        return synth.pgm_bytes(synth.synth(w, h, seed))
    return inputs.data(ent["input"])
