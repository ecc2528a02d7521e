"""What tests/golden/make_reconst_pixels.py, tests/test_seq_device_api.py (CPU) and tests/test_gpu_seq_device.py (device)
share: the cases of tests/golden/RECONST_PIXELS.json -- the pinned videos of tests/reconst_cases.py and the two all-intra
colour sequences whose minimum level ratchets from frame to frame -- their inputs as arrays, and the numpy form of the
PNM reader's pixel conversion.  No codec logic here: inputs, selection, file handling.

The fixture holds, per case and display frame, what a video's device outputs must deliver (fiasco_amd_seq_set_outputs_device):
the md5 of the 8-bit pixels of the REFERENCE CODER's reconstructed planes (pixels_ref.pixels_of_planes: gray H x W, colour
H x W x 3 interleaved), and per band the exact sum of squared differences and the largest absolute difference between
those planes and the frame's original planes (distortion_ref.distortion_of_planes).  Nothing in it comes from the code
under test.
"""
import hashlib
import json
import os

import numpy as np

import reconst_cases as rc
from conftest import GOLDEN, options_from_args

FIXTURE = os.path.join(GOLDEN, "RECONST_PIXELS.json")
CARRY = ["seq3_color_carry48", "seq3_color_carry74"]      # all-intra, three groups of pictures each (MANIFEST.json "cases")


def names(manifest):
    return rc.pinned_names(manifest) + CARRY


def case_of(manifest, inputs, name):
    """-> (frames as PNM bytes, cfiasco arguments, md5 of the reference's stream)"""
    if name in CARRY:
        case = [c for c in manifest["cases"] if c["name"] == name][0]
        return [inputs.data(i) for i in case["inputs"]], list(case["args"]), case["md5"]
    frames, args = rc.case_of(manifest, inputs, name)
    return frames, args, rc.fixture()[name]["stream_md5"]


def fixture():
    return json.load(open(FIXTURE))["cases"]


def array_of_pnm(frame):
    """raw PGM / PPM bytes -> uint8 H x W or H x W x 3"""
    w, h, nb = rc.geometry([frame])
    a = np.frombuffer(frame[len(frame) - w * h * nb:], np.uint8)
    return a.reshape((h, w, 3) if nb == 3 else (h, w))


def original_planes(a):
    """the PNM reader's planes of an 8-bit frame (host/fa_image.c convert_planes, reference lib/image.c:365-389): int16
    [bands, H, W].  The colour form is pinned to convert_planes for all 2^24 triples by tests/test_device_input_api.py"""
    if a.ndim == 2:
        return ((a.astype(np.int16) - 128) * 16)[None]
    r, g, b = (a[..., k].astype(np.float64) for k in range(3))
    y = ((+0.2989 * r + 0.5866 * g + 0.1145 * b - 128) * 16).astype(np.int32).astype(np.int16)
    cb = ((-0.1687 * r - 0.3312 * g + 0.5000 * b) * 16).astype(np.int32).astype(np.int16)
    cr = ((+0.5000 * r - 0.4183 * g - 0.0816 * b) * 16).astype(np.int32).astype(np.int16)
    return np.stack([y, cb, cr])


def pixels_md5(pixels):
    return hashlib.md5(np.ascontiguousarray(pixels, np.uint8).tobytes()).hexdigest()


def record_of_planes(frame, planes):
    """what the fixture holds for one display frame: from its PNM bytes and reconstructed planes [bands, H, W]"""
    from distortion_ref import distortion_of_planes
    from pixels_ref import pixels_of_planes
    sse, mx = distortion_of_planes(original_planes(array_of_pnm(frame)), planes)
    return {"pixels_md5": pixels_md5(pixels_of_planes(planes if planes.shape[0] == 3 else planes[0])), "sse": sse, "maxdiff": mx}


def open_options(lib, args):
    return options_from_args(lib, args)
