"""The border list of the reference's smoothing (fiasco_amd_batch_smoothing_borders) and the unsmoothed planes
(fiasco_amd_batch_decode_planes) of frames the DEVICE coded and decoded: the list is built from the coordinates the
device coder leaves in its automata, which no stream carries, so the CPU pin (tests/test_smoothing_api.py, oracle
library) does not cover them.  Applied sequentially by the numpy restatement (tests/smooth_ref.py) they must give the
bytes `dfiasco_ref -s N' wrote (tests/golden/DECODED_SMOOTH.json)."""
import hashlib
import json
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch  # noqa: F401                      # before the product library: one HIP runtime for both

import fiasco_amd
import smooth_ref
from conftest import GOLDEN, options_from_args
from pixels_ref import pixels_of_planes

pytestmark = pytest.mark.gpu


def test_device_coded_frames_give_the_references_smoothed_bytes(product, oracle, inputs):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    cases = json.load(open(os.path.join(GOLDEN, "DECODED_SMOOTH.json")))["cases"]
    for name, ent in cases.items():
        got = []
        for lib in (product, oracle):
            q, o = options_from_args(lib, ent["args"])
            o.set_smoothing(ent["smoothing"])
            b = fiasco_amd.Batch(lib, [smooth_ref.case_input(inputs, ent)], q, o)
            stream = b.encode()[0]
            assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], (name, lib.error_message())
            got.append((b.decode_planes(0), b.smoothing_borders(0)))
            if lib is product:
                w, h, bands = b._geom[0]
                for k in range(bands):              # the planes are what decode_plane turns into bytes
                    want = np.frombuffer(b.decode_plane(0, k, w, h), dtype=np.uint8).reshape(h, w)
                    assert np.array_equal(np.clip((got[0][0][k].astype(np.int32) >> 4) + 128, 0, 255), want), (name, k)
            b.free(); o.delete()
        (planes, borders), (oplanes, oborders) = got
        assert borders == oborders and np.array_equal(planes, oplanes), name
        for n in (0, 1, 35, 70, 100):
            out = smooth_ref.smooth_planes(planes, borders, n)
            md5 = hashlib.md5(pixels_of_planes(out[0] if out.shape[0] == 1 else out).tobytes()).hexdigest()
            assert md5 == ent["decoded_md5"][str(n)], (name, n)
