#!/usr/bin/env python3
"""Known answers for the device outputs of a video: tests/golden/RECONST_PIXELS.json, from the reference binaries alone.

For every case of tests/seq_device_cases.py -- the pinned videos of tests/reconst_cases.py and the all-intra colour
sequences seq3_color_carry48 / seq3_color_carry74 -- cfiasco_ref_recon (oracle/ref_build.sh) codes the frames and writes
the planes it reconstructed, intra frames included.  Per display frame the fixture records
  * pixels_md5: the md5 of pixels_ref.pixels_of_planes of those planes (gray H x W, colour H x W x 3 interleaved),
  * sse, maxdiff per band: distortion_ref.distortion_of_planes(original planes, those planes); the original planes are
    the PNM reader's, in the numpy form tests/test_device_input_api.py pins for all 2^24 triples.
Checked on the way: the planes of the pinned videos have the md5 of RECONST.json, every stream the md5 the fixtures hold
for it.  The frames of the all-intra pair are decoded I frames: `dfiasco_ref -s 0' must show the very pixels recorded
(it never differs on an I frame); a stream of MANIFEST.json that DECODED_RGB.json also holds is cross-checked there.
Results only, no program text.  Build container only (oracle/_ref)."""
import hashlib
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import conftest  # noqa: E402
import reconst_cases as rc  # noqa: E402
import seq_device_cases as sd  # noqa: E402
from pixels_ref import pixels_of_planes  # noqa: E402


def main():
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    pinned = rc.fixture()
    decoded_rgb = json.load(open(os.path.join(HERE, "DECODED_RGB.json")))["cases"]
    td = tempfile.mkdtemp(prefix="fiasco_reconst_pixels_")
    inputs = conftest.Inputs(man, td)
    cases = {}
    for name in sd.names(man):
        frames, args, stream_md5 = sd.case_of(man, inputs, name)
        geom = rc.geometry(frames)
        err, stream, planes = rc.run_reference(rc.CFIASCO_RECON, frames, args, os.path.join(td, name))
        if err:
            sys.exit("%s: the reference does not code this case (%s)" % (name, err))
        assert hashlib.md5(stream).hexdigest() == stream_md5, name
        assert sorted(planes) == list(range(len(frames))), (name, sorted(planes))
        if name in pinned:
            for f in pinned[name]["frames"]:
                assert rc.planes_md5(planes[f["display"]][1]) == f["planes_md5"] and planes[f["display"]][0] == f["type"], (name, f)
        else:
            dec = rc.reference_decode(stream, len(frames), geom, os.path.join(td, name))
            assert dec is not None, "%s: dfiasco_ref dies" % name
            for d, (t, p) in planes.items():
                assert t == 0 and (pixels_of_planes(p if geom[2] == 3 else p[0]) == dec[d]).all(), (name, d)
        if name in decoded_rgb:
            assert sd.pixels_md5(pixels_of_planes(planes[0][1])) == decoded_rgb[name]["decoded_md5"], name
        ent = {"geometry": list(geom), "stream_md5": stream_md5, "frames": []}
        for d in sorted(planes):
            t, p = planes[d]
            ent["frames"].append(dict({"display": d, "type": t}, **sd.record_of_planes(frames[d], p)))
        cases[name] = ent
        print("%-26s %s" % (name, " ".join("%d%s:%d" % (f["display"], "IPB"[f["type"]], f["sse"][0]) for f in ent["frames"])))
    with open(sd.FIXTURE, "w") as f:
        json.dump({"generator": "tests/golden/make_reconst_pixels.py", "reference": "oracle/_ref/cfiasco_ref_recon (oracle/ref_build.sh)",
                   "cases": cases}, f, indent=1)
        f.write("\n")
    shutil.rmtree(td)


if __name__ == "__main__":
    main()
