#!/usr/bin/env python3
"""Known answers for the reconstructed frames of a video: tests/golden/RECONST.json, from the reference binaries alone.

oracle/ref_build.sh builds cfiasco_ref_recon: the reference coder with one block added behind its restore_mc line that
writes reconst->pixels[] of every frame it has coded (the image the next P / B frame is predicted from).  For every
case of tests/reconst_cases.py this script
  * checks that the variant writes the STOCK coder's stream, with and without the variable that makes it write frames,
  * records per frame the display number, the type and the md5 of the plane bytes (int16, little endian, 1 or 3 bands),
    and the md5 of the stream,
  * records per frame whether `dfiasco_ref -s 0` gives pixels_ref.pixels_of_planes of those planes ("dfiasco_equal":
    true / false, null where dfiasco_ref dies) and, where not, how many bytes differ and by how much at most.  The
    reference's decoder is not the yardstick of these frames; the figures are the record of that.
"""
import hashlib
import json
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import conftest  # noqa: E402
import reconst_cases as rc  # noqa: E402
from pixels_ref import pixels_of_planes  # noqa: E402


def main():
    man = json.load(open(os.path.join(HERE, "MANIFEST.json")))
    td = tempfile.mkdtemp(prefix="fiasco_reconst_")
    inputs = conftest.Inputs(man, td)
    cases = {}
    for name in rc.pinned_names(man):
        frames, args = rc.case_of(man, inputs, name)
        geom = rc.geometry(frames)
        tmp = os.path.join(td, name)
        e0, s0, _ = rc.run_reference(rc.CFIASCO, frames, args, os.path.join(tmp, "stock"), dump=False)
        e1, s1, _ = rc.run_reference(rc.CFIASCO_RECON, frames, args, os.path.join(tmp, "quiet"), dump=False)
        err, stream, planes = rc.run_reference(rc.CFIASCO_RECON, frames, args, os.path.join(tmp, "recon"))
        if (e0, s0) != (e1, s1) or (e0, s0) != (err, stream):
            sys.exit("%s: cfiasco_ref_recon does not write what the stock reference writes (%s / %s / %s)" % (name, e0, e1, err))
        if err:
            sys.exit("%s: the reference does not code this case (%s): it cannot be pinned" % (name, err))
        if any(c["name"] == name for c in man["video_cases"]):
            case = [c for c in man["video_cases"] if c["name"] == name][0]
            assert hashlib.md5(stream).hexdigest() == case["md5"], name
        assert sorted(planes) == list(range(len(frames))), (name, sorted(planes))
        dec = rc.reference_decode(stream, len(frames), geom, tmp)
        ent = {"args": args, "inputs_md5": rc.inputs_md5(frames), "geometry": list(geom),
               "stream_md5": hashlib.md5(stream).hexdigest(), "bytes": len(stream), "frames": []}
        for display in sorted(planes):
            t, p = planes[display]
            fr = {"display": display, "type": t, "planes_md5": rc.planes_md5(p), "dfiasco_equal": None}
            if geom[2] == 3:
                fr["chroma_at_clip"] = [int((p[1:] == b).sum()) for b in rc.CHROMA_CLIP]
            if dec is not None:
                want = pixels_of_planes(p if geom[2] == 3 else p[0])
                d = np.abs(want.astype(np.int32) - dec[display].astype(np.int32))
                fr["dfiasco_equal"] = bool(d.max() == 0)
                if d.max():
                    fr["dfiasco_differs"] = {"bytes": int((d != 0).sum()), "largest": int(d.max())}
            ent["frames"].append(fr)
        cases[name] = ent
        print("%-26s %6d B %s  %s" % (name, len(stream), ent["stream_md5"], " ".join(
            "%d%s%s" % (f["display"], "IPB"[f["type"]], {True: "=", False: "!", None: "x"}[f["dfiasco_equal"]]) for f in ent["frames"])))
    json.dump({"generator": "tests/golden/make_reconst.py", "reference": "oracle/_ref/cfiasco_ref_recon (oracle/ref_build.sh)",
               "cases": cases}, open(rc.FIXTURE, "w"), indent=1)
    shutil.rmtree(td)


if __name__ == "__main__":
    main()
