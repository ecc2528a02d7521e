#!/usr/bin/env python3
"""Known answers for fiasco_c_options_set_video_param and the coding orders of B frames: tests/golden/VIDEO_PARAM.json,
from the reference alone.  Build container only (oracle/_ref from oracle/ref_build.sh).

The reference's command-line tool never calls the setter, so oracle/_ref/libfiasco_ref_recon.so is driven through ctypes
(tests/video_param_cases.py run_reference_library: the option calls in the order of bin/cwfa.c:252-393, then
set_video_param, then fiasco_coder; one child process per run, any status but 0 means "no stream").  For every case of
tests/video_param_cases.py this script
  * asserts that the driver with (25, 1, 1), and with no set_video_param call at all, writes the stream of
    `cfiasco_ref_recon <args>` on the same files: the driver is the command-line tool's mapping;
  * asserts that writing the frames out does not change the stream;
  * records the md5 and length of the stream and, per frame, the display number, the type and the md5 of the planes;
  * records the numbers of forward, backward and interpolated blocks that restore_mc applies to each frame ("blocks").
    The reference does not print them: they are read from the CPU oracle's run AFTER its stream has been found equal to
    the reference's, so they are counts of the reference's own automaton;
  * runs the twin (the other B_as_past_ref value) and records whether its stream differs and which frames' planes do;
  * for the refused patterns records how the reference ends.
No pixels are kept."""
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
import fiasco_amd  # noqa: E402
import reconst_cases as rc  # noqa: E402
import video_param_cases as vc  # noqa: E402


def main():
    td = tempfile.mkdtemp(prefix="fiasco_video_param_")
    ora = fiasco_amd.Library(conftest.ORACLE_LIB)
    ora.set_verbosity(0)
    cases, refusals, cli = {}, {}, {}
    for name in vc.NAMES:
        frames, args, vp = vc.case_of(name)
        tmp = os.path.join(td, name)
        key = (rc.inputs_md5(frames), tuple(args))
        if key not in cli:           # the tie to the command-line tool, once per (inputs, arguments)
            e0, s0, _ = rc.run_reference(rc.CFIASCO_RECON, frames, args, os.path.join(tmp, "cli"), dump=False)
            e1, s1, _ = vc.run_reference_library(frames, args, (25, 1, 1), os.path.join(tmp, "as_cli"), dump=False)
            e2, s2, _ = vc.run_reference_library(frames, args, None, os.path.join(tmp, "no_call"), dump=False)
            if e0 or e1 or e2 or s0 != s1 or s0 != s2:
                sys.exit("%s: the driven library does not write the command-line tool's stream (%s / %s / %s)" % (name, e0, e1, e2))
            cli[key] = hashlib.md5(s0).hexdigest()
        err, stream, planes = vc.run_reference_library(frames, args, vp, os.path.join(tmp, "recon"))
        if err:
            sys.exit("%s: the reference does not code this case (%s): it cannot be pinned" % (name, err))
        eq, quiet, _ = vc.run_reference_library(frames, args, vp, os.path.join(tmp, "quiet"), dump=False)
        assert eq is None and quiet == stream, "%s: writing the frames out changes the stream" % name
        assert sorted(planes) == list(range(len(frames))), (name, sorted(planes))
        ostream, oplanes, counts, msg = vc.run_library(ora, frames, args, vp, os.path.join(tmp, "oracle"))
        if ostream != stream:
            sys.exit("%s: the oracle's stream is not the reference's (%s): no block counts to record" % (name, msg))
        terr, tstream, tplanes = vc.run_reference_library(frames, args, vc.twin_of(vp), os.path.join(tmp, "twin"))
        assert terr is None, (name, terr)
        ent = {"args": args, "video_param": list(vp), "inputs_md5": rc.inputs_md5(frames), "geometry": list(rc.geometry(frames)),
               "cli_stream_md5": cli[key], "stream_md5": hashlib.md5(stream).hexdigest(), "bytes": len(stream), "frames": [],
               "twin": {"stream_differs": tstream != stream, "bytes": len(tstream),
                        "planes_differ": [d for d in sorted(planes) if not np.array_equal(planes[d][1], tplanes[d][1])]}}
        for display in sorted(planes):
            t, p = planes[display]
            assert tplanes[display][0] == t, (name, display)
            c = counts[display]
            ent["frames"].append({"display": display, "type": t, "planes_md5": rc.planes_md5(p),
                                  "blocks": [c["forward"], c["backward"], c["interpolated"]]})
        cases[name] = ent
        print("%-34s %6d B %s  %s  twin: stream %s, frames %s" % (name, len(stream), ent["stream_md5"], " ".join(
            "%d%s" % (f["display"], "IPB"[f["type"]]) for f in ent["frames"]), "differs" if ent["twin"]["stream_differs"] else "equal",
            ent["twin"]["planes_differ"]))
    for name in vc.REFUSED:
        frames, args, vp = vc.case_of(name)
        err, stream, _ = vc.run_reference_library(frames, args, vp, os.path.join(td, name))
        assert err is not None and stream is None, (name, "the reference codes a refused pattern")
        refusals[name] = {"args": args, "video_param": list(vp), "inputs_md5": rc.inputs_md5(frames), "reference": err.split(":")[0]}
        print("%-34s reference: %s" % (name, err))
    json.dump({"generator": "tests/golden/make_video_param.py", "reference": "oracle/_ref/libfiasco_ref_recon.so (oracle/ref_build.sh), driven through ctypes",
               "cases": cases, "refusals": refusals}, open(vc.FIXTURE, "w"), indent=1)
    shutil.rmtree(td)


if __name__ == "__main__":
    main()
