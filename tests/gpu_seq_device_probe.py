#!/usr/bin/env python3
"""Developer probe (not part of the suite): what feeding a video from device memory saves and what its device outputs
cost.  BASELINE config 5 -- 300 frames of 1280 x 720 colour, pattern ippppppppp, --prediction (the generator of
tests/gpu_config5.py) -- through Sequence.encode() in ONE process, three ways:
  pnm      fiasco_amd_seq_open: PNM bytes in host memory, parsed by 16 host threads per step and uploaded
  device   fiasco_amd_seq_open_device: the frames as one uint8 tensor on the GPU (open, its conversion included, is timed too)
  outputs  device-fed, with a target for every frame and the distortion (every frame decoded: 30 more than the 270
           references of this pattern)
One warm-up of the PNM route first, then `--reps' rounds of the three, alternating; median, min and max are kept.
Per run: wall clock around open + encode + torch.cuda.synchronize(), the phases FIASCO_AMD_SEQ_TIMING prints (prepare /
core / decode of fa_seq_search, probe, writer), and decoder_frames / decoder_us of fiasco_amd_stats.  Every stream must
be the real reference's (md5 714a25c6...).
--ab LIB: afterwards tests/gpu_config5.py (fiasco_coder() on files, PNM-fed, a fresh process each) alternates between
this library and LIB, a build of the parent commit, `--reps' times each, the one that goes first changing from round
to round: the new library's time must lie inside the parent's own spread.  (--ab-only: that comparison alone.)  Writes profiles/seq_device.json."""
import argparse
import hashlib
import json
import multiprocessing as mp
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

os.environ.setdefault("FIASCO_AMD_DEBUG", "1")          # the timing lines are a developer switch
os.environ["FIASCO_AMD_SEQ_TIMING"] = "1"

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import fiasco_amd  # noqa: E402
import synth  # noqa: E402

W, H = 1280, 720
REFERENCE_MD5 = "714a25c639d8daae598f84095f4856f7"      # 300 frames, the real reference (68 min on one core)


def make_frame(f):
    return synth.synth_color_k(W, H, 1234, 3 * f)


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


class Stderr:
    """fd 2 into a file while the C side prints its timing lines"""
    def __enter__(self):
        self.tmp = tempfile.TemporaryFile()
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode("latin-1")
        self.tmp.close()


def phases(text):
    out = {"prepare": 0.0, "core": 0.0, "decode": 0.0, "probe": 0.0, "writer": 0.0, "searches": 0}
    for m in re.finditer(r"fa_seq_search: .*?prepare ([\d.]+) s, core ([\d.]+) s, decode ([\d.]+) s", text):
        out["prepare"] += float(m.group(1)); out["core"] += float(m.group(2)); out["decode"] += float(m.group(3))
        out["searches"] += 1
    for key, pat in (("probe", r"probe ([\d.]+) s"), ("writer", r"writer ([\d.]+) s")):
        for m in re.finditer(pat, text):
            out[key] += float(m.group(1))
    return out


def one(lib, route, pnms, dev, targets, o):
    lib.reset_stats()
    torch.cuda.synchronize()
    with Stderr() as err:
        t0 = time.perf_counter()
        if route == "pnm":
            seq = fiasco_amd.Sequence(lib, pnms, 20.0, o)
        else:
            seq = fiasco_amd.Sequence.from_device(lib, list(dev), 20.0, o)
        t_open = time.perf_counter() - t0
        if route == "outputs":
            seq.set_outputs(list(targets), True)
        data = seq.encode()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    st = lib.get_stats()
    res = {"wall_s": wall, "open_s": t_open, "md5": hashlib.md5(data).hexdigest(), "decoder_frames": int(st.decoder_frames),
           "decoder_us": int(st.decoder_us)}
    res.update(phases(err.text))
    if route == "outputs":
        sse, mx, wr = seq.distortion()
        res["written"] = int(wr.sum())
        res["sse_y_mean"] = float(sse[:, 0].mean())
    seq.free()
    return res


def ab(parent, frames, reps):
    """tests/gpu_config5.py in fresh processes, this library and the parent's alternating -> seconds of fiasco_coder()"""
    out = {"new": [], "parent": []}
    pair = (("parent", parent), ("new", fiasco_amd.LIB_PATH))
    for r in range(reps):
        for which, lib in (pair if r % 2 == 0 else pair[::-1]):        # who goes first changes from round to round
            env = dict(os.environ, FIASCO_AMD_LIB=lib)
            env.pop("FIASCO_AMD_SEQ_TIMING", None)
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_config5.py"), str(frames)], env=env,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            assert frames != 300 or j["md5"] == REFERENCE_MD5, (which, j["md5"])
            out[which].append(j["seconds"])
            print("ab %s: %.2f s" % (which, j["seconds"]), flush=True)
    res = {k: stat(v) for k, v in out.items()}
    res["seconds_in_order"] = out
    res["new_inside_parents_spread"] = res["parent"]["min"] <= res["new"]["median"] <= res["parent"]["max"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ab", default=None, help="libfiasco_amd.so of the parent commit")
    ap.add_argument("--ab-only", action="store_true", help="only the comparison with the parent, into the file --out names")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_device.json"))
    a = ap.parse_args()
    if a.ab_only:
        res = json.load(open(a.out))
        res["pnm_fed_fiasco_coder_against_parent_s"] = ab(a.ab, a.frames, a.reps)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res["pnm_fed_fiasco_coder_against_parent_s"]))
        return
    # the frames first, on the host's cores, before anything touches the GPU (forked workers)
    with mp.get_context("fork").Pool(min(16, len(os.sched_getaffinity(0)))) as pool:
        frames = np.stack(pool.map(make_frame, range(a.frames)))
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    pnms = [synth.ppm_bytes(f) for f in frames]
    dev = torch.from_numpy(frames).cuda()
    targets = torch.zeros_like(dev)
    o = lib.cli_options()
    o.set_prediction(1, 6, 10)
    res = {"device": torch.cuda.get_device_name(0), "workload": "%d frames %d x %d colour, ippppppppp, --prediction" % (a.frames, W, H),
           "reps": a.reps, "reference_md5": REFERENCE_MD5, "runs": {"pnm": [], "device": [], "outputs": []}}
    one(lib, "pnm", pnms, dev, targets, o)                      # warm-up
    for r in range(a.reps):
        for route in ("pnm", "device", "outputs"):
            res["runs"][route].append(one(lib, route, pnms, dev, targets, o))
            print(route, json.dumps(res["runs"][route][-1]), flush=True)
    for route, runs in res["runs"].items():
        res[route] = {k: stat([x[k] for x in runs]) for k in ("wall_s", "open_s", "prepare", "core", "decode", "probe", "writer")}
        res[route]["decoder_frames"] = runs[0]["decoder_frames"]
        res[route]["decoder_us_per_frame"] = stat([x["decoder_us"] / max(x["decoder_frames"], 1) for x in runs])
        res[route]["md5_is_the_references"] = all(x["md5"] == REFERENCE_MD5 for x in runs)
    res["device_feeding_saves_s"] = res["pnm"]["wall_s"]["median"] - res["device"]["wall_s"]["median"]
    res["outputs_cost_s"] = res["outputs"]["wall_s"]["median"] - res["device"]["wall_s"]["median"]
    o.delete()
    del dev, targets
    torch.cuda.empty_cache()
    if a.ab:
        res["pnm_fed_fiasco_coder_against_parent_s"] = ab(a.ab, a.frames, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "runs"}))
    assert a.frames != 300 or all(res[r]["md5_is_the_references"] for r in ("pnm", "device", "outputs")), "a stream is not the reference's"


if __name__ == "__main__":
    main()
