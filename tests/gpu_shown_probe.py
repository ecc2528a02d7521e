#!/usr/bin/env python3
"""Developer probe (not part of the suite): which smoothed planes of a decoder flight should take the fused kernel
(sm_frame_kernel: one launch, one workgroup per plane, all passes) and which the per-pass launches (sm_pass_kernel: one
launch per pass for all planes of the flight) -- the measurement behind SM_FUSED_MAX_PAIRS (csrc/hip/smooth.inc) -- and what
smoothing costs a flight of thumbnails.

Shapes: ONE flight of 32 device-fed replicas of a gray frame of 256 x 256, 1024 x 768 and 1920 x 1080, each shown at
magnifications 0, -1, -2 and -3 where the size rule allows: planes from a 32 x 32 thumbnail to a coded 1080p frame.  Three
routes per shape through fiasco_amd_batch_decode_device_shown():
  unsmoothed   smoothing 0
  per_pass     smoothing 70, developer switch FIASCO_AMD_SMOOTH_FUSED=0
  fused        smoothing 70, FIASCO_AMD_SMOOTH_FUSED=1
The switch is read when a flight is prepared, so the routes alternate call by call in ONE process.  Time: the decoder's own
device time for the flight (fiasco_amd_stats.decoder_us: device events around uploads, kernels and the conversion).  Every
shape is warmed up with one round, then measured for 20 rounds, and the whole sweep runs twice: per route the two medians
and their difference, the spread.  After EVERY call the device is synchronised and the error state checked; on an error
the probe says which call it was, exits at once and starts nothing more.  per_pass and fused must write equal bytes,
unsmoothed other ones.

fused_wins: the mean of the two per_pass medians exceeds that of the two fused medians by more than the larger spread of the
two routes.  threshold_pairs: the largest pairs-per-plane of a shape where fused wins (0: nowhere).  Writes all numbers to
--out (default profiles/shown_device.json)."""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [(256, 256), (1024, 768), (1920, 1080)]
MAGS = (0, -1, -2, -3)
ROUTES = ("unsmoothed", "per_pass", "fused")
FRAMES, REPS, RUNS = 32, 20, 2
PARENT_THUMBS_US = 993          # README: a flight of 32 gray 1080p frames as thumbnails at -2, unsmoothed, parent commit


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shown_device.json"))
    a = ap.parse_args()
    os.environ["FIASCO_AMD_DEBUG"] = "1"
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fiasco_amd
    import synth
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.library()
    lib.set_verbosity(0)
    res = {"device": torch.cuda.get_device_name(0),
           "method": "one flight of %d device-fed replicas per shape; decoder_us of the flight (device events); 1 warm-up round, then %d "
                     "rounds, the three routes alternating call by call in one process; the sweep runs %d times" % (FRAMES, REPS, RUNS),
           "sweep": []}

    def call(b, route, m, targets, where):
        os.environ["FIASCO_AMD_SMOOTH_FUSED"] = "1" if route == "fused" else "0"
        torch.cuda.synchronize()
        lib.reset_stats()
        try:
            good = b.decode_shown(targets, magnify=m, smoothing=0 if route == "unsmoothed" else 70)
            torch.cuda.synchronize()                    # raises on a device error
        except Exception as e:                          # noqa: BLE001
            print("PROBE ERROR at %s: %s" % (where, e), flush=True)
            sys.exit(3)
        st = lib.get_stats()
        if good != FRAMES or st.decoder_frames != FRAMES:
            print("PROBE ERROR at %s: %d of %d frames: %s" % (where, good, FRAMES, lib.error_message()), flush=True)
            sys.exit(3)
        return st.decoder_us

    for w, h in SOURCES:
        frame = synth.synth(w, h, 1234)
        src = torch.from_numpy(frame).cuda().unsqueeze(0).repeat(FRAMES, 1, 1)
        o = lib.cli_options()
        b = fiasco_amd.Batch.from_device(lib, list(src), 20.0, o)
        assert None not in b.encode(), lib.error_message()
        torch.cuda.synchronize()
        for m in MAGS:
            try:
                mw, mh = fiasco_amd.magnified_size(lib, w, h, m)
            except fiasco_amd.FiascoError:
                continue
            borders = b.smoothing_borders(0, magnify=m)
            row = {"source": [w, h], "magnify": m, "width": mw, "height": mh, "borders": len(borders), "passes": borders[-1][4] + 1,
                   "pairs": sum(x[2] for x in borders), "runs": []}
            targets = [torch.zeros((mh, mw), dtype=torch.uint8, device="cuda") for _ in range(FRAMES)]
            md5 = {}
            for run in range(RUNS):
                us = {r: [] for r in ROUTES}
                for rep in range(REPS + 1):             # round 0 warms up
                    for route in ROUTES:
                        t = call(b, route, m, targets, "%d x %d at %d, %s, run %d, call %d" % (w, h, m, route, run, rep))
                        if rep:
                            us[route].append(t)
                        if rep in (0, REPS):
                            digest = hashlib.md5(torch.stack(targets).cpu().numpy().tobytes()).hexdigest()
                            if md5.setdefault(route, digest) != digest:
                                print("PROBE ERROR: the bytes of %s changed between two calls" % route, flush=True)
                                sys.exit(3)
                row["runs"].append({r: {"median": statistics.median(us[r]), "min": min(us[r]), "max": max(us[r]), "n": len(us[r])} for r in ROUTES})
            if md5["per_pass"] != md5["fused"] or md5["per_pass"] == md5["unsmoothed"]:
                print("PROBE ERROR: %d x %d at %d: per_pass and fused differ, or smoothing changed nothing" % (w, h, m), flush=True)
                sys.exit(3)
            med = {r: [run[r]["median"] for run in row["runs"]] for r in ROUTES}
            row["median_us"] = {r: statistics.mean(med[r]) for r in ROUTES}
            row["spread_us"] = {r: max(med[r]) - min(med[r]) for r in ROUTES}
            row["fused_gain_us"] = row["median_us"]["per_pass"] - row["median_us"]["fused"]
            row["fused_wins"] = row["fused_gain_us"] > max(row["spread_us"]["per_pass"], row["spread_us"]["fused"])
            row["smoothing_cost_us"] = {r: row["median_us"][r] - row["median_us"]["unsmoothed"] for r in ("per_pass", "fused")}
            res["sweep"].append(row)
            print("%4d x %-4d at %2d: %4d x %-4d %6d pairs %2d passes | unsmoothed %7.1f per_pass %7.1f fused %7.1f us | spread %5.1f | fused %s"
                  % (w, h, m, mw, mh, row["pairs"], row["passes"], row["median_us"]["unsmoothed"], row["median_us"]["per_pass"],
                     row["median_us"]["fused"], max(row["spread_us"].values()), "wins" if row["fused_wins"] else "does not win"), flush=True)
            if (w, h, m) == (1920, 1080, -2):
                res["thumbnails_1080p_at_-2"] = dict(row["median_us"], parent_unsmoothed_us=PARENT_THUMBS_US, unit="decoder_us of a flight of 32")
            with open(a.out, "w") as f:                 # after every shape: what was measured survives a later error
                json.dump(res, f, indent=1)
        b.free(); o.delete()
        del src
    wins = [r["pairs"] for r in res["sweep"] if r["fused_wins"]]
    res["threshold_pairs"] = max(wins) if wins else 0
    res["rule"] = "threshold_pairs = the largest pairs-per-plane of a measured shape at which fused_gain_us exceeds the spread of the two runs' medians"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("threshold_pairs = %d" % res["threshold_pairs"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
