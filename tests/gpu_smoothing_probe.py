#!/usr/bin/env python3
"""Developer probe (not part of the suite): what smoothing decoded frames on the device costs a decoder flight.

Two workloads, each ONE flight of 32 device-fed replicas of one frame: gray 1920 x 1080 and colour 1280 x 720.  Four
routes from the finished automata to 8-bit pixels in device memory, timed by the decoder's own device time for the
flight (fiasco_amd_stats.decoder_us: HIP events around uploads, kernels and the conversion):
  parent        Batch.decode_device() of a library built from the parent commit (--parent-lib); parent_2nd and
                parent_3rd are the same call again, so that both processes make three calls per round
  old_entry     the same call on this tree's library
  smoothing_0   fiasco_amd_batch_decode_device_smoothed(smoothing = 0) on this tree's library
  smoothing_70  ... (smoothing = 70): one launch of sm_pass_kernel per pass of the border list more
The parent's library and this tree's run in separate child processes of one session, the parent first; this process
never opens the device.  In a child the routes alternate, one warm-up round and then 9 measured ones; after EVERY call
the device is synchronised and the error state checked, and a child that meets an error says which route and call it
was, exits at once and nothing more is started.  The bytes of old_entry and smoothing_0 must be equal, those of
smoothing_70 must differ.

Acceptance (recorded as booleans, judged by the reader): the medians of old_entry and smoothing_0 lie inside the
parent's own min .. max of the session.  The cost of smoothing_70 is recorded, not bounded, with the borders and passes
per frame.  Writes profiles/smoothing_device.json."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKLOADS = {"gray_1080p": (1920, 1080, False), "colour_720p": (1280, 720, True)}
FRAMES, REPS = 32, 9


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)}


def child(path, routes, out):
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import fiasco_amd
    import synth
    assert torch.cuda.is_available(), "the probe needs a GPU"
    lib = fiasco_amd.Library(path)
    assert lib.core_name() == "hip-gfx950"
    lib.set_verbosity(0)
    res = {"library": path, "device": torch.cuda.get_device_name(0), "workloads": {}}

    def run(b, route, targets):
        if route.startswith("parent") or route == "old_entry":
            return b.decode_device(targets)
        arr = fiasco_amd._device_targets(targets)
        return lib.L.fiasco_amd_batch_decode_device_smoothed(b.handle, 70 if route == "smoothing_70" else 0, arr,
                                                             fiasco_amd._stream_of(targets, None))

    for name, (w, h, colour) in WORKLOADS.items():
        frame = synth.synth_color_k(w, h, 1234) if colour else synth.synth(w, h, 1234)
        src = torch.from_numpy(frame).cuda().unsqueeze(0).repeat(FRAMES, *([1] * frame.ndim))
        o = lib.cli_options()
        b = fiasco_amd.Batch.from_device(lib, list(src), 20.0, o)
        assert None not in b.encode(), lib.error_message()
        torch.cuda.synchronize()
        borders = b.smoothing_borders(0)
        wl = {"frames": FRAMES, "width": w, "height": h, "colour": colour, "borders_per_frame": len(borders),
              "passes_per_frame": borders[-1][4] + 1, "pairs_per_frame": sum(x[2] for x in borders), "routes": {}}
        us = {r: [] for r in routes}
        md5 = {}
        for rep in range(REPS + 1):                     # round 0 warms up
            for route in routes:
                targets = [torch.zeros(frame.shape, dtype=torch.uint8, device="cuda") for _ in range(FRAMES)]
                torch.cuda.synchronize()
                lib.reset_stats()
                where = "%s, %s, call %d" % (name, route, rep)
                try:
                    good = run(b, route, targets)
                    torch.cuda.synchronize()            # raises on a device error
                except Exception as e:                  # noqa: BLE001
                    print("PROBE ERROR at %s: %s" % (where, e), flush=True)
                    sys.exit(3)
                st = lib.get_stats()
                if good != FRAMES or st.decoder_frames != FRAMES:
                    print("PROBE ERROR at %s: %d of %d frames: %s" % (where, good, FRAMES, lib.error_message()), flush=True)
                    sys.exit(3)
                if rep:
                    us[route].append(st.decoder_us)
                if rep in (0, REPS):                    # the bytes of the first and of the last call
                    digest = hashlib.md5(torch.stack(targets).cpu().numpy().tobytes()).hexdigest()
                    if md5.setdefault(route, digest) != digest:
                        print("PROBE ERROR at %s: the bytes changed between two calls" % where, flush=True)
                        sys.exit(3)
                print("ok %s: %d us" % (where, st.decoder_us), flush=True)
        for route in routes:
            wl["routes"][route] = dict(stat(us[route]), md5=md5[route], unit="decoder_us of the flight")
        res["workloads"][name] = wl
        b.free(); o.delete()
        del src
        with open(out, "w") as f:                       # after every workload: what was measured survives a later error
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="libfiasco_amd.so built from the parent commit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smoothing_device.json"))
    ap.add_argument("--scratch", default=None, help="where the two processes leave their parts (default: a temporary directory)")
    ap.add_argument("--child", nargs=3, metavar=("LIB", "ROUTES", "OUT"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1].split(","), a.child[2])
        return 0
    assert a.parent_lib and os.path.exists(a.parent_lib), "--parent-lib: a library built from the parent commit"
    if a.scratch is None:
        a.scratch = tempfile.mkdtemp(prefix="smoothing_probe_")
    os.makedirs(a.scratch, exist_ok=True)
    new_lib = os.path.join(ROOT, "fiasco_amd", "libfiasco_amd.so")
    parts = []
    # three calls per round in either process, so that the two are loaded alike (a parent process with ONE call per round
    # measured 2442 us for gray 1080p where this tree's old entry point measured 2305 in its three-route process).
    # parent_2nd and parent_3rd are the same call again
    for lib, routes, tag in ((a.parent_lib, "parent,parent_2nd,parent_3rd", "parent"), (new_lib, "old_entry,smoothing_0,smoothing_70", "new")):
        out = os.path.join(a.scratch, "smoothing_probe_%s.json" % tag)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", lib, routes, out], timeout=420)
        if r.returncode != 0:
            print("the %s library's process ended with status %d: nothing more is started" % (tag, r.returncode), flush=True)
            return 1
        parts.append(json.load(open(out)))
    res = {"device": parts[0]["device"], "method": "one flight of %d device-fed replicas; decoder_us of the flight; 1 warm-up round, then %d "
           "rounds, routes alternating; parent and new library in separate processes of one session" % (FRAMES, REPS), "workloads": {}}
    ok = True
    for name in WORKLOADS:
        wl = parts[1]["workloads"][name]
        wl["routes"] = dict(parts[0]["workloads"][name]["routes"], **wl["routes"])
        p, r = wl["routes"]["parent"], wl["routes"]
        wl["old_entry_inside_parent_spread"] = p["min"] <= r["old_entry"]["median"] <= p["max"]
        wl["smoothing_0_inside_parent_spread"] = p["min"] <= r["smoothing_0"]["median"] <= p["max"]
        again = [r[k] for k in ("parent", "parent_2nd", "parent_3rd")]
        wl["parent_spread_of_all_three"] = {"min": min(x["min"] for x in again), "max": max(x["max"] for x in again)}
        wl["smoothing_70_cost_us"] = r["smoothing_70"]["median"] - r["old_entry"]["median"]
        wl["smoothing_70_cost_us_per_pass"] = wl["smoothing_70_cost_us"] / wl["passes_per_frame"]
        wl["bytes_equal_parent_old_entry_smoothing_0"] = p["md5"] == r["old_entry"]["md5"] == r["smoothing_0"]["md5"]
        wl["bytes_differ_smoothing_70"] = r["smoothing_70"]["md5"] != r["old_entry"]["md5"]
        ok = ok and wl["bytes_equal_parent_old_entry_smoothing_0"] and wl["bytes_differ_smoothing_70"]
        res["workloads"][name] = wl
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res, indent=1))
    return 0 if ok else 2


if __name__ == "__main__":
    sys.exit(main())
