"""What tests/golden/make_video_param.py, tests/test_video_param_pins.py (CPU oracle) and tests/test_gpu_video_param.py
(device) share: the cases of tests/golden/VIDEO_PARAM.json and the helpers that run a library, or the reference library,
with fiasco_c_options_set_video_param(fps, half_pixel = 0, cross_B_search, B_as_past_ref).  No codec logic here: inputs,
selection, file handling; the planes, the block counts and the checks are those of tests/reconst_cases.py.

Why.  The reference's command-line tool parses --fps, --cross-B-search and --B-as-past-ref and drops them (bin/cwfa.c
never calls the setter), so every stream a `cfiasco` made has the library defaults fps = 25, B_as_past_ref = YES.  The
setter is part of fiasco.h, though, and with B_as_past_ref = NO a B frame that follows a B frame keeps the old past
reference (codec/coder.c:603-627, host/fa_sequence.c).  The reference is therefore driven as a LIBRARY here:
oracle/_ref/libfiasco_ref_recon.so (oracle/ref_build.sh: the reference with the block that writes its reconstructed
frames) through ctypes, the option calls in the order of bin/cwfa.c:252-393, then set_video_param, then fiasco_coder.
Its error path ends the process, so every run is a child process of its own (`python tests/video_param_cases.py DIR`).

A case is (frames, cfiasco arguments, (fps, cross_B_search, B_as_past_ref)).  Its name says all three.  The patterns are
the coding orders that `--pattern` can reach and nothing else pins: a P frame coded right after a B frame (`ibpbp`: coding
order I0 P2 B1 P4 B3; P4 takes B1's reconstruction as its past whatever the flag says, codec/coder.c:593-598), runs of
three and four B frames, two B runs in one group of pictures, trailing B runs (the last frame is forced to P), uppercase.
The twin of a case is the same case with the other flag value.  Gray frames are the moving windows of
reconst_cases._shift.  The two colour cases take frames the reference was found to code under their pattern with both
flag values: under `ibbp` and `ibpbp` it ends with "Can't write more than n weights" on reconst_cases._saturated (-q 20,
40, 60, 90), on synth_color_c (the inputs of seq3_color_ibp) at 96 x 64 and 128 x 96 and on most other small colour frames
tried, so they are the gray windows tinted (`ibbp`) and synth_color_k at 70 x 50 (`ibpbp`).

The random cases (random_case): default_rng(seed); pattern "i" + 1 .. 3 groups of (0 .. 3 `b`, then `p`) -- no B run ever
meets an `i`, so the cyclic continuation of the pattern is safe; 3 .. 9 frames; colour 1 in 4; flag, cross and prediction
0 / 1 each; fps of FUZZ_FPS; even sides 32 .. 128 x 32 .. 96; the first frame from fuzz_parity.random_image, every later
frame the first one rolled by up to +-3 f pixels in both directions with +-2 noise.
"""
import json
import os
import subprocess
import sys

import numpy as np

import reconst_cases as rc
import synth
from conftest import GOLDEN, REF_SHARE, options_from_args
from fuzz_parity import random_image

FIXTURE = os.path.join(GOLDEN, "VIDEO_PARAM.json")
REF_LIB = os.path.join(rc.REF_DIR, "libfiasco_ref_recon.so")
REFUSAL = "Motion search without a reference frame (frame pattern)."


def _tinted(n):
    """the windows of reconst_cases._shift as colour frames: R, G, B = gray + 30, - 20, + 10, clipped to a byte"""
    a = synth.synth(160, 120, 7).astype(np.int32)
    return [synth.ppm_bytes(np.clip(np.stack([a[10 + 2 * i:80 + 2 * i, 20 + 3 * i:120 + 3 * i] + d for d in (30, -20, 10)], -1),
                                    0, 255).astype(np.uint8)) for i in range(n)]


def _colour_k(n):
    """synth.synth_color_k (textured chroma) at 70 x 50, moving by one pixel per frame"""
    return [synth.ppm_bytes(synth.synth_color_k(70, 50, 6, f)) for f in range(n)]


def _name(pattern, n, vp, extra=""):
    return "%s_x%d%s_fps%d_cross%d_b%d" % (pattern, n, extra, vp[0], vp[1], vp[2])


def _gray(pattern, n, vp, more=()):
    return _name(pattern, n, vp, "_pred" if more else ""), ((lambda: rc._shift(n)), ["--pattern", pattern] + list(more), tuple(vp))


# name -> (frames, cfiasco arguments, (fps, cross_B_search, B_as_past_ref))
CASES = dict(
    [_gray("ibbp", 4, vp) for vp in ((25, 1, 0), (25, 0, 0), (30, 0, 1), (0, 1, 0), (100000, 1, 0))]
    + [_gray("IBBP", 4, (25, 1, 0))]
    + [_gray(p, n, (25, 1, b)) for p, n in (("ibbbp", 5), ("ibbbbp", 6), ("ibpbp", 5), ("ibbpbp", 6)) for b in (0, 1)]
    + [_gray("ibbpbbp", 7, (25, 1, b), ["--prediction"]) for b in (0, 1)]
    + [_gray(p, n, (25, 1, 0)) for p, n in (("ipbbpbbp", 8), ("ipbpb", 5), ("ibb", 3), ("ib", 2))]
    + [_gray("ibbp", 9, (25, 1, b)) for b in (0, 1)]
    + [("colour_" + _name("ibbp", 4, (25, 1, 0)), ((lambda: _tinted(4)), ["--pattern", "ibbp"], (25, 1, 0))),
       ("colour_" + _name("ibpbp", 5, (25, 1, 0)), ((lambda: _colour_k(5)), ["--pattern", "ibpbp"], (25, 1, 0)))])
NAMES = list(CASES)
# an I frame between a B frame and its future reference: the reference dies (a null frame at its first motion search),
# the libraries refuse
REFUSED = dict([_gray("ibbi", 4, (25, 1, 0)), _gray("ipbbi", 5, (25, 1, 0))])

LOWERCASE_TWIN = {_name("IBBP", 4, (25, 1, 0)): _name("ibbp", 4, (25, 1, 0))}
CROSS_TWIN = (_name("ibbp", 4, (25, 0, 0)), _name("ibbp", 4, (25, 1, 0)))        # codec/coder.c:359 overwrites cross_B_search
FPS_CASES = [n for n in NAMES if n.startswith("ibbp_x4_")]
P_AFTER_B = {_name("ibpbp", 5, (25, 1, b)): 4 for b in (0, 1)}                   # case -> display number of that P frame
P_AFTER_B.update({_name("ibbpbp", 6, (25, 1, b)): 5 for b in (0, 1)})
NO_WIDE = [_name(p, n, (25, 1, 0), e) for p, n, e in (("ibbbp", 5, ""), ("ibpbp", 5, ""), ("ibbpbbp", 7, "_pred"))]
DEVICE_FED = [_name("ibbbp", 5, (25, 1, 0)), _name("ibpbp", 5, (25, 1, 0)), "colour_" + _name("ibpbp", 5, (25, 1, 0))]
THREE_GOPS = [_name("ibbp", 9, (25, 1, b)) for b in (0, 1)]

FUZZ_SEEDS = range(5200, 5224)
FUZZ_MIN_COMPARED = 18
FUZZ_FPS = [0, 1, 24, 25, 30, 60, 1000, 65536]


def case_of(name):
    """-> (frames as PNM bytes, cfiasco arguments, (fps, cross_B_search, B_as_past_ref))"""
    make, args, vp = (CASES.get(name) or REFUSED[name])
    return make(), list(args), vp


def twin_of(vp):
    return (vp[0], vp[1], 1 - vp[2])


def has_b_after_b(types):
    """two B frames in a row among the frame types in display order (a trailing B frame is coded as a P frame): the
    only place where B_as_past_ref changes a reference"""
    return any(a == 2 and b == 2 for a, b in zip(types, types[1:]))


def fixture():
    return json.load(open(FIXTURE))


def random_case(seed):
    """-> (frames as PNM bytes, cfiasco arguments, (fps, cross_B_search, B_as_past_ref))"""
    rng = np.random.default_rng(seed)
    pattern = "i" + "".join("b" * int(rng.integers(0, 4)) + "p" for _ in range(int(rng.integers(1, 4))))
    nfr = int(rng.integers(3, 10))
    colour = bool(rng.integers(0, 4) == 0)
    flag, cross, pred = (int(rng.integers(0, 2)) for _ in range(3))
    fps = int(rng.choice(FUZZ_FPS))
    w, h = int(rng.integers(16, 65)) * 2, int(rng.integers(16, 49)) * 2
    first = random_image(rng, colour, (w, h))
    shape = (h, w, 3) if colour else (h, w)
    a0 = np.frombuffer(first[len(first) - int(np.prod(shape)):], np.uint8).reshape(shape)
    frames = [first]
    for f in range(1, nfr):
        a = np.roll(a0, (int(rng.integers(-3, 4)) * f, int(rng.integers(-3, 4)) * f), (0, 1)).astype(np.int32)
        a = np.clip(a + rng.integers(-2, 3, a.shape), 0, 255).astype(np.uint8)
        frames.append((synth.ppm_bytes if colour else synth.pgm_bytes)(a))
    return frames, ["--pattern", pattern] + (["--prediction"] if pred else []), (fps, cross, flag)


# ------------------------------------------------------------------ running a library of this project

def open_options(lib, args, vp):
    """options_from_args, then set_video_param as a caller of fiasco.h makes it -> (quality, options)"""
    q, o = options_from_args(lib, args)
    o.set_video_param(vp[0], 0, vp[1], vp[2])
    return q, o


def run_library(lib, frames, args, vp, tmp, env=None, out_holds=None):
    """reconst_cases.run_library with the video parameters set; env: variables that hold during the call; out_holds:
    bytes the output file holds before the call -> (stream or None, {display: (type, planes)}, {display: counts}, message)"""
    names = rc.write_inputs(frames, tmp)
    dump = os.path.join(str(tmp), "dump_" + lib.core_name())
    os.makedirs(dump)
    q, o = open_options(lib, args, vp)
    out = os.path.join(str(tmp), lib.core_name() + ".fco")
    if out_holds is not None:
        open(out, "wb").write(out_holds)
    held = dict(env or {}, FIASCO_AMD_SEQ_RECONST_DIR=dump)
    old = {k: os.environ.get(k) for k in held}
    os.environ.update(held)
    try:
        ok = lib.fiasco_coder(names, out, q, o)
        msg = lib.error_message() if ok != 1 else ""
    finally:
        o.delete()
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    if ok != 1:
        assert ok == 0, ok
        return None, {}, {}, msg
    return open(out, "rb").read(), rc._read_planes(dump, "d", rc.geometry(frames)), rc._read_counts(dump), ""


def refusal_leaves_the_output(lib, name, tmp):
    """a refused pattern: 0, the message, and the bytes an existing output file held"""
    frames, args, vp = case_of(name)
    stream, _, _, msg = run_library(lib, frames, args, vp, tmp, out_holds=b"keep")
    assert stream is None and msg == REFUSAL, (name, msg)
    assert open(os.path.join(str(tmp), lib.core_name() + ".fco"), "rb").read() == b"keep", name


# ------------------------------------------------------------------ running the reference library, a child per case

class _Noted:
    """stands in for a library in options_from_args: notes the setter calls instead of making them"""

    def __init__(self):
        self.calls = {}

    def cli_options(self, *a, **kw):
        import fiasco_amd
        return fiasco_amd.Library.cli_options(self, *a, **kw)

    def c_options_new(self):
        return self

    def __getattr__(self, name):
        if name.startswith("set_"):
            return lambda *a: self.calls.__setitem__(name, a)
        raise AttributeError(name)


CWFA_ORDER = ["set_frame_pattern", "set_basisfile", "set_chroma_quality", "set_smoothing", "set_progress_meter", "set_title",
              "set_comment", "set_tiling", "set_optimizations", "set_prediction", "set_quantization"]


def _child(workdir):
    """one fiasco_coder() call of the reference library; exit status 0 where it wrote a stream"""
    import fiasco_amd
    job = json.load(open(os.path.join(workdir, "job.json")))
    ref = fiasco_amd.Library(job["library"])
    noted = _Noted()
    quality, _ = options_from_args(noted, job["args"])
    noted.calls.setdefault("set_basisfile", (b"small.fco",))        # bin/cwfa.c always names one: its default
    assert set(noted.calls) <= set(CWFA_ORDER), sorted(noted.calls)
    o = ref.c_options_new()
    for call in CWFA_ORDER:
        if call in noted.calls:
            getattr(o, call)(*noted.calls[call])
    if job["video_param"] is not None:
        fps, cross, flag = job["video_param"]
        o.set_video_param(fps, 0, cross, flag)
    sys.stdout.flush()
    ok = ref.fiasco_coder(job["names"], job["out"], quality, o)
    if ok != 1:
        sys.stderr.write(ref.error_message() + "\n")
    sys.exit(0 if ok == 1 else 1)


def run_reference_library(frames, args, vp, tmp, dump=True, library=REF_LIB):
    """libfiasco_ref_recon.so in a child process.  vp None: set_video_param is not called, as bin/cwfa.c does not.
    -> (None or why there is no stream, stream, {display: (type, planes)}); any status but 0 means no stream"""
    names = rc.write_inputs(frames, tmp)
    d = os.path.join(str(tmp), "dump_reflib")
    os.makedirs(d, exist_ok=True)
    out = os.path.join(str(tmp), "reflib.fco")
    json.dump({"library": library, "names": names, "args": list(args), "video_param": None if vp is None else list(vp), "out": out},
              open(os.path.join(str(tmp), "job.json"), "w"))
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    env.pop("FIASCO_REF_RECONST_DIR", None)
    if dump:
        env["FIASCO_REF_RECONST_DIR"] = d
    r = subprocess.run([sys.executable, os.path.abspath(__file__), str(tmp)], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    if r.returncode < 0:
        return "signal %d" % -r.returncode, None, {}
    if r.returncode != 0:
        last = r.stderr.decode("latin-1").strip().split("\n")[-1]
        return "exit %d: %s" % (r.returncode, last), None, {}
    return None, open(out, "rb").read(), (rc._read_planes(d, "r", rc.geometry(frames)) if dump else {})


# ------------------------------------------------------------------ the checks both libraries go through

def check_case(name, rec, stream, planes, counts):
    """reconst_cases.check_against_fixture, and the numbers of blocks restore_mc applies to every frame"""
    rc.check_against_fixture(name, rec, stream, planes, counts)
    for f in rec["frames"]:
        c = counts[f["display"]]
        assert [c["forward"], c["backward"], c["interpolated"]] == f["blocks"], (name, f["display"], c)


def check_not_hollow(runs):
    """runs: {name: (stream, planes, counts)} of every pinned case.  Every flag-0 case with two B frames in a row differs
    from its twin -- the fixture's record of the reference's twin -- in the stream and in a B frame's planes; where both
    twins are pinned the runs themselves differ there; the P frame coded right after a B frame has a forward block"""
    fx = fixture()["cases"]
    for name in NAMES:
        vp = CASES[name][2]
        types = {f["display"]: f["type"] for f in fx[name]["frames"]}
        if vp[2] == 0 and has_b_after_b([types[d] for d in sorted(types)]):
            twin = fx[name]["twin"]
            assert twin["stream_differs"] and any(types[d] == 2 for d in twin["planes_differ"]), (name, twin)
            other = name[:-1] + "1"
            if other in runs:
                assert runs[name][0] != runs[other][0], name
                differ = [d for d in sorted(types) if not np.array_equal(runs[name][1][d][1], runs[other][1][d][1])]
                assert differ == twin["planes_differ"], (name, differ, twin)
    for name, display in P_AFTER_B.items():
        t, _ = runs[name][1][display]
        assert t == 1 and runs[name][2][display]["forward"] >= 1, (name, runs[name][2][display])


def fuzz_seed(lib, seed, tmp, yardstick=None, live=True):
    """One random case through `lib`: against the library `yardstick` (streams as bytes, planes as int16 arrays) and,
    where libfiasco_ref_recon.so is there and `live`, against the reference library in a child process.  A seed is left
    out only where both libraries refuse; the reference is compared wherever it writes a stream.
    -> ("compared" | "skipped" | "MISMATCH", text, whether the reference coded it)"""
    frames, args, vp = random_case(seed)
    what = "seed %d %s %s fps %d cross %d B_as_past_ref %d, %d frames" % ((seed, rc.geometry(frames), " ".join(args)) + vp + (len(frames),))
    stream, planes, counts, msg = run_library(lib, frames, args, vp, os.path.join(str(tmp), "lib%d" % seed))
    ymsg = "no yardstick"
    if yardstick is not None:
        ystream, yplanes, _, ymsg = run_library(yardstick, frames, args, vp, os.path.join(str(tmp), "yard%d" % seed))
        if (stream is None) != (ystream is None):
            return "MISMATCH", "%s: one of the two fails: %r; %s: %r" % (what, msg, yardstick.core_name(), ymsg), False
    if stream is not None:
        if sorted(planes) != list(range(len(frames))) or any(c["skipped"] for c in counts.values()):
            return "MISMATCH", "%s: reconstructed %s, skipped blocks %s" % (what, sorted(planes), [c["skipped"] for c in counts.values()]), False
        bad = yardstick is not None and rc.compare_runs(what, stream, planes, ystream, yplanes, yardstick.core_name())
        if bad:
            return "MISMATCH", bad, False
    coded = False
    if live and os.path.exists(REF_LIB):
        err, rstream, rplanes = run_reference_library(frames, args, vp, os.path.join(str(tmp), "ref%d" % seed))
        coded = err is None
        if coded and stream is None:
            return "MISMATCH", "%s: the reference codes it, the library fails: %s" % (what, msg), coded
        if coded:
            bad = rc.compare_runs(what, stream, planes, rstream, rplanes, "the reference library")
            if bad:
                return "MISMATCH", bad, coded
        elif stream is not None:
            what += " (reference: %s)" % err
    if stream is None:
        return "skipped", "%s: both fail: %s; %s" % (what, msg, ymsg), coded
    return "compared", what, coded


if __name__ == "__main__":
    _child(sys.argv[1])
