"""What tests/test_reconst_pins.py (CPU oracle) and tests/test_gpu_reconst.py (device) share: the cases of
tests/golden/RECONST.json and the helpers that run a library, the reference coder and the reference decoder on one
sequence and collect the reconstructed frames.  No codec logic here: inputs, selection, file handling.

The yardstick.  A reconstructed frame is what the coder decodes after it has coded a frame (decode_image + restore_mc,
reference codec/coder.c:647-651) and what it predicts the next P or B frame from: 12.4 fixed point planes, int16,
1 or 3 bands of width * height.  The REFERENCE CODER's own planes are the yardstick: oracle/ref_build.sh builds
cfiasco_ref_recon, the reference coder with one added block that writes them (r<display>_t<type>.i16 under
FIASCO_REF_RECONST_DIR).  The reference's decoder front end is not one: on some videos `dfiasco -s 0` gives other
pixels on P and B frames than the coder reconstructed, or dies; the fixture records per frame whether it
agrees ("dfiasco_equal"), nothing is asserted about it.

A library under test (the CPU oracle, the device) writes its planes through FIASCO_AMD_SEQ_RECONST_DIR of the
sequence engine (fa_sequence.c): d<display>_t<type>.i16, and d<display>.txt with the numbers of motion blocks that
restore_mc applies to the frame by type and level.

Blocks above p_max_level.  The decoders here leave out a block whose level is above wfainfo->p_max_level (oracle/
oracle_decoder.c fa_restore_mc, frame_decoder.inc dec_prepare); the reference's restore_mc has no such test
(codec/motion.c:65-67).  No automaton a coder built can hold such a block: a motion vector is given to a range only
where try_mc holds, and try_mc asks for p_min_level <= level <= p_max_level (codec/subdivide.c:141-147); the children
of such a range are smaller (:311).  NONE_SKIPPED_CAN_EXIST says so, and the tests assert that the count is 0 on every
frame: a frame with a skipped block would be one where the restatements and the reference may differ.

The random cases (random_case): default_rng(seed); colour with probability 1 in 3; a pattern of PATTERNS with 3 .. 6
frames; --prediction 1 in 2; a prediction window (lo = 6 .. 10, hi = lo .. 12, as tests/test_gpu_fuzz_reference.py
make_case draws it) 1 in 3; -q of {5, 20, 45, 90}; -z 0 or 1; both mantissas 2 .. 8; chroma qfactor of {1, 2, 3.5};
even sizes 32 .. 128; the first frame from fuzz_parity.random_image, every later frame the first one rolled by up to
+-5 f pixels in both directions with +-3 noise.
"""
import hashlib
import json
import os
import subprocess

import numpy as np

import synth
from conftest import GOLDEN, REF_SHARE, ROOT, options_from_args
from fuzz_parity import random_image

FIXTURE = os.path.join(GOLDEN, "RECONST.json")
REF_DIR = os.path.join(ROOT, "oracle", "_ref")
CFIASCO = os.path.join(REF_DIR, "cfiasco_ref")
CFIASCO_RECON = os.path.join(REF_DIR, "cfiasco_ref_recon")
DFIASCO = os.path.join(REF_DIR, "dfiasco_ref")

NONE_SKIPPED_CAN_EXIST = True          # see the module docstring: no coder gives a vector to a block above p_max_level
CHROMA_CLIP = (-2048, 2032)            # restore_mc clips chroma to [-128, 127] * 16 (codec/motion.c:190-225)

# the refusals of the reference that the project names: a seed on which the reference ends with one is left out
REFERENCE_REFUSALS = ("Motion search without a reference frame", "Can't write more than")

# ------------------------------------------------------------------ the pinned inputs


def _shift(n):
    """100 x 70 windows of one 160 x 120 frame, moving by (3, 2) pixels per frame"""
    a = synth.synth(160, 120, 7)
    return [synth.pgm_bytes(a[10 + 2 * i:80 + 2 * i, 20 + 3 * i:120 + 3 * i].copy()) for i in range(n)]


def _reveal():
    """a brightened 32 x 32 square that only frames 2 and 3 show: a B frame whose past reference lacks it"""
    a = synth.synth(96, 64, 41)
    b = a.astype(np.int32)
    b[16:48, 32:64] += 60
    b = np.clip(b, 0, 255).astype(np.uint8)
    return [synth.pgm_bytes(f) for f in (a, a, b, b)]


def _checker(n=4):
    """0 / 255 checker board, squares of 8, moving by (3, 2) pixels per frame"""
    y, x = np.mgrid[0:64, 0:96]
    return [synth.pgm_bytes((255 * ((((x + 3 * i) // 8) + ((y + 2 * i) // 8)) % 2)).astype(np.uint8)) for i in range(n)]


def _noise(n=4):
    """white noise, rolled by (3, 2) pixels per frame"""
    a = np.random.default_rng(77).integers(0, 256, (70, 100)).astype(np.uint8)
    return [synth.pgm_bytes(np.roll(a, (2 * i, 3 * i), (0, 1))) for i in range(n)]


def _saturated(n=3):
    """a blue ground, a red and a green rectangle that move against each other: chroma at both clip bounds.  The
    reference refuses most frames of this kind ("Can't write more than n weights": 147 of 150 random placements of
    the two rectangles at -q 60 --pattern ibp); this placement is one it codes"""
    out = []
    for i in range(n):
        a = np.zeros((70, 100, 3), np.uint8)
        a[:, :, 2] = 255
        a[31:66, 2 + 4 * i:35 + 4 * i] = (255, 0, 0)
        a[4:43, 34 - 4 * i:72 - 4 * i] = (0, 255, 0)
        out.append(synth.ppm_bytes(a))
    return out


def _blend():
    """a B frame that is the mean of its two references, both white noise: 50 of its blocks are interpolated, each with
    two vectors.  (I and P frames hold even values only, so past + future is odd only where a reference is itself a B
    frame, the second B frame of an `ibbp` case: noise100x70_ibbp is the case that tells `>> 1` from `/ 2`.)"""
    a = np.random.default_rng(78).integers(0, 256, (70, 100)).astype(np.int32)
    c = np.random.default_rng(79).integers(0, 256, (70, 100)).astype(np.int32)
    return [synth.pgm_bytes(f.astype(np.uint8)) for f in (a, (a + c) // 2, c)]


# name -> (frames, cfiasco arguments); md5 of the joined inputs is in the fixture ("inputs_md5")
SYNTH_CASES = {
    "shift100x70_ippp": (lambda: _shift(4), ["--pattern", "ippp"]),
    "shift100x70_ibbp": (lambda: _shift(4), ["--pattern", "ibbp"]),
    "shift100x70_ibp": (lambda: _shift(5), ["--pattern", "ibp"]),
    "shift100x70_ibbp_pred": (lambda: _shift(4), ["--pattern", "ibbp", "--prediction"]),
    "shift100x70_ibbp_lv67": (lambda: _shift(5), ["--pattern", "ibbp", "--min-level", "6", "--max-level", "7"]),
    "reveal_ibbp": (_reveal, ["--pattern", "ibbp"]),
    "checker_q2_ippp": (_checker, ["-q", "2", "--pattern", "ippp"]),
    "checker_q2_ibbp": (_checker, ["-q", "2", "--pattern", "ibbp"]),
    "noise100x70_ippp": (_noise, ["--pattern", "ippp"]),
    "noise100x70_ibbp": (_noise, ["--pattern", "ibbp"]),
    "sat_q60_ibp": (_saturated, ["-q", "60", "--pattern", "ibp"]),
    "blend_q60_ibp": (_blend, ["-q", "60", "--pattern", "ibp"]),
    # several groups of pictures in one call: frames of different groups are reconstructed in one decoder batch
    "gops_ippi": (lambda: _shift(6), ["--pattern", "ippi"]),
    "gops_ibpi": (lambda: _shift(6), ["--pattern", "ibpi"]),
}
MULTI_GOP = ["gops_ippi", "gops_ibpi"]

# the random seeds pinned: those on which dfiasco_ref drifted from the reference coder or died when the set was chosen
PINNED_SEEDS = [9003, 9004, 9007, 9009, 9011, 9018, 9022]
FUZZ_SEEDS = range(9000, 9024)
FUZZ_MIN_COMPARED = 14
PATTERNS = ["ip", "ipp", "ippp", "ibp", "ibbp", "ipb", "ipbbp", "ippi", "ibpi"]
MAX_MANIFEST_WIDTH = 256


def random_case(seed):
    """-> (frames as PNM bytes, cfiasco arguments)"""
    rng = np.random.default_rng(seed)
    colour = bool(rng.integers(0, 3) == 0)
    pattern = str(rng.choice(PATTERNS))
    nfr = int(rng.integers(3, 7))
    args = ["--pattern", pattern]
    if rng.integers(0, 2):
        args.append("--prediction")
    if rng.integers(0, 3) == 0:
        lo = int(rng.integers(6, 11))
        args += ["--min-level", str(lo), "--max-level", str(int(rng.integers(lo, 13)))]
    args += ["-q", str(int(rng.choice([5, 20, 45, 90]))), "-z", str(int(rng.integers(0, 2))),
             "--rpf-mantissa", str(int(rng.integers(2, 9))), "--dc-rpf-mantissa", str(int(rng.integers(2, 9))),
             "--chroma-qfactor", str(float(rng.choice([1.0, 2.0, 3.5])))]
    w, h = (int(rng.integers(16, 65)) * 2 for _ in range(2))
    first = random_image(rng, colour, (w, h))
    shape = (h, w, 3) if colour else (h, w)
    a0 = np.frombuffer(first[len(first) - int(np.prod(shape)):], np.uint8).reshape(shape)
    frames = [first]
    for f in range(1, nfr):
        a = np.roll(a0, (int(rng.integers(-5, 6)) * f, int(rng.integers(-5, 6)) * f), (0, 1)).astype(np.int32)
        a = np.clip(a + rng.integers(-3, 4, a.shape), 0, 255).astype(np.uint8)
        frames.append((synth.ppm_bytes if colour else synth.pgm_bytes)(a))
    return frames, args


def manifest_names(manifest):
    """the multi-frame video cases of MANIFEST.json up to 256 pixels wide"""
    out = []
    for c in manifest["video_cases"]:
        if len(c["inputs"]) > 1 and all(manifest["inputs"][i]["args"]["w"] <= MAX_MANIFEST_WIDTH for i in c["inputs"]):
            out.append(c["name"])
    return out


def pinned_names(manifest):
    return manifest_names(manifest) + list(SYNTH_CASES) + ["seed%d" % s for s in PINNED_SEEDS]


def case_of(manifest, inputs, name):
    """-> (frames as PNM bytes, cfiasco arguments)"""
    if name in SYNTH_CASES:
        make, args = SYNTH_CASES[name]
        return make(), list(args)
    if name.startswith("seed"):
        return random_case(int(name[4:]))
    case = [c for c in manifest["video_cases"] if c["name"] == name][0]
    return [inputs.data(i) for i in case["inputs"]], list(case["args"])


def inputs_md5(frames):
    return hashlib.md5(b"".join(frames)).hexdigest()


def fixture():
    return json.load(open(FIXTURE))["cases"]


# ------------------------------------------------------------------ running the three programs

def geometry(frames):
    w, h = (int(v) for v in frames[0].split(b"\n", 2)[1].split())
    return w, h, 3 if frames[0][:2] == b"P6" else 1


def write_inputs(frames, tmp):
    os.makedirs(str(tmp), exist_ok=True)
    names = []
    for i, f in enumerate(frames):
        names.append(os.path.join(str(tmp), "in%02d.%s" % (i, "ppm" if f[:2] == b"P6" else "pgm")))
        open(names[-1], "wb").write(f)
    return names


def _read_planes(dirname, prefix, geom):
    """{display: (type, int16 array bands x h x w)} of the <prefix><display>_t<type>.i16 files of a directory"""
    w, h, nb = geom
    out = {}
    for fn in sorted(os.listdir(dirname)):
        if fn.startswith(prefix) and fn.endswith(".i16"):
            display, t = fn[len(prefix):-4].split("_t")
            a = np.fromfile(os.path.join(dirname, fn), np.int16)
            assert a.size == w * h * nb, (fn, a.size, geom)
            out[int(display)] = (int(t), a.reshape(nb, h, w))
    return out


def _read_counts(dirname):
    """{display: {"forward", "backward", "interpolated", "skipped", "levels": {level: (f, b, i)}}} of the d<n>.txt files"""
    out = {}
    for fn in os.listdir(dirname):
        if fn.startswith("d") and fn.endswith(".txt"):
            t = open(os.path.join(dirname, fn)).read().split()
            rec = {t[i]: int(t[i + 1]) for i in range(0, 12, 2)}
            rec["levels"] = {int(t[i + 1]): tuple(int(v) for v in t[i + 2:i + 5]) for i in range(12, len(t), 5)}
            assert rec["display"] == int(fn[1:-4]) and all(t[i] == "level" for i in range(12, len(t), 5)), t
            out[rec["display"]] = rec
    return out


def run_library(lib, frames, args, tmp):
    """fiasco_coder() of a library with the planes of every reconstructed frame written out
    -> (stream or None, {display: (type, planes)}, {display: counts}, error message)"""
    names = write_inputs(frames, tmp)
    dump = os.path.join(str(tmp), "dump_" + lib.core_name())
    os.makedirs(dump)
    q, o = options_from_args(lib, args)
    out = os.path.join(str(tmp), lib.core_name() + ".fco")
    old = os.environ.get("FIASCO_AMD_SEQ_RECONST_DIR")
    os.environ["FIASCO_AMD_SEQ_RECONST_DIR"] = dump
    try:
        rc = lib.fiasco_coder(names, out, q, o)
        msg = lib.error_message() if rc != 1 else ""
    finally:
        o.delete()
        if old is None:
            del os.environ["FIASCO_AMD_SEQ_RECONST_DIR"]
        else:
            os.environ["FIASCO_AMD_SEQ_RECONST_DIR"] = old
    if rc != 1:
        return None, {}, {}, msg
    return open(out, "rb").read(), _read_planes(dump, "d", geometry(frames)), _read_counts(dump), ""


def run_reference(exe, frames, args, tmp, dump=True):
    """the reference coder (cfiasco_ref, cfiasco_ref_recon) -> (None or why it wrote nothing, stream, {display: (type, planes)})"""
    names = write_inputs(frames, tmp)
    d = os.path.join(str(tmp), "dump_ref")
    os.makedirs(d, exist_ok=True)
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    env.pop("FIASCO_REF_RECONST_DIR", None)
    if dump:
        env["FIASCO_REF_RECONST_DIR"] = d
    out = os.path.join(str(tmp), "ref.fco")
    r = subprocess.run([exe, "--progress-meter", "0"] + args + ["-o", out] + names, env=env,
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    if r.returncode < 0 or r.returncode >= 128:
        return "crash (rc %d)" % r.returncode, None, {}
    if r.returncode != 0:
        return r.stderr.decode("latin-1").strip().split("\n")[-1], None, {}
    return None, open(out, "rb").read(), (_read_planes(d, "r", geometry(frames)) if dump else {})


def reference_decode(stream, nframes, geom, tmp):
    """dfiasco_ref -s 0 on a stream -> {display: uint8 pixels as write_image orders them}, or None where it dies"""
    w, h, nb = geom
    base = os.path.join(str(tmp), "dec")
    open(base + ".fco", "wb").write(stream)
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    r = subprocess.run([DFIASCO, "-s", "0", "-o", base + ".pnm", base + ".fco"], env=env, capture_output=True)
    if r.returncode != 0:
        return None
    out = {}
    for n in range(nframes):
        raw = open("%s.%0*d.pnm" % (base, len(str(nframes - 1)), n), "rb").read()
        a = np.frombuffer(raw[len(raw) - w * h * nb:], np.uint8)
        out[n] = a.reshape((h, w, 3) if nb == 3 else (h, w))
    return out


def where_differ(a, b):
    """bounding boxes of the samples in which two plane stacks differ, per band, as text ("" if equal)"""
    parts = []
    for band in range(a.shape[0]):
        ys, xs = np.nonzero(a[band] != b[band])
        if len(ys):
            d = np.abs(a[band].astype(np.int32) - b[band].astype(np.int32))
            parts.append("band %d: %d samples in x %d..%d y %d..%d, largest difference %d"
                         % (band, len(ys), xs.min(), xs.max(), ys.min(), ys.max(), int(d.max())))
    return "; ".join(parts)


def planes_md5(planes):
    return hashlib.md5(np.ascontiguousarray(planes, "<i2").tobytes()).hexdigest()


# ------------------------------------------------------------------ the checks both libraries go through

def check_against_fixture(name, rec, stream, planes, counts):
    """stream md5, the set of frames, their types, the md5 of every frame's planes; no block above p_max_level"""
    assert hashlib.md5(stream).hexdigest() == rec["stream_md5"] and len(stream) == rec["bytes"], name
    assert sorted(planes) == [f["display"] for f in rec["frames"]], (name, sorted(planes))
    assert sorted(counts) == sorted(planes), name
    bad = []
    for f in rec["frames"]:
        t, p = planes[f["display"]]
        assert t == f["type"], (name, f["display"], t)
        if planes_md5(p) != f["planes_md5"]:
            bad.append("frame %d (%s)" % (f["display"], "IPB"[t]))
        assert counts[f["display"]]["skipped"] == 0, (name, f["display"], counts[f["display"]])
        if t == 0:
            assert not counts[f["display"]]["levels"], (name, f["display"])
    assert not bad, "%s: planes differ from the reference coder's: %s" % (name, ", ".join(bad))


def check_not_hollow(runs):
    """over all pinned cases: at least 10 applied blocks of each type, at least 50 chroma samples at a clip bound in a
    P or B frame; no frame holds a block above p_max_level, and none can (reconst_cases.NONE_SKIPPED_CAN_EXIST)"""
    total = {"forward": 0, "backward": 0, "interpolated": 0, "skipped": 0}
    clipped = 0
    for rec, _, planes, counts in runs:
        for display, c in counts.items():
            for k in total:
                total[k] += c[k]
            t, p = planes[display]
            if t != 0 and p.shape[0] == 3:
                clipped += int(sum((p[1:] == b).sum() for b in CHROMA_CLIP))
    print("pinned cases: blocks applied %s, chroma samples at a clip bound in P / B frames %d" % (total, clipped))
    assert min(total["forward"], total["backward"], total["interpolated"]) >= 10, total
    assert clipped >= 50, clipped
    assert total["skipped"] == 0 and NONE_SKIPPED_CAN_EXIST, total


def compare_runs(what, stream, planes, other_stream, other_planes, whose):
    """the stream and every frame of a library against another coder's -> "" or the first difference: frame, type,
    band and bounding box"""
    if stream != other_stream:
        return "%s: the stream differs from %s" % (what, whose)
    if sorted(planes) != sorted(other_planes):
        return "%s: frames %s, %s has %s" % (what, sorted(planes), whose, sorted(other_planes))
    for d in sorted(planes):
        (t, p), (ot, op) = planes[d], other_planes[d]
        if t != ot or not np.array_equal(p, op):
            return "%s: frame %d type %s (%s: %s) differs from %s: %s" % (what, d, "IPB"[t], whose, "IPB"[ot], whose, where_differ(p, op))
    return ""


def fuzz_seed(lib, seed, tmp, yardstick=None):
    """One random case through `lib`: against the live reference coder where cfiasco_ref_recon is built, and against
    the library `yardstick` if one is given (streams as bytes, planes as int16 arrays).  A seed is left out only where
    both coders fail, or where the reference crashes or refuses.  -> ("compared" | "skipped" | "MISMATCH", text)"""
    frames, args = random_case(seed)
    what = "seed %d %s %s" % (seed, geometry(frames), " ".join(args))
    stream, planes, counts, msg = run_library(lib, frames, args, os.path.join(str(tmp), "lib%d" % seed))
    if stream is not None:
        if sorted(planes) != list(range(len(frames))):
            return "MISMATCH", "%s: %d frames, reconstructed %s" % (what, len(frames), sorted(planes))
        if any(c["skipped"] for c in counts.values()):
            return "MISMATCH", "%s: a frame holds a block above p_max_level" % what
    left_out = None
    if yardstick is not None:
        ystream, yplanes, _, ymsg = run_library(yardstick, frames, args, os.path.join(str(tmp), "yard%d" % seed))
        if stream is None and ystream is None:
            left_out = "%s: both fail: %s; %s: %s" % (what, msg, yardstick.core_name(), ymsg)
        elif stream is None or ystream is None:
            return "MISMATCH", "%s: one of the two fails: %r; %s: %r" % (what, msg, yardstick.core_name(), ymsg)
        else:
            bad = compare_runs(what, stream, planes, ystream, yplanes, yardstick.core_name())
            if bad:
                return "MISMATCH", bad
    if os.path.exists(CFIASCO_RECON):
        err, rstream, rplanes = run_reference(CFIASCO_RECON, frames, args, os.path.join(str(tmp), "ref%d" % seed))
        if err:
            if stream is None or err.startswith("crash") or any(m in err for m in REFERENCE_REFUSALS):
                return "skipped", "%s: reference: %s; library: %s" % (what, err, msg or "coded it")
            return "MISMATCH", "%s: the reference fails with %r, the library codes it" % (what, err)
        if stream is None:
            return "MISMATCH", "%s: the reference codes it, the library fails: %s" % (what, msg)
        bad = compare_runs(what, stream, planes, rstream, rplanes, "the reference coder")
        if bad:
            return "MISMATCH", bad
    if left_out:
        return "skipped", left_out
    return "compared", what


def run_fuzz(key, lib, tmp, seeds=FUZZ_SEEDS, yardstick=None):
    """every seed printed, a mismatch fails -> number compared"""
    res = [(s,) + fuzz_seed(lib, s, tmp, yardstick) for s in seeds]
    for s, verdict, text in res:
        print("reconst fuzz %s seed %d: %s %s" % (key, s, verdict, text))
    bad = [text for _, verdict, text in res if verdict == "MISMATCH"]
    assert not bad, "\n".join(bad)
    return sum(1 for _, verdict, _ in res if verdict == "compared")
