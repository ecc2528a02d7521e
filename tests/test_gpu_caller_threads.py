"""The threading contract of the library on the device (-m gpu): calls on distinct batch, sequence and options objects
from several host threads at once (include/libfiasco_amd_hip.h "Threading", csrc/hip/shares.inc).  What such calls share
is the DevState of a device share -- slab pool, counters, the once-guard of the log2 table (csrc/hip/dev_state.h) --;
tests/dev_state_check.cpp is the race detector for that code, on the CPU under the sanitizers.  The tests here pin what
an integrator sees: every caller gets the reference's bytes, and the counters add up exactly.

Every expected value is the real reference's: streams and md5s of MANIFEST.json, decoded bytes of DECODED_OPTIONS.json,
reconstructed planes of RECONST.json.  Callers are Python threads released by one barrier (ctypes drops the GIL for the
length of a call); every thread has its own options, batches and sequences; frames are at most 256 x 256 and the
workgroups of all calls together a fraction of what the chip holds at once, so that residency is not what is tested.
A thread that does not come back within the time limit ends the session: nothing more is started on the device."""
import hashlib
import os
import subprocess
import sys
import threading
import time
import traceback

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import decoder_cases as dc
import reconst_cases as rc
import synth
from conftest import GOLDEN, ROOT, encode_case, options_from_args
from distortion_ref import distortion_of_bytes, reference_of_batch

pytestmark = pytest.mark.gpu

JOIN_SECONDS = 120
HUNG = []                   # callers that did not come back: nothing touches the device after that, not even a clean-up


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def run_callers(bodies):
    """every body on a thread of its own, all released by one barrier; the first exception of a caller fails the test
    with its traceback; a caller that is still inside the library after JOIN_SECONDS ends the session"""
    barrier = threading.Barrier(len(bodies))
    failed = [None] * len(bodies)

    def caller(i):
        try:
            barrier.wait(timeout=60)
            bodies[i]()
        except BaseException:
            failed[i] = traceback.format_exc()

    threads = [threading.Thread(target=caller, args=(i,), daemon=True) for i in range(len(bodies))]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_SECONDS
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    hung = [i for i, t in enumerate(threads) if t.is_alive()]
    if hung:
        HUNG.extend(hung)
        pytest.exit("caller threads %s did not come back within %d s: nothing more is started on the device" % (hung, JOIN_SECONDS), 1)
    bad = ["caller %d:\n%s" % (i, f) for i, f in enumerate(failed) if f]
    assert not bad, "\n".join(bad)


def still(manifest, inputs, name):
    """a golden still of MANIFEST.json "cases" -> (PNM bytes, cfiasco arguments, the case)"""
    case = [c for c in manifest["cases"] + manifest["video_cases"] if c["name"] == name][0]
    assert len(case["inputs"]) == 1
    return inputs.data(case["inputs"][0]), case["args"], case


def is_golden(stream, case):
    """the reference's stream of the case: its committed file where there is one, its md5 and length always"""
    if stream is None or len(stream) != case["bytes"] or hashlib.md5(stream).hexdigest() != case["md5"]:
        return False
    return not case.get("file") or stream == open(os.path.join(GOLDEN, case["file"]), "rb").read()


def array_of(pnm):
    """the pixels of raw PGM / PPM bytes: H x W or H x W x 3"""
    w, h, bands = fiasco_amd._pnm_geometry(pnm)
    a = np.frombuffer(pnm[len(pnm) - w * h * bands:], dtype=np.uint8).copy()
    return a.reshape((h, w) if bands == 1 else (h, w, 3))


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ 1. first use of a process, from two threads

CHILD = r"""
import hashlib, os, sys, threading
sys.path.insert(0, %r)
import fiasco_amd
lib = fiasco_amd.library(); lib.set_verbosity(0)
src = open(%r, 'rb').read()
barrier = threading.Barrier(2)
res = [None, None]
def caller(i):
    try:
        o = lib.cli_options()                       # its own options
        barrier.wait(timeout=60)
        out = lib.encode_batch([src], 20.0, o)[0]
        res[i] = (hashlib.md5(out).hexdigest() if out else 'NONE') + ' | ' + lib.error_message()
        o.delete()
    except BaseException as e:
        res[i] = 'EXCEPTION ' + repr(e)
threads = [threading.Thread(target=caller, args=(i,), daemon=True) for i in range(2)]
for t in threads: t.start()
for t in threads: t.join(240)
if any(t.is_alive() for t in threads):
    print('HUNG'); sys.stdout.flush(); os._exit(3)
for r in res: print('RESULT', r)
"""


def test_first_use_from_two_threads_builds_the_log2_table_once(gpu, manifest, tmp_path):
    """Two threads of a fresh process, behind a barrier, each encode g256.pgm with an empty private cache directory:
    the log2 correction table is built (a comparison of about 10^9 arguments on the device) by whoever comes first, the
    other waits for it -- both streams are the reference's g256_q20, one cache file is written.  (Before the once-guard
    the second caller met "an earlier attempt on this device failed" and lost its frame.)  A second process, which
    finds the cache file, gives the same."""
    good = [c for c in manifest["cases"] if c["name"] == "g256_q20"][0]["md5"]
    code = CHILD % (ROOT, os.path.join(GOLDEN, "g256.pgm"))
    cache = tmp_path / "cache"
    cache.mkdir()
    for what in ("cache empty", "cache present"):
        t0 = time.monotonic()
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, FIASCO_AMD_CACHE=str(cache)),
                           capture_output=True, text=True, timeout=300)
        print("first use, %s: %.1f s" % (what, time.monotonic() - t0))
        lines = [l for l in r.stdout.splitlines() if l.startswith("RESULT")]
        assert r.returncode == 0 and len(lines) == 2, (what, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
        assert all(l.split()[1] == good for l in lines), (what, lines)
        files = list(cache.glob("*"))
        assert len(files) == 1 and files[0].name.startswith("fiasco_amd_log2_") and files[0].name.endswith(".bin"), (what, files)


# ------------------------------------------------------------------ 2. four callers, stills

# caller -> its rounds: (cfiasco arguments, golden cases of one encode_batch call).  Callers 0, 1 and 2 code 256 x 256 gray
# frames at the default block levels: their slabs have one size, so what one releases the other acquires.
STILL_ROUNDS = [
    [([], ["g256_q20", "g160x120_q20", "g256_q20"])] * 3,
    [([], ["c256_q20", "g256_q20"])] * 3,
    [(["-q", "5"], ["g256_q5", "g256_q5", "g256_q5"])] * 3,
    [(["-z", "1"], ["n128x96_z1", "n128x96_z1"]), (["-z", "2"], ["g256_z2", "g256_z2"]), (["-z", "1"], ["n128x96_z1", "n128x96_z1"])],
]


@pytest.mark.parametrize("policy", ["one_workgroup_per_frame", "launcher"])
def test_four_callers_code_golden_stills(gpu, manifest, inputs, monkeypatch, policy):
    """Four threads, three rounds of fiasco_amd_encode_batch each on two to four golden stills under the golden's own
    options: every stream is the reference's, and the counters of the launches account for every frame submitted,
    exactly.  Once with one workgroup per frame (FIASCO_AMD_SPEC=0: the host state is all the calls share) and once
    under the launcher's own policy (speculating and cooperating builds; every wait between the workgroups of a frame
    is bounded: fc_serial.inc SPEC_TIMEOUT_TICKS, fc_spec.inc tab_wait, fc_append.inc wait_ticks, FcCoop.done_ticks)."""
    if policy == "one_workgroup_per_frame":
        monkeypatch.setenv("FIASCO_AMD_DEBUG", "1")
        monkeypatch.setenv("FIASCO_AMD_SPEC", "0")
    names = sorted({n for rounds in STILL_ROUNDS for _, group in rounds for n in group})
    stills = {n: still(manifest, inputs, n) for n in names}             # materialised before the threads start
    got = [[None] * len(rounds) for rounds in STILL_ROUNDS]

    def caller(k):
        def body():
            for r, (args, group) in enumerate(STILL_ROUNDS[k]):
                assert all(stills[n][1] == args for n in group)
                q, o = options_from_args(gpu, args)
                got[k][r] = gpu.encode_batch([stills[n][0] for n in group], q, o)
                o.delete()
        return body

    gpu.reset_stats()
    t0 = time.monotonic()
    run_callers([caller(k) for k in range(len(STILL_ROUNDS))])
    print("four callers, %s: %.2f s" % (policy, time.monotonic() - t0))
    st = gpu.get_stats()
    submitted = 0
    for k, rounds in enumerate(STILL_ROUNDS):
        for r, (_, group) in enumerate(rounds):
            submitted += len(group)
            for i, n in enumerate(group):
                assert is_golden(got[k][r][i], stills[n][2]), (policy, "caller %d round %d frame %d" % (k, r, i), n)
    print("frames_by_build %s spec_frames %d reencodes %d launches %d" % (list(st.frames_by_build), st.spec_frames, st.reencodes, st.launches))
    assert submitted == 30 and st.frames == submitted
    assert sum(st.frames_by_build) + st.spec_frames == submitted
    if policy == "one_workgroup_per_frame":
        assert st.spec_frames == 0


# ------------------------------------------------------------------ 3. different entries at once

def test_different_entries_at_once(gpu, manifest, inputs, tmp_path):
    """Four threads, four kinds of call: fiasco_amd_encode_batch; a staged batch that is coded, decoded into device
    memory and measured there; fiasco_coder() on two videos; a batch staged from device memory whose inputs are replaced
    there.  Each checks its results against its fixture.  The decoding callers run once alone first: together, the
    decoder's counters are the sum of what each of them decoded alone."""
    dec = dc.fixture()
    a_stills = [still(manifest, inputs, n) for n in ("g256_q20", "g160x120_q20")]
    b_stills = [still(manifest, inputs, n) for n in ("pred_g256", "pred_n128x96")]
    d_stills = [still(manifest, inputs, n) for n in ("g256_q20", "g160x120_q20")]
    videos = [c for c in manifest["video_cases"] if c["name"] in ("seq2_gray_ip", "seq4_gray_ibbp")]
    assert [c["name"] for c in videos] == ["seq2_gray_ip", "seq4_gray_ibbp"]
    for c in videos:
        for n in c["inputs"]:
            inputs.path(n)                          # written before the threads start
    kept = []                                       # caller B's finished batches, for the host outlets afterwards

    def caller_a():
        q, o = options_from_args(gpu, [])
        out = gpu.encode_batch([s[0] for s in a_stills], q, o)
        o.delete()
        assert all(is_golden(s, c[2]) for s, c in zip(out, a_stills)), "encode_batch"

    def caller_b():
        q, o = options_from_args(gpu, ["--prediction"])
        assert all(s[1] == ["--prediction"] for s in b_stills)
        b = fiasco_amd.Batch(gpu, [s[0] for s in b_stills], q, o)
        out = b.encode()
        assert all(is_golden(s, c[2]) for s, c in zip(out, b_stills)), "staged batch"
        targets = [torch.zeros((h, w), dtype=torch.uint8, device="cuda") for w, h, _ in b._geom]
        assert b.decode_device(targets) == b.n
        pixels = [t.cpu().numpy() for t in targets]
        for p, c in zip(pixels, b_stills):
            assert hashlib.md5(p.tobytes()).hexdigest() == dec[c[2]["name"]]["decoded_md5"], c[2]["name"]
        good, sse, maxdiff, _ = b.decode_distortion_device()
        assert good == b.n
        # gray: the bytes compared are the picture's own and the decoded ones (tests/distortion_ref.py)
        want = [distortion_of_bytes(array_of(c[0]), p) for c, p in zip(b_stills, pixels)]
        assert (sse, maxdiff) == ([w[0] for w in want], [w[1] for w in want])
        kept.append((b, o, sse, maxdiff))

    def caller_c(tmp):
        def body():
            os.makedirs(tmp, exist_ok=True)
            for case in videos:
                assert is_golden(encode_case(gpu, case, inputs, tmp), case), (case["name"], gpu.error_message())
        return body

    def caller_d():
        q, o = options_from_args(gpu, [])
        first = [to_gpu(array_of(s[0])) for s in d_stills]
        b = fiasco_amd.Batch.from_device(gpu, first, q, o)
        assert all(is_golden(s, c[2]) for s, c in zip(b.encode(), d_stills)), "batch from device memory"
        other = [to_gpu(synth.synth(w, h, 4242 + i)) for i, (w, h, _) in enumerate(b._geom)]
        b.upload_device(other)                      # other pictures ...
        out = b.encode()
        assert None not in out and not any(is_golden(s, c[2]) for s, c in zip(out, d_stills))
        b.upload_device([to_gpu(array_of(s[0])) for s in d_stills])     # ... and the golden ones again, from other memory
        assert all(is_golden(s, c[2]) for s, c in zip(b.encode(), d_stills)), "replaced inputs"
        b.free(); o.delete()

    def release():
        for b, o, _, _ in kept:
            b.free(); o.delete()
        del kept[:]

    alone = []
    for body in (caller_b, caller_c(str(tmp_path / "alone"))):
        gpu.reset_stats()
        body()
        st = gpu.get_stats()
        alone.append((st.decoder_frames, st.decoder_bytes))
    release()
    assert alone[0][0] == 4 and alone[1][0] >= 2         # B: two frames twice; C: at least the I frames its P and B frames refer to

    gpu.reset_stats()
    t0 = time.monotonic()
    run_callers([caller_a, caller_b, caller_c(str(tmp_path / "together")), caller_d])
    print("different entries at once: %.2f s" % (time.monotonic() - t0))
    st = gpu.get_stats()
    print("decoder: %d frames, %d bytes; alone %s" % (st.decoder_frames, st.decoder_bytes, alone))
    assert (st.decoder_frames, st.decoder_bytes) == (alone[0][0] + alone[1][0], alone[0][1] + alone[1][1])
    # caller B's integers once more, against the batch's own host outlets as tests/test_gpu_device_distortion.py does
    (b, _, sse, maxdiff), = kept
    refs = [reference_of_batch(b, i) for i in range(b.n)]
    release()
    assert (sse, maxdiff) == ([r[0] for r in refs], [r[1] for r in refs])


# ------------------------------------------------------------------ 4. two shares on one GPU, several callers

def test_two_shares_on_one_gpu_from_several_callers(gpu, manifest, inputs):
    """Device 0 listed twice.  Caller A's six stills use both shares and share 1's worker thread; caller B's one still
    is a single part on its calling thread; caller C's video has several groups of pictures, dealt by their key: a call
    of the sequence engine whose only part lies on share 1 runs on C's thread, on the DevState that worker 1 uses for A.
    Streams against MANIFEST.json, C's reconstructed frames against RECONST.json."""
    six = [still(manifest, inputs, n) for n in ("g256_q20", "g160x120_q20", "g96x64_q20", "g100x70_q20", "g64x32_q20", "g256_q20")]
    one = still(manifest, inputs, "g256_q20")
    assert all(s[1] == [] for s in six)
    frames, args = rc.case_of(manifest, inputs, "gops_ippi")
    rec = rc.fixture()["gops_ippi"]
    assert rc.inputs_md5(frames) == rec["inputs_md5"] and args == rec["args"]

    def caller_a():
        q, o = options_from_args(gpu, [])
        out = gpu.encode_batch([s[0] for s in six], q, o)
        o.delete()
        assert [is_golden(s, c[2]) for s, c in zip(out, six)] == [True] * 6, gpu.error_message()

    def caller_b():
        q, o = options_from_args(gpu, [])
        out = gpu.encode_batch([one[0]], q, o)
        o.delete()
        assert is_golden(out[0], one[2]), gpu.error_message()

    def caller_c():
        q, o = options_from_args(gpu, args)
        seq = fiasco_amd.Sequence(gpu, frames, q, o)
        try:
            assert seq.gops >= 2
            seq.keep_reconstructed()
            stream = seq.encode()
            assert hashlib.md5(stream).hexdigest() == rec["stream_md5"] and len(stream) == rec["bytes"]
            assert [f["display"] for f in rec["frames"]] == list(range(len(frames)))
            for f in rec["frames"]:
                planes, t = seq.reconstructed_planes(f["display"])
                assert t == f["type"] and rc.planes_md5(planes) == f["planes_md5"], "frame %d" % f["display"]
        finally:
            seq.free(); o.delete()

    try:
        gpu.set_devices([0, 0])
        assert gpu.device_count() == 2
        t0 = time.monotonic()
        run_callers([caller_a, caller_b, caller_c])
        print("two shares, three callers: %.2f s" % (time.monotonic() - t0))
    finally:
        if not HUNG:
            gpu.set_devices([])
