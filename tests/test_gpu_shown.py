"""Magnified frames and thumbnails smoothed as `dfiasco' shows them (include/libfiasco_amd_display.h; csrc/hip/smooth.inc,
frame_decoder.inc), on the device: decode_shown against the bytes `dfiasco_ref -m M -s N' wrote
(tests/golden/DECODED_SHOWN.json) at every magnification the reference accepts; the same bytes from the unsmoothed magnified
planes smoothed in numpy along the library's list (independent of the smoothing kernels); frame and thumbnail from one
decode, both smoothed; the fused and the per-pass path on one flight of mixed sizes; the fused kernel alone; a frame the
library refuses beside frames it writes; refused calls write nothing; the live reference decoder."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import shown_ref
import smooth_ref
import synth
from conftest import GOLDEN, REF_SHARE, ROOT, options_from_args
from pixels_ref import pixels_of_planes

pytestmark = pytest.mark.gpu

DFIASCO = os.path.join(ROOT, "oracle", "_ref", "dfiasco_ref")
LEVELS = shown_ref.LEVELS


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pattern(*shape):
    """a tensor of bytes that no decoded frame looks like: what a call must leave alone is compared with it"""
    n = int(np.prod(shape))
    return to_gpu(((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8).reshape(shape))


def target(w, h, bands, layout="interleaved"):
    return pattern(h, w) if bands == 1 else pattern(h, w, 3) if layout == "interleaved" else pattern(3, h, w)


def as_pixels(t):
    a = t.cpu().numpy()
    return a.transpose(1, 2, 0) if a.ndim == 3 and a.shape[0] == 3 and a.shape[2] != 3 else a


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def pixels(planes):
    return pixels_of_planes(planes[0] if planes.shape[0] == 1 else planes)


@pytest.fixture(scope="module")
def coded(gpu, inputs):
    """per fixture case: the frame coded on the device, as a finished batch of one; computed once and left alone"""
    out, keep = {}, []
    for name, ent in shown_ref.fixture_cases().items():
        b, o = shown_ref.staged(gpu, inputs, ent)
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], (name, gpu.error_message())
        out[name] = (ent, b)
        keep.append(o)
    yield out
    for ent, b in out.values():
        b.free()
    for o in keep:
        o.delete()


# ------------------------------------------------------------------ 1. the reference's bytes

@pytest.mark.parametrize("name", sorted(shown_ref.fixture_cases()))
def test_decode_shown_gives_the_references_bytes(gpu, coded, name):
    ent, b = coded[name]
    bands = 3 if ent["color"] else 1
    seen = 0
    for m, rec in shown_ref.accepted(ent):
        w, h = rec["width"], rec["height"]
        if (name, m) in shown_ref.LIBRARY_REFUSES:
            t = target(w, h, bands)
            keep = t.clone()
            with pytest.raises(fiasco_amd.FiascoError) as e:
                b.decode_shown([t], magnify=m, smoothing=70)
            assert "<device target 0>" in str(e.value) and "magnification %d" % m in str(e.value) and "falls to level" in str(e.value)
            assert torch.equal(t, keep)
            t = target(w, h, bands)
            assert b.decode_shown([t], magnify=m, smoothing=0) == 1 and md5(as_pixels(t)) == rec["md5"]["0"]      # unsmoothed: decoded
            continue
        for n in LEVELS + (0,):
            t = target(w, h, bands)
            assert b.decode_shown([t], magnify=m, smoothing=n) == 1, (name, m, n, gpu.error_message())
            assert md5(as_pixels(t)) == rec["md5"][str(n)], (name, m, n)
            seen += 1
        t = target(w, h, bands, "planar")                               # the defaults: what plain `dfiasco -m M -o' writes
        if m:
            assert b.decode_shown([t], magnify=m) == 1 and md5(as_pixels(t)) == rec["md5"]["-1"], (name, m)
        else:
            assert b.decode_shown([t]) == 1 and md5(as_pixels(t)) == rec["md5"]["-1"], name
    assert seen >= 12
    # what the size rule refuses is refused with its message, nothing written
    for m, rec in shown_ref.refused(ent):
        t = target(ent["width"], ent["height"], bands)
        keep = t.clone()
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_shown([t], magnify=m)
        assert "value is %d." % rec["limit"] in str(e.value) and torch.equal(t, keep), (name, m)


@pytest.mark.parametrize("name", sorted(shown_ref.fixture_cases()))
def test_numpy_smoothing_of_the_magnified_planes_gives_the_same_bytes(gpu, coded, name):
    """independent of the smoothing kernels: decode_planes(magnify=M) is the unsmoothed decoder, the blend is numpy's"""
    ent, b = coded[name]
    for m, rec in shown_ref.accepted(ent):
        if (name, m) in shown_ref.LIBRARY_REFUSES:
            continue
        planes = b.decode_planes(0, magnify=m)
        assert planes.shape[1:] == (rec["height"], rec["width"]) and md5(pixels(planes)) == rec["md5"]["0"], (name, m)
        borders = b.smoothing_borders(0, magnify=m)
        for n in (35, 70):
            assert md5(pixels(smooth_ref.smooth_planes(planes, borders, n))) == rec["md5"][str(n)], (name, m, n)


# ------------------------------------------------------------------ 2. thumbnails

@pytest.mark.parametrize("name", ["g256_q60", "c256sq", "c256", "g100x70", "g130x66", "carry74_a", "g100x70_s35", "g256_z1_q300"])
def test_frame_and_thumbnail_from_one_decode_are_both_smoothed(gpu, coded, name):
    ent, b = coded[name]
    bands = 3 if ent["color"] else 1
    full = ent["shown"]["0"]
    done = 0
    for reduce in (1, 2, 3):
        rec = ent["shown"][str(-reduce)]
        if "md5" not in rec:
            continue
        if (name, -reduce) in shown_ref.LIBRARY_REFUSES:
            # the thumbnail cannot be smoothed: the frame fails alone, neither of its targets is written
            t, small = target(ent["width"], ent["height"], bands), target(rec["width"], rec["height"], bands)
            kt, ks = t.clone(), small.clone()
            with pytest.raises(fiasco_amd.FiascoError) as e:
                b.decode_thumbnails([t], reduce, [small], smoothing=70)
            assert "falls to level" in str(e.value) and torch.equal(t, kt) and torch.equal(small, ks)
            continue
        for n in LEVELS:
            t, small = target(ent["width"], ent["height"], bands), target(rec["width"], rec["height"], bands)
            assert b.decode_thumbnails([t], reduce, [small], smoothing=n) == 1, (name, reduce, n, gpu.error_message())
            assert md5(as_pixels(t)) == full["md5"][str(n)] and md5(as_pixels(small)) == rec["md5"][str(n)], (name, reduce, n)
            done += 1
        # the same bytes as the two calls that give one of them each; the thumbnail alone
        t, small = target(ent["width"], ent["height"], bands), target(rec["width"], rec["height"], bands)
        one, two = target(ent["width"], ent["height"], bands), target(rec["width"], rec["height"], bands)
        assert b.decode_thumbnails([t], reduce, [small], smoothing=70) == 1
        assert b.decode_device([one], smoothing=70) == 1 and b.decode_shown([two], magnify=-reduce, smoothing=70) == 1
        assert torch.equal(t, one) and torch.equal(small, two), (name, reduce)
        alone = target(rec["width"], rec["height"], bands)
        assert b.decode_thumbnails(None, reduce, [alone], smoothing=70) == 1 and torch.equal(alone, two), (name, reduce)
        # smoothing 0 stays the unsmoothed entry's
        t, small = target(ent["width"], ent["height"], bands), target(rec["width"], rec["height"], bands)
        assert b.decode_thumbnails([t], reduce, [small]) == 1
        assert md5(as_pixels(t)) == full["md5"]["0"] and md5(as_pixels(small)) == rec["md5"]["0"], (name, reduce)
    assert done >= 3


# ------------------------------------------------------------------ 3. the two paths

def test_fused_and_per_pass_paths_write_identical_bytes(gpu):
    """tests/gpu_shown_paths.py in two child processes, the developer switch forcing one path each: a flight that mixes
    four sizes at three magnifications and as thumbnails.  The policy itself (this process) agrees with both."""
    outs = {}
    for forced in ("0", "1"):
        env = dict(os.environ, FIASCO_AMD_DEBUG="1", FIASCO_AMD_SMOOTH_FUSED=forced)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_shown_paths.py")], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[forced] = json.loads(r.stdout.strip().splitlines()[-1])
        assert outs[forced]["switch"] == forced
    a, c = outs["0"], outs["1"]
    assert a["shown"] == c["shown"] and a["thumbs"] == c["thumbs"] and a["pairs"] == c["pairs"]
    assert len(a["shown"]["0"]) == 34 and len(set(a["shown"]["0"])) == 34
    # and the policy's own choice, in this process, writes the same bytes
    import gpu_shown_paths
    o = gpu.cli_options()
    arrs = gpu_shown_paths.frames()
    b = fiasco_amd.Batch(gpu, [synth.pgm_bytes(x) for x in arrs], 20.0, o)
    assert None not in b.encode(), gpu.error_message()
    for m in gpu_shown_paths.MAGS:
        ts = [pattern(h, w) for w, h in (fiasco_amd.magnified_size(gpu, w, h, m) for w, h, _ in b._geom)]
        assert b.decode_shown(ts, magnify=m, smoothing=70) == 34, gpu.error_message()
        assert [md5(as_pixels(t)) for t in ts] == a["shown"][str(m)], m
    b.free(); o.delete()


@pytest.mark.parametrize("name,m", [("noise256", 1), ("noise256", -3), ("g130x66", -1), ("g100x70", 3), ("carry74_a", -1), ("c256sq", -3)])
def test_fused_kernel_alone_equals_numpy_on_a_magnified_plane(gpu, coded, name, m):
    ent, b = coded[name]
    planes = b.decode_planes(0, magnify=m)
    borders = b.smoothing_borders(0, magnify=m)
    for n in (35, 70, 100):
        want = smooth_ref.smooth_planes(planes, borders, n)
        d = to_gpu(planes)
        fiasco_amd.smooth_planes_device(gpu, d if planes.shape[0] == 3 else d[0], borders, n, fused=True)
        assert np.array_equal(d.cpu().numpy(), want), (name, m, n)
        d = to_gpu(planes)
        fiasco_amd.smooth_planes_device(gpu, d if planes.shape[0] == 3 else d[0], borders, n)
        assert np.array_equal(d.cpu().numpy(), want), (name, m, n)
    assert not np.array_equal(want, planes)
    # nothing to do, and a refused list: nothing written
    d = to_gpu(planes)
    fiasco_amd.smooth_planes_device(gpu, d if planes.shape[0] == 3 else d[0], [], 70, fused=True)
    fiasco_amd.smooth_planes_device(gpu, d if planes.shape[0] == 3 else d[0], borders, 0, fused=True)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.smooth_planes_device(gpu, d if planes.shape[0] == 3 else d[0], borders + [(0, planes.shape[1], 1, 1, borders[-1][4] + 1)], 70, fused=True)
    assert "outside the plane" in str(e.value) and np.array_equal(d.cpu().numpy(), planes)


# ------------------------------------------------------------------ 4. a frame that is refused beside frames that are written

def test_refused_frame_fails_alone_and_refused_calls_write_nothing(gpu, inputs):
    ent = shown_ref.fixture_cases()["g256_z1_q300"]
    q, o = options_from_args(gpu, ent["args"])
    y, x = np.mgrid[0:256, 0:256]
    ramp, diag = x.astype(np.uint8), ((x + y) // 2).astype(np.uint8)
    b = fiasco_amd.Batch(gpu, [synth.pgm_bytes(ramp), inputs.data("g256"), synth.pgm_bytes(diag)], q, o)
    assert None not in b.encode(), gpu.error_message()
    ts = [pattern(32, 32) for _ in range(3)]
    keep = ts[1].clone()
    assert b.decode_shown(ts, magnify=-3, smoothing=70) == 2
    msg = gpu.error_message()
    assert "<device target 1>" in msg and "magnification -3" in msg and "level 5 falls to level -1" in msg and "undefined" in msg, msg
    assert torch.equal(ts[1], keep)
    for i in (0, 2):
        planes = b.decode_planes(i, magnify=-3)
        borders = b.smoothing_borders(i, magnify=-3)
        want = pixels(smooth_ref.smooth_planes(planes, borders, 70))
        assert np.array_equal(as_pixels(ts[i]), want) and not np.array_equal(want, pixels(planes)), i
    # at -2 all three are written
    ts = [pattern(64, 64) for _ in range(3)]
    assert b.decode_shown(ts, magnify=-2, smoothing=70) == 3, gpu.error_message()
    assert md5(as_pixels(ts[1])) == ent["shown"]["-2"]["md5"]["70"]
    # thumbnails at 3: frame 1 fails alone, frame and thumbnail
    full, small = [pattern(256, 256) for _ in range(3)], [pattern(32, 32) for _ in range(3)]
    kf, ks = full[1].clone(), small[1].clone()
    assert b.decode_thumbnails(full, 3, small, smoothing=70) == 2
    assert "<device target 1>" in gpu.error_message() and torch.equal(full[1], kf) and torch.equal(small[1], ks)
    assert not torch.equal(full[0], kf) and not torch.equal(small[2], ks)
    # refused calls: every target untouched
    ts = [pattern(64, 64), pattern(64, 64), pattern(32, 32)]
    keeps = [t.clone() for t in ts]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_shown(ts, magnify=-2, smoothing=70)                    # the last target has another size
    assert "<device target 2>" in str(e.value) and all(torch.equal(t, k) for t, k in zip(ts, keeps))
    for bad in (-2, 101):
        with pytest.raises(fiasco_amd.FiascoError):
            b.decode_shown(ts[:2] + [pattern(64, 64)], magnify=-2, smoothing=bad)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_shown(ts, magnify=-4)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_device(ts, magnify=-2, smoothing=70)                   # decode_device keeps refusing the pair
    assert all(torch.equal(t, k) for t, k in zip(ts, keeps))
    b.free(); o.delete()


# ------------------------------------------------------------------ 5. the live reference

def test_live_reference_decoder_shows_the_same_bytes(gpu, tmp_path):
    if not os.path.exists(DFIASCO):
        pytest.skip("the reference's binaries did not travel (oracle/ref_build.sh builds them in the build container)")
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    frames = [synth.noise(100, 70, 7), np.random.default_rng(3).integers(0, 256, (64, 96, 3)).astype(np.uint8)]
    o = gpu.cli_options()
    b = fiasco_amd.Batch.from_device(gpu, [to_gpu(a) for a in frames], 20.0, o)
    streams = b.encode()
    assert None not in streams, gpu.error_message()
    for m in (-1, 1):
        ts = [target(*fiasco_amd.magnified_size(gpu, w, h, m), bands) for w, h, bands in b._geom]
        assert b.decode_shown(ts, magnify=m) == 2, gpu.error_message()
        for i, a in enumerate(frames):
            fco, dec = str(tmp_path / ("l%d.fco" % i)), str(tmp_path / ("l%d_%d.pnm" % (i, m)))
            open(fco, "wb").write(streams[i])
            subprocess.check_call([DFIASCO, "-m", str(m), "-o", dec, fco], env=env, stderr=subprocess.DEVNULL)
            raw = open(dec, "rb").read()
            got = as_pixels(ts[i])
            assert raw[:2] == (b"P6" if a.ndim == 3 else b"P5")
            assert raw[len(raw) - got.size:] == got.tobytes(), (i, m)
        plain = [target(*fiasco_amd.magnified_size(gpu, w, h, m), bands) for w, h, bands in b._geom]
        assert b.decode_device(plain, magnify=m) == 2
        assert all(not torch.equal(p, t) for p, t in zip(plain, ts))   # the smoothing changed something
    b.free(); o.delete()
