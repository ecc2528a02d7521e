"""Magnified decodes on the device (`dfiasco -m M'; include/libfiasco_amd_hip.h: fiasco_amd_batch_decode_device_magnified,
fiasco_amd_batch_decode_planes_magnified, fiasco_amd_batch_decode_device_thumbnails; csrc/hip/frame_decoder.inc): every
(case, M) the real reference decoded (tests/golden/DECODED_MAGNIFIED.json) gives its bytes through the device route and
through the host route, every (case, M) it refused is refused with nothing written, and the thumbnails of ONE decode
(dec_thumb_kernel) are those of separate decodes, over two flights of frames that differ in size."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import magnify_ref
import synth
from conftest import GOLDEN, REF_SHARE, ROOT, options_from_args
from pixels_ref import pixels_of_planes

pytestmark = pytest.mark.gpu

DFIASCO = os.path.join(ROOT, "oracle", "_ref", "dfiasco_ref")
CASES = sorted(magnify_ref.fixture_cases())


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


@pytest.fixture(scope="module")
def coded(gpu, inputs):
    """every fixture case as a finished batch of one frame, coded once: name -> (entry, batch, stream)"""
    out, opts = {}, []
    for name, ent in magnify_ref.fixture_cases().items():
        q, o = options_from_args(gpu, ent["args"])
        b = fiasco_amd.Batch(gpu, [magnify_ref.case_input(inputs, ent)], q, o)
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], (name, gpu.error_message())
        out[name] = (ent, b, stream)
        opts.append(o)
    yield out
    for _, b, _ in out.values():
        b.free()
    for o in opts:
        o.delete()


def pattern(*shape):
    """a tensor of bytes that no decoded frame looks like: what a call must leave alone is compared with it"""
    n = int(np.prod(shape))
    a = ((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8).reshape(shape)
    return torch.from_numpy(a).cuda()


def target(w, h, colour, layout="interleaved"):
    if not colour:
        return pattern(h, w)
    return pattern(h, w, 3) if layout == "interleaved" else pattern(3, h, w)


def as_pixels(t):
    """a target as the bytes of a PGM / PPM: H x W or H x W x 3"""
    a = t.cpu().numpy()
    return a.transpose(1, 2, 0) if a.ndim == 3 and a.shape[0] == 3 and a.shape[2] != 3 else a


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


# ------------------------------------------------------------------ 1. the reference's bytes, both routes

@pytest.mark.parametrize("name", CASES)
def test_device_route_gives_the_references_bytes(gpu, coded, name):
    ent, b, _ = coded[name]
    col = ent["color"]
    plain = target(ent["width"], ent["height"], col)
    assert b.decode_device([plain]) == 1, gpu.error_message()
    assert md5(as_pixels(plain)) == ent["magnified"]["0"]["md5"]
    pitched_at = min(m for m, _ in magnify_ref.accepted(ent))
    for m, rec in magnify_ref.accepted(ent):
        w, h = rec["width"], rec["height"]
        assert fiasco_amd.magnified_size(gpu, ent["width"], ent["height"], m) == (w, h)
        for layout in (("interleaved", "planar") if col else ("gray",)):
            t = target(w, h, col, layout)
            assert b.decode_device([t], magnify=m) == 1, (name, m, gpu.error_message())
            got = as_pixels(t)
            assert md5(got) == rec["md5"], (name, m, layout)
            if m == 0:
                assert np.array_equal(got, as_pixels(plain))           # the old entry's bytes
        if m == pitched_at:                                            # a frame cut out of a larger tensor
            big = pattern(h + 5, w + 9, 3) if col else pattern(h + 5, w + 9)
            before = big.clone()
            cut = big[3:3 + h, 7:7 + w]
            assert b.decode_device([cut], magnify=m) == 1, (name, m, gpu.error_message())
            assert md5(cut.cpu().numpy()) == rec["md5"], (name, m, "pitched")
            cut.copy_(before[3:3 + h, 7:7 + w])
            assert torch.equal(big, before), (name, m, "written outside the cut")


@pytest.mark.parametrize("name", CASES)
def test_host_route_gives_the_references_bytes(gpu, coded, name):
    ent, b, _ = coded[name]
    for m, rec in magnify_ref.accepted(ent):
        planes = b.decode_planes(0, magnify=m)
        assert planes.shape == (3 if ent["color"] else 1, rec["height"], rec["width"]), (name, m)
        assert md5(pixels_of_planes(planes if ent["color"] else planes[0])) == rec["md5"], (name, m)
        if m == 0:
            assert np.array_equal(planes, b.decode_planes(0))


@pytest.mark.parametrize("name", CASES)
def test_live_reference_decodes_what_the_device_coded(gpu, coded, name, tmp_path):
    """one comparison per case with the reference's decoder itself, where its binary travelled: the stream the device
    wrote, at the smallest magnification the case allows (its largest where that is 0)"""
    if not os.path.exists(DFIASCO):
        return
    ent, b, stream = coded[name]
    mags = [m for m, _ in magnify_ref.accepted(ent) if m]
    m = min(mags) if min(mags) < 0 else 1
    fco, dec = str(tmp_path / "dev.fco"), str(tmp_path / "dec.pnm")
    open(fco, "wb").write(stream)
    subprocess.check_call([DFIASCO, "-s", "0", "-m", str(m), "-o", dec, fco], env=dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE),
                          stderr=subprocess.DEVNULL)
    raw = open(dec, "rb").read()
    w, h = fiasco_amd.magnified_size(gpu, ent["width"], ent["height"], m)
    assert [int(v) for v in raw.split(b"\n", 2)[1].split()] == [w, h]
    t = target(w, h, ent["color"])
    assert b.decode_device([t], magnify=m) == 1, gpu.error_message()
    assert raw[len(raw) - t.numel():] == t.cpu().numpy().tobytes(), (name, m)


# ------------------------------------------------------------------ 2. the refusals write nothing

@pytest.mark.parametrize("name", CASES)
def test_refusals_of_the_reference_are_refused_with_nothing_written(gpu, coded, name):
    ent, b, _ = coded[name]
    w, h, col = ent["width"], ent["height"], ent["color"]
    for m, rec in magnify_ref.refused(ent):
        want = "%s value is %d." % (rec["refused"].capitalize(), rec["limit"])
        # whatever the target's size: the coded one, and the one the shifts alone would give
        for tw, th in ((w, h), ((w << m, h << m) if m > 0 else (max(w >> -m, 2), max(h >> -m, 2)))):
            t = target(tw, th, col)
            keep = t.clone()
            with pytest.raises(fiasco_amd.FiascoError) as e:
                b.decode_device([t], magnify=m)
            assert want in str(e.value), (name, m, str(e.value))
            torch.cuda.synchronize()
            assert torch.equal(t, keep), (name, m)
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_planes(0, magnify=m)
        assert want in str(e.value), (name, m)
    # a target of the coded size at a magnification the frame allows: refused, all three sizes named
    for m, rec in magnify_ref.accepted(ent):
        if not m:
            continue
        t = target(w, h, col)
        keep = t.clone()
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_device([t], magnify=m)
        said = str(e.value)
        assert "%d x %d pixels for a frame of %d x %d at magnification %d: %d x %d" % (w, h, w, h, m, rec["width"], rec["height"]) in said, said
        torch.cuda.synchronize()
        assert torch.equal(t, keep), (name, m)


def test_a_batch_is_refused_as_a_whole_where_one_frame_is(gpu, inputs):
    """64 x 32 allows no reduction: with such a frame in the batch -1 is refused for all, nothing written."""
    cases = magnify_ref.fixture_cases()
    o = gpu.cli_options()
    b = fiasco_amd.Batch(gpu, [magnify_ref.case_input(inputs, cases[n]) for n in ("g64x64_a", "g64x32")], 20.0, o)
    assert None not in b.encode()
    ts = [pattern(32, 32), pattern(16, 32)]
    keep = [t.clone() for t in ts]
    for call in (lambda: b.decode_device(ts, magnify=-1), lambda: b.decode_thumbnails(None, 1, ts)):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            call()
        assert "Minimum value is 0." in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_device([ts[0], None], magnify=-1)                     # ... target or not: the rule is the batch's
    assert "Minimum value is 0." in str(e.value)
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip(ts, keep))
    # the thumbnail of the frame that allows one, the other skipped
    assert b.decode_thumbnails(None, 1, [ts[0], None]) == 1, gpu.error_message()
    assert md5(ts[0].cpu().numpy()) == cases["g64x64_a"]["magnified"]["-1"]["md5"]
    b.free(); o.delete()


# ------------------------------------------------------------------ 3. one decode, the frame and its thumbnail

def separate(b, geoms, m):
    """every frame of the batch through decode_device at m -> list of numpy arrays"""
    ts = []
    for w, h, bands in geoms:
        tw, th = fiasco_amd.magnified_size(b.lib, w, h, m)
        ts.append(target(tw, th, bands == 3))
    assert b.decode_device(ts, magnify=m) == b.n, b.lib.error_message()
    return [t.cpu().numpy() for t in ts]


def test_thumbnails_of_two_flights_of_mixed_frames(gpu, inputs):
    """34 frames -- two flights --, 64 x 64 and 100 x 70 mixed, every one another picture: the full frames are those of
    decode_device, the thumbnails those of decode_device(magnify=-1); with and without full-size targets; a skipped
    thumbnail and a skipped frame are left alone."""
    cases = magnify_ref.fixture_cases()
    arrs = [synth.synth(100, 70, 200 + i) if i % 3 == 1 else synth.synth(64, 64, 100 + i) for i in range(34)]
    pnm = [synth.pgm_bytes(a) for a in arrs]
    pnm[0], pnm[1], pnm[33] = (magnify_ref.case_input(inputs, cases[n]) for n in ("g64x64_a", "g100x70", "g64x64_b"))
    o = gpu.cli_options()
    b = fiasco_amd.Batch(gpu, pnm, 20.0, o)
    streams = b.encode()
    assert None not in streams, gpu.error_message()
    assert len(set(streams)) == 34
    full, small = separate(b, b._geom, 0), separate(b, b._geom, -1)
    for i, n in ((0, "g64x64_a"), (1, "g100x70"), (33, "g64x64_b")):
        assert md5(full[i]) == cases[n]["magnified"]["0"]["md5"] and md5(small[i]) == cases[n]["magnified"]["-1"]["md5"], n
    assert small[1].shape == (36, 50) and small[0].shape == (32, 32)

    def fresh(m):
        return [target(*fiasco_amd.magnified_size(gpu, w, h, m), False) for w, h, _ in b._geom]

    # both
    ts, th = fresh(0), fresh(-1)
    assert b.decode_thumbnails(ts, 1, th) == 34, gpu.error_message()
    for i in range(34):
        assert np.array_equal(ts[i].cpu().numpy(), full[i]), i
        assert np.array_equal(th[i].cpu().numpy(), small[i]), i
    # the thumbnails alone
    th = fresh(-1)
    assert b.decode_thumbnails(None, 1, th) == 34, gpu.error_message()
    assert all(np.array_equal(th[i].cpu().numpy(), small[i]) for i in range(34))
    # frame 2 without a thumbnail, frame 5 without a full-size target, frame 32 (second flight) with neither
    ts, th = fresh(0), fresh(-1)
    keep_th2, keep_th32, keep_t5, keep_t32 = th[2].clone(), th[32].clone(), ts[5].clone(), ts[32].clone()
    assert b.decode_thumbnails([None if i in (5, 32) else t for i, t in enumerate(ts)], 1,
                               [None if i in (2, 32) else t for i, t in enumerate(th)]) == 33, gpu.error_message()
    torch.cuda.synchronize()
    assert torch.equal(th[2], keep_th2) and torch.equal(th[32], keep_th32) and torch.equal(ts[5], keep_t5) and torch.equal(ts[32], keep_t32)
    for i in range(34):
        assert i in (5, 32) or np.array_equal(ts[i].cpu().numpy(), full[i]), i
        assert i in (2, 32) or np.array_equal(th[i].cpu().numpy(), small[i]), i
    # a thumbnail of the wrong size, the coded one included: refused, nothing written
    ts, th = fresh(0), fresh(-1)
    th[6] = pattern(64, 64)
    keep = [t.clone() for t in ts + th]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_thumbnails(ts, 1, th)
    assert "<device target 6>: 64 x 64 pixels for a frame of 64 x 64 at magnification -1: 32 x 32" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip(ts + th, keep))
    b.free(); o.delete()


@pytest.mark.parametrize("name", ["c256", "c256sq"])
def test_colour_thumbnails_at_every_reduction(gpu, coded, name):
    ent, b, _ = coded[name]
    w, h = ent["width"], ent["height"]
    for reduce in (1, 2, 3):
        rec = ent["magnified"][str(-reduce)]
        if "md5" not in rec:                                           # c256 at -3: 192 >> 3 < 32
            t = pattern(max(h >> reduce, 2), max(w >> reduce, 2), 3)
            keep = t.clone()
            with pytest.raises(fiasco_amd.FiascoError) as e:
                b.decode_thumbnails(None, reduce, [t])
            assert "Minimum value is %d." % rec["limit"] in str(e.value)
            torch.cuda.synchronize()
            assert torch.equal(t, keep)
            continue
        for layout in ("interleaved", "planar"):
            t, th = target(w, h, True, layout), target(rec["width"], rec["height"], True, layout)
            assert b.decode_thumbnails([t], reduce, [th]) == 1, (name, reduce, gpu.error_message())
            assert md5(as_pixels(t)) == ent["magnified"]["0"]["md5"], (name, reduce, layout)
            assert md5(as_pixels(th)) == rec["md5"], (name, reduce, layout)


# ------------------------------------------------------------------ 4. blocks smaller than the reduction

def test_blocks_smaller_than_the_reduction_are_refused(gpu):
    """No option of cfiasco gives such a frame (noise, -q 99 and --optimize 1 leave linear combinations at level 6 and
    above in a frame large enough for -3); block levels 4 .. 6 through the options object do: white noise of 256 x 256
    at quality 99 has its largest linear combination at level 5.  -2 needs level 4 and works; -3 needs level 6: the
    reference would clamp the levels at 0 and pile blocks onto one pixel, this decoder refuses the frame, on every
    route, with nothing written."""
    a = np.random.default_rng(1).integers(0, 256, (256, 256)).astype(np.uint8)
    o = gpu.cli_options()
    o.set_optimizations(4, 6, 3, 10000, 0)
    b = fiasco_amd.Batch(gpu, [synth.pgm_bytes(a)], 99.0, o)
    assert b.encode()[0] is not None, gpu.error_message()
    full, th2 = pattern(256, 256), pattern(64, 64)
    assert b.decode_thumbnails([full], 2, [th2]) == 1, gpu.error_message()
    want2 = pattern(64, 64)
    assert b.decode_device([want2], magnify=-2) == 1, gpu.error_message()
    assert torch.equal(th2, want2)
    assert np.array_equal(pixels_of_planes(b.decode_planes(0, magnify=-2)[0]), want2.cpu().numpy())
    assert fiasco_amd.magnified_size(gpu, 256, 256, -3) == (32, 32)            # the size rule allows it
    t, th = pattern(256, 256), pattern(32, 32)
    keep_t, keep_th = t.clone(), th.clone()
    for call in (lambda: b.decode_device([th], magnify=-3), lambda: b.decode_thumbnails([t], 3, [th]),
                 lambda: b.decode_thumbnails(None, 3, [th]), lambda: b.decode_planes(0, magnify=-3)):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            call()
        assert "smaller than the reduction" in str(e.value), str(e.value)
    torch.cuda.synchronize()
    assert torch.equal(t, keep_t) and torch.equal(th, keep_th)
    b.free(); o.delete()


def test_a_reduction_down_to_level_zero(gpu, tmp_path):
    """The same noise at quality 20 keeps its largest linear combination at level 6: at -3 every block the frame shows
    is ONE pixel, the level-0 image -- the pixel table -- on both kernels' level-0 paths (the assembly of the decode at
    -3, the gather beside a full-size decode).  The reference's decoder agrees where its binary travelled."""
    a = np.random.default_rng(1).integers(0, 256, (256, 256)).astype(np.uint8)
    o = gpu.cli_options()
    o.set_optimizations(4, 6, 3, 10000, 0)
    b = fiasco_amd.Batch(gpu, [synth.pgm_bytes(a)], 20.0, o)
    stream = b.encode()[0]
    assert stream is not None, gpu.error_message()
    direct, th, full, plain = pattern(32, 32), pattern(32, 32), pattern(256, 256), pattern(256, 256)
    assert b.decode_device([direct], magnify=-3) == 1, gpu.error_message()
    assert b.decode_thumbnails([full], 3, [th]) == 1, gpu.error_message()
    assert b.decode_device([plain]) == 1
    assert torch.equal(th, direct) and torch.equal(full, plain) and not torch.equal(direct, pattern(32, 32))
    assert np.array_equal(pixels_of_planes(b.decode_planes(0, magnify=-3)[0]), direct.cpu().numpy())
    if os.path.exists(DFIASCO):
        fco, dec = str(tmp_path / "dev.fco"), str(tmp_path / "dec.pgm")
        open(fco, "wb").write(stream)
        subprocess.check_call([DFIASCO, "-s", "0", "-m", "-3", "-o", dec, fco], env=dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE),
                              stderr=subprocess.DEVNULL)
        raw = open(dec, "rb").read()
        assert raw[len(raw) - 32 * 32:] == direct.cpu().numpy().tobytes()
    b.free(); o.delete()
