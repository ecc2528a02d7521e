"""Decoded frames smoothed along their partition borders on the device (include/libfiasco_amd_smooth.h:
fiasco_amd_batch_decode_device_smoothed, fiasco_amd_batch_decode_distortion_device_smoothed,
fiasco_amd_smooth_planes_device; csrc/hip/smooth.inc), on the device: the kernel alone against the numpy restatement
(tests/smooth_ref.py) over the whole domain of its arithmetic and at the edges of its geometry; the batch entries against
the bytes `dfiasco_ref -s N' wrote (tests/golden/DECODED_SMOOTH.json), PNM-fed and device-fed; two flights of mixed
colour frames, repeated; the distortion of the smoothed frame; that the unsmoothed outlets did not move; the live
reference decoder on the device's own streams."""
import ctypes
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import smooth_ref
import synth
from conftest import GOLDEN, REF_SHARE, ROOT, options_from_args
from distortion_ref import distortion_of_planes
from pixels_ref import pixels_of_planes

pytestmark = pytest.mark.gpu

DFIASCO = os.path.join(ROOT, "oracle", "_ref", "dfiasco_ref")
LEVELS = (-1, 0, 1, 35, 70, 100)


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


def target(geom, layout="interleaved"):
    w, h, bands = geom
    return pattern(h, w) if bands == 1 else pattern(h, w, 3) if layout == "interleaved" else pattern(3, h, w)


def as_pixels(t):
    """a target as H x W or H x W x 3 on the host"""
    a = t.cpu().numpy()
    return a.transpose(1, 2, 0) if a.ndim == 3 and a.shape[0] == 3 and a.shape[2] != 3 else a


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def pixels(planes):
    return pixels_of_planes(planes[0] if planes.shape[0] == 1 else planes)


def array_of_pnm(data):
    """raw PGM / PPM bytes -> H x W or H x W x 3"""
    w, h, bands = fiasco_amd._pnm_geometry(data)
    a = np.frombuffer(data[len(data) - w * h * bands:], dtype=np.uint8).copy()
    return a.reshape(h, w) if bands == 1 else a.reshape(h, w, 3)


def smoothed_entry(b, targets, n):
    """the C entry itself, whatever n is (Batch.decode_device goes to the unsmoothed entry for 0)"""
    arr = fiasco_amd._device_targets(targets)
    on = fiasco_amd._stream_of([t for t in targets if t is not None], None)
    return b.lib.L.fiasco_amd_batch_decode_device_smoothed(b.handle, n, arr, on)


# ------------------------------------------------------------------ 1. the arithmetic over its domain, kernel alone

def sweep(orientation):
    """(index arrays of a and b, the border list) of a 256 x 512 plane in which 65 536 pairs lie across borders of one
    pass: horizontal -- rows 2 r (a) and 2 r + 1 (b), one border of 512 columns per row pair (level 19); vertical --
    columns 2 c (a) and 2 c + 1 (b), one border of 256 rows per column pair (level 16)"""
    if orientation == "horizontal":
        borders = [(0, 2 * r + 1, 512, 19, 0) for r in range(128)]
        ia = (slice(0, 256, 2), slice(None))
        ib = (slice(1, 256, 2), slice(None))
    else:
        borders = [(2 * c + 1, 0, 256, 16, 0) for c in range(256)]
        ia = (slice(None), slice(0, 512, 2))
        ib = (slice(None), slice(1, 512, 2))
    return ia, ib, borders


@pytest.mark.parametrize("orientation", ["horizontal", "vertical"])
def test_arithmetic_is_exact_over_all_int16_values(gpu, orientation):
    ia, ib, borders = sweep(orientation)
    rng = np.random.default_rng(7)
    a = rng.permutation(np.arange(-32768, 32768, dtype=np.int64))
    shape = (128, 512) if orientation == "horizontal" else (256, 256)
    others = [np.full(65536, v, dtype=np.int64) for v in (-32768, -1, 0, 1, 32767)] + [a, np.full(65536, 12345, dtype=np.int64),
                                                                                      np.full(65536, -20001, dtype=np.int64)]
    for n in (1, 35, 70, 100):
        f = smooth_ref.factors(n)
        for k, b in enumerate(others):
            plane = np.zeros((256, 512), dtype=np.int16)
            plane[ia], plane[ib] = a.reshape(shape), b.reshape(shape)
            want = plane.copy()
            one, two = smooth_ref.blend(a, b, *f)
            want[ia], want[ib] = one.reshape(shape), two.reshape(shape)
            d = to_gpu(plane)
            fiasco_amd.smooth_planes_device(gpu, d, borders, n)
            got = d.cpu().numpy()
            assert np.array_equal(got, want), (orientation, n, k, int((got != want).sum()))
    # the restatement's own loop over the list says the same for one of them
    assert np.array_equal(smooth_ref.smooth(plane, borders, 100), want)


# ------------------------------------------------------------------ 2. order and edges, kernel alone, 16 x 16

def small_plane(seed=1):
    return np.random.default_rng(seed).integers(-32768, 32768, (16, 16)).astype(np.int16)


def run_small(gpu, plane, borders, n):
    d = to_gpu(plane)
    fiasco_amd.smooth_planes_device(gpu, d, borders, n)
    return d.cpu().numpy()


def test_order_of_the_passes_and_the_edges_of_the_plane(gpu):
    plane = small_plane()
    # a horizontal border (level 5: 4 long, rows 7 and 8, columns 4 .. 7) crossed by a vertical one (level 6: 8 long,
    # columns 5 and 6, rows 4 .. 11): four pixels belong to both
    h, v = (4, 8, 4, 5), (6, 4, 8, 6)
    first_h = [h + (0,), v + (1,)]
    first_v = [v + (0,), h + (1,)]
    want_h, want_v = smooth_ref.smooth(plane, first_h, 70), smooth_ref.smooth(plane, first_v, 70)
    assert not np.array_equal(want_h, want_v)
    assert np.array_equal(run_small(gpu, plane, first_h, 70), want_h)
    assert np.array_equal(run_small(gpu, plane, first_v, 70), want_v)
    # the last row, the first column a border can have, a border clipped to one pair in the last row and column
    edges = [(0, 15, 4, 5, 0), (12, 15, 4, 5, 0), (1, 0, 8, 6, 1), (15, 15, 1, 6, 1), (15, 0, 8, 6, 1)]
    want = smooth_ref.smooth(plane, edges, 35)
    assert (want != plane).sum() > 30
    assert np.array_equal(run_small(gpu, plane, edges, 35), want)
    # nothing to do: an empty list, 0 per cent
    assert np.array_equal(run_small(gpu, plane, [], 70), plane)
    assert np.array_equal(run_small(gpu, plane, edges, 0), plane)
    # a plane inside a larger allocation: what lies around it stays
    big = to_gpu(np.random.default_rng(2).integers(-32768, 32768, (3, 16, 16)).astype(np.int16))
    keep = big.clone()
    fiasco_amd.smooth_planes_device(gpu, big[1], edges, 35)
    assert np.array_equal(big[1].cpu().numpy(), smooth_ref.smooth(keep[1].cpu().numpy(), edges, 35))
    assert torch.equal(big[0], keep[0]) and torch.equal(big[2], keep[2])


class Raw:
    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<i2", "data": (ptr, False), "version": 3, "strides": None}


def test_refusals_of_the_kernel_alone_write_nothing(gpu):
    plane = small_plane(3)
    d = to_gpu(plane)
    cases = [
        ([(0, 16, 4, 5, 0)], "outside the plane"),                       # row 16 of 16
        ([(14, 8, 4, 5, 0)], "outside the plane"),                       # columns 14 .. 17
        ([(0, 4, 8, 6, 0)], "outside the plane"),                        # no column before the first
        ([(4, 12, 8, 6, 0)], "outside the plane"),                       # rows 12 .. 19
        ([(4, 8, 4, 5, 0), (6, 4, 8, 6, 2)], "without gaps"),
        ([(4, 8, 4, 5, 1)], "without gaps"),
        ([(4, 8, 4, 5, 0), (6, 4, 8, 6, 0)], "two levels in one pass"),
        ([(4, 8, 0, 5, 0)], "length"),
        ([(4, 8, 4, 5, 0), (6, 4, 8, 6, 1), (4, 16, 4, 5, 2)], "outside the plane"),      # the last of a good list
    ]
    for borders, msg in cases:
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.smooth_planes_device(gpu, d, borders, 70)
        assert msg in str(e.value), (borders, str(e.value))
        assert np.array_equal(d.cpu().numpy(), plane), borders
    host = plane.copy()
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.smooth_planes_device(gpu, Raw(host.ctypes.data, (16, 16)), [(4, 8, 4, 5, 0)], 70)
    assert "not in device memory" in str(e.value) and np.array_equal(host, plane)
    # a plane that is larger than its allocation (128 MB claimed at a tensor of 512 bytes)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.smooth_planes_device(gpu, Raw(d.data_ptr(), (8192, 8192)), [(4, 8, 4, 5, 0)], 70)
    assert "beyond the end of its device allocation" in str(e.value) and np.array_equal(d.cpu().numpy(), plane)


# ------------------------------------------------------------------ 3. the reference's bytes

def fixture_cases():
    return json.load(open(os.path.join(GOLDEN, "DECODED_SMOOTH.json")))["cases"]


@pytest.fixture(scope="module")
def coded(gpu, inputs):
    """per fixture case: the frame coded on the device twice -- PNM-fed and device-fed --, its unsmoothed planes and its
    border list; computed once and left alone"""
    out, keep = {}, []
    for name, ent in fixture_cases().items():
        q, o = options_from_args(gpu, ent["args"])
        o.set_smoothing(ent["smoothing"])
        data = smooth_ref.case_input(inputs, ent)
        fed = []
        for device_fed in (False, True):
            b = fiasco_amd.Batch.from_device(gpu, [to_gpu(array_of_pnm(data))], q, o) if device_fed else fiasco_amd.Batch(gpu, [data], q, o)
            stream = b.encode()[0]
            assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], (name, device_fed, gpu.error_message())
            fed.append(b)
        planes, borders = fed[0].decode_planes(0), fed[0].smoothing_borders(0)
        assert np.array_equal(fed[1].decode_planes(0), planes) and fed[1].smoothing_borders(0) == borders, name
        planes.setflags(write=False)
        out[name] = (ent, fed, planes, borders)
        keep.append(o)
    yield out
    for ent, fed, _, _ in out.values():
        for b in fed:
            b.free()
    for o in keep:
        o.delete()


@pytest.mark.parametrize("name", sorted(fixture_cases()))
def test_batch_entry_gives_the_references_bytes(gpu, coded, name):
    ent, fed, planes, borders = coded[name]
    geom = fed[0]._geom[0]
    layouts = ("interleaved", "planar") if ent["color"] else ("gray",)
    for b in fed:
        for n in LEVELS:
            for layout in layouts:
                t = target(geom, layout)
                assert smoothed_entry(b, [t], n) == 1, (name, n, gpu.error_message())
                assert md5(as_pixels(t)) == ent["decoded_md5"][str(n)], (name, n, layout)
        t = target(geom)
        assert b.decode_device([t], smoothing=-1) == 1 and md5(as_pixels(t)) == ent["decoded_md5"]["-1"]
    # the restatement on the device's planes says the same, and the counters count the pairs: 8 bytes each
    assert md5(pixels(smooth_ref.smooth_planes(planes, borders, 70))) == ent["decoded_md5"]["70"]
    counted = []
    for n in (0, 70):
        gpu.reset_stats()
        assert smoothed_entry(fed[0], [target(geom)], n) == 1
        st = gpu.get_stats()
        assert st.decoder_frames == 1
        counted.append(st.decoder_bytes)
    assert counted[1] - counted[0] == 8 * sum(b[2] for b in borders), name


# ------------------------------------------------------------------ 4. flights

def test_two_flights_of_mixed_colour_frames_three_times(gpu, inputs):
    names = ["carry48_a", "carry48_b", "carry48_c", "carry74_a", "carry74_b"]
    ent = fixture_cases()["carry74_a"]
    q, o = options_from_args(gpu, ent["args"])
    arrs = [array_of_pnm(inputs.data(names[i % 5])) for i in range(34)]
    sizes = {a.shape for a in arrs[:32]}
    assert len(sizes) == 2                                              # two sizes in one flight
    b = fiasco_amd.Batch.from_device(gpu, [to_gpu(a) for a in arrs], q, o)
    streams = b.encode()
    assert None not in streams, gpu.error_message()
    want = {}
    for i in range(34):
        if streams[i] not in want:                                      # five pictures: five streams
            want[streams[i]] = pixels(smooth_ref.smooth_planes(b.decode_planes(i), b.smoothing_borders(i), 70))
        else:
            assert b.smoothing_borders(i) == b.smoothing_borders(i % 5)
    assert len(want) == 5
    plain = [target(g) for g in b._geom]
    assert b.decode_device(plain) == 34
    for call in range(3):
        ts = [target(g) for g in b._geom]
        assert b.decode_device(ts, smoothing=70) == 34, gpu.error_message()
        for i in range(34):
            got = as_pixels(ts[i])
            assert np.array_equal(got, want[streams[i]]), (call, i)
            assert not np.array_equal(got, as_pixels(plain[i])), i
    # frames without a target are skipped and counted out; their neighbours are written
    ts = [None if i in (0, 7, 31, 33) else target(g) for i, g in enumerate(b._geom)]
    assert b.decode_device(ts, smoothing=70) == 30
    assert all(t is None or np.array_equal(as_pixels(t), want[streams[i]]) for i, t in enumerate(ts))
    b.free(); o.delete()


# ------------------------------------------------------------------ 5. the distortion of the smoothed frame

@pytest.mark.parametrize("name", sorted(fixture_cases()))
def test_distortion_is_that_of_the_smoothed_frame(gpu, coded, name):
    ent, fed, planes, borders = coded[name]
    bands = planes.shape[0]
    plain = fed[0].decode_distortion_device()
    for b in fed:
        orig = b.input_planes(0)
        for n in (70, 35, -1):
            shown = smooth_ref.smooth_planes(planes, borders, ent["smoothing"] if n < 0 else n)
            sse, mx = distortion_of_planes(orig, shown)
            good, gsse, gmx, _ = b.decode_distortion_device(smoothing=n)
            assert good == 1 and gsse[0] == sse and gmx[0] == mx, (name, n, gsse, sse)
            assert gsse[0][bands:] == [0] * (3 - bands)
            if bands == 3:
                assert gsse[0][1:] == plain[1][0][1:]                   # only Y is smoothed
            t = target(b._geom[0])
            good, tsse, tmx, _ = b.decode_distortion_device([t], smoothing=n)
            assert good == 1 and tsse[0] == sse and tmx[0] == mx and md5(as_pixels(t)) == ent["decoded_md5"][str(n)], (name, n)
    assert fed[0].decode_distortion_device() == plain                   # the unsmoothed call as before
    # smoothing 0 through the C entry: the unsmoothed sums
    s, m = (ctypes.c_ulonglong * 3)(), (ctypes.c_uint * 3)()
    assert gpu.L.fiasco_amd_batch_decode_distortion_device_smoothed(fed[0].handle, 0, s, m, None, None) == 1
    assert list(s) == plain[1][0] and list(m) == plain[2][0]


# ------------------------------------------------------------------ 6. nothing else moved

def test_unsmoothed_outlets_give_what_they_gave(gpu, coded):
    for name, (ent, fed, planes, borders) in coded.items():
        for b in fed:
            t = target(b._geom[0])
            assert b.decode_device([t]) == 1 and md5(as_pixels(t)) == ent["decoded_md5"]["0"], name
    for name in ("c256", "g100x70"):
        ent, fed, planes, borders = coded[name]
        b = fed[1]
        w, h, bands = b._geom[0]
        tw, th = fiasco_amd.magnified_size(gpu, w, h, -1)
        t, small, want = target(b._geom[0]), target((tw, th, bands)), target((tw, th, bands))
        assert b.decode_thumbnails([t], 1, [small]) == 1, gpu.error_message()
        assert md5(as_pixels(t)) == ent["decoded_md5"]["0"], name
        assert b.decode_device([want], magnify=-1) == 1 and torch.equal(small, want), name


def test_refusals_of_the_batch_entries_on_the_device(gpu, coded):
    ent, fed, planes, borders = coded["g100x70"]
    b = fed[0]
    t = target(b._geom[0])
    keep = t.clone()
    for bad in (-2, 101):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_device([t], smoothing=bad)
        assert "smoothing out of range" in str(e.value) and torch.equal(t, keep)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_device([t], magnify=-1, smoothing=70)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_device([pattern(64, 64)], smoothing=70)                # the sibling's target rules
    assert "<device target 0>" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_device([None], smoothing=70)
    assert torch.equal(t, keep)


# ------------------------------------------------------------------ 7. the live reference

def test_live_reference_decoder_shows_the_same_bytes(gpu, tmp_path):
    if not os.path.exists(DFIASCO):
        pytest.skip("the reference's binaries did not travel (oracle/ref_build.sh builds them in the build container)")
    env = dict(os.environ, FIASCO_DATA=GOLDEN + ":" + REF_SHARE)
    frames = [synth.noise(100, 70, 7), np.random.default_rng(3).integers(0, 256, (64, 96, 3)).astype(np.uint8)]
    o = gpu.cli_options()
    b = fiasco_amd.Batch.from_device(gpu, [to_gpu(a) for a in frames], 20.0, o)
    streams = b.encode()
    assert None not in streams, gpu.error_message()
    for n in (-1, 35):
        ts = [target(g) for g in b._geom]
        assert b.decode_device(ts, smoothing=n) == 2, gpu.error_message()
        for i, a in enumerate(frames):
            fco, dec = str(tmp_path / ("l%d.fco" % i)), str(tmp_path / ("l%d_%d.pnm" % (i, n)))
            open(fco, "wb").write(streams[i])
            subprocess.check_call([DFIASCO, "-s", str(n), "-o", dec, fco], env=env, stderr=subprocess.DEVNULL)
            raw = open(dec, "rb").read()
            got = as_pixels(ts[i])
            assert raw[:2] == (b"P6" if a.ndim == 3 else b"P5")
            assert raw[len(raw) - got.size:] == got.tobytes(), (i, n)
    plain = [target(g) for g in b._geom]
    assert b.decode_device(plain) == 2
    assert all(not torch.equal(p, t) for p, t in zip(plain, ts))       # the smoothing changed something
    b.free(); o.delete()
