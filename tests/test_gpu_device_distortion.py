"""Decoded distortion of a batch measured on the device (include/libfiasco_amd_hip.h:
fiasco_amd_batch_decode_distortion_device, fiasco_amd_planes_distortion_device; csrc/hip/distortion.inc), on the device:
the reduction kernel against its numpy restatement (tests/distortion_ref.py, pinned to the oracle's float sums by
tests/test_device_distortion_api.py) over its domain and the shapes at which it takes another path, the batch call
against the batch's own host outlets and the legacy PSNR call, flights, repeats, targets, shares, accounting, refusals.
Every comparison is == on integers."""
import ctypes
import math
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import synth
from distortion_ref import GOLDEN_CASES, distortion_of_planes, legacy_mse, reference_of_batch, staged_case

pytestmark = pytest.mark.gpu

EDGES = [-32768, -2049, -2048, -2033, -16, 0, 2031, 2032, 2047, 32767]


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


def pnm_of(a):
    return synth.pgm_bytes(a) if a.ndim == 2 else synth.ppm_bytes(a)


def array_of(pnm):
    """the pixels of raw PGM / PPM bytes: H x W or H x W x 3"""
    w, h, bands = fiasco_amd._pnm_geometry(pnm)
    a = np.frombuffer(pnm[len(pnm) - w * h * bands:], dtype=np.uint8).copy()
    return a.reshape((h, w) if bands == 1 else (h, w, 3))


def from_device(lib, pnms, q, o):
    return fiasco_amd.Batch.from_device(lib, [to_gpu(array_of(p)) for p in pnms], q, o)


def reference(b):
    """(sse, maxdiff) of every frame of a finished batch from its host outlets"""
    refs = [reference_of_batch(b, i) for i in range(b.n)]
    return [r[0] for r in refs], [r[1] for r in refs]


def raw_call(gpu, b, want_sse=True, want_max=True, targets=None):
    """the C entry itself with result arrays pre-filled with 7s -> (return value, sse array or None, maxdiff or None)"""
    c = ctypes
    f = gpu.L.fiasco_amd_batch_decode_distortion_device
    f.argtypes = [c.c_void_p, c.POINTER(c.c_ulonglong), c.POINTER(c.c_uint), c.POINTER(fiasco_amd.DeviceTarget), c.c_void_p]
    f.restype = c.c_int
    n = max(b.n if b else 1, 1)
    s = (c.c_ulonglong * (3 * n))(*([7] * (3 * n))) if want_sse else None
    m = (c.c_uint * (3 * n))(*([7] * (3 * n))) if want_max else None
    t = fiasco_amd._device_targets(targets) if targets is not None else None
    rc = f(b.handle if b else None, s, m, t, None)
    rows = lambda v: None if v is None else [list(v[3 * i:3 * i + 3]) for i in range(n)]
    return rc, rows(s), rows(m)


# ------------------------------------------------------------------ 1. the kernel over its domain

def random_planes(rng, bands, h, w):
    """int16 over the full range (both clips occur on both sides) with the edge values mixed in"""
    a = rng.integers(-32768, 32768, (bands, h, w)).astype(np.int16)
    flat = a.reshape(-1)
    at = rng.integers(0, flat.size, max(flat.size // 8, 1))
    flat[at] = rng.choice(np.array(EDGES, dtype=np.int16), at.size)
    return a


def test_kernel_equals_the_restatement_over_its_domain(gpu):
    rng = np.random.default_rng(7771)
    for bands in (1, 3):
        for w, h in ((1, 1), (16, 1), (33, 5), (47, 3), (250, 7), (256, 64)):
            a, c = random_planes(rng, bands, h, w), random_planes(rng, bands, h, w)
            if w * h >= 2 * len(EDGES):                 # every edge value against every other, on both sides
                a.reshape(-1)[:len(EDGES)] = EDGES
                c.reshape(-1)[:len(EDGES)] = EDGES[::-1]
            want = distortion_of_planes(a, c)
            da, dc = (to_gpu(a), to_gpu(c)) if bands == 3 else (to_gpu(a[0]), to_gpu(c[0]))
            assert fiasco_amd.planes_distortion_device(gpu, da, dc) == want, (bands, w, h)
    # the restatement saw both clips and the bytes next to them
    big = random_planes(rng, 1, 64, 256)
    big.reshape(-1)[:len(EDGES)] = EDGES
    by = np.clip((big.astype(np.int64) >> 4) + 128, 0, 255)
    assert {0, 1, 127, 128, 254, 255} <= set(np.unique(by).tolist())


def test_planes_that_are_only_two_byte_aligned(gpu):
    rng = np.random.default_rng(7772)
    for bands, w, h in ((1, 250, 7), (3, 33, 5), (1, 256, 64)):
        n = bands * w * h
        a, c = random_planes(rng, bands, h, w), random_planes(rng, bands, h, w)
        shape = (bands, h, w) if bands == 3 else (h, w)
        ha, hc = (np.concatenate([[12345], v.reshape(-1)]).astype(np.int16) for v in (a, c))
        da, dc = to_gpu(ha)[1:].view(shape), to_gpu(hc)[1:].view(shape)
        assert da.data_ptr() % 4 == 2 and dc.data_ptr() % 4 == 2 and da.numel() == n
        assert fiasco_amd.planes_distortion_device(gpu, da, dc) == distortion_of_planes(a, c), (bands, w, h)
        # one side aligned, the other not
        assert fiasco_amd.planes_distortion_device(gpu, to_gpu(a.reshape(shape)), dc) == distortion_of_planes(a, c), (bands, w, h)


# ------------------------------------------------------------------ 2. the sum needs 64 bits

def test_the_sum_is_64_bits_wide(gpu):
    lo = torch.full((512, 512), -32768, dtype=torch.int16, device="cuda")
    hi = torch.full((512, 512), 32767, dtype=torch.int16, device="cuda")
    sse, mx = fiasco_amd.planes_distortion_device(gpu, lo, hi)
    assert sse == [255 * 255 * 262144, 0, 0] and sse[0] == 17045913600 and sse[0] > 2 ** 32
    assert mx == [255, 0, 0]
    assert fiasco_amd.planes_distortion_device(gpu, hi, lo) == (sse, mx)


# ------------------------------------------------------------------ 3. equal planes

def test_equal_planes_give_zero_and_the_batch_reports_inf(gpu):
    rng = np.random.default_rng(7773)
    a = to_gpu(random_planes(rng, 3, 33, 47))
    assert fiasco_amd.planes_distortion_device(gpu, a, a) == ([0, 0, 0], [0, 0, 0])
    assert fiasco_amd.planes_distortion_device(gpu, a, a.clone()) == ([0, 0, 0], [0, 0, 0])
    # a frame of byte 128 is the zero plane, which the coder reproduces exactly (the host outlets say so)
    o = gpu.cli_options()
    b = fiasco_amd.Batch(gpu, [pnm_of(np.full((32, 32), 128, dtype=np.uint8)), pnm_of(synth.synth(32, 32, 5))], 20.0, o)
    assert None not in b.encode(), gpu.error_message()
    assert reference_of_batch(b, 0) == ([0, 0, 0], [0, 0, 0]) and reference_of_batch(b, 1)[0][0] > 0
    good, sse, mx, psnr = b.decode_distortion_device()
    assert good == 2 and sse[0] == [0, 0, 0] and mx[0] == [0, 0, 0]
    assert psnr[0] == [float("inf"), 0.0, 0.0]
    assert psnr[1][0] == 10.0 * math.log10(255.0 * 255.0 * 32 * 32 / sse[1][0]) and psnr[1][1:] == [0.0, 0.0]
    b.free(); o.delete()


# ------------------------------------------------------------------ 4. the batch path on the goldens

@pytest.mark.parametrize("name", GOLDEN_CASES)
def test_batch_equals_its_host_outlets_and_the_legacy_float_sum(gpu, manifest, inputs, name):
    count = 0
    for stage in (None, from_device):
        b, o, out = staged_case(gpu, manifest, inputs, name, stage)
        assert None not in out, (name, gpu.error_message())
        want_sse, want_max = reference(b)
        good, sse, mx, psnr = b.decode_distortion_device()
        assert good == b.n and sse == want_sse and mx == want_max, (name, stage is not None)
        legacy = b.decode_psnr_all()
        assert legacy[0] == b.n
        for i in range(b.n):
            w, h, bands = b._geom[i]
            for k in range(bands):
                if sse[i][k] < 2 ** 24:
                    assert legacy_mse(sse[i][k], w, h) == legacy[2][i][k], (name, i, k)
                    count += 1
        b.free(); o.delete()
    assert count                                        # the comparison with the legacy call must not be hollow


# ------------------------------------------------------------------ 5. two flights

def test_forty_frames_are_two_flights(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(32, 32, 400 + i) for i in range(40)]
    for stage in (None, from_device):
        b = (stage or fiasco_amd.Batch)(gpu, [pnm_of(a) for a in arrs], 20.0, o)
        assert None not in b.encode(), gpu.error_message()
        want_sse, want_max = reference(b)
        assert len(set(s[0] for s in want_sse)) > 20            # distinct frames, distinct numbers
        good, sse, mx, _ = b.decode_distortion_device()
        assert good == 40 and sse == want_sse and mx == want_max
        b.free()
    o.delete()


def test_a_frame_that_drops_out_of_a_flight_shifts_no_result(gpu, inputs):
    """35 frames, the second of which fails to code (MAXSTATES 103: the 256 x 256 survey image needs one state more): the
    first flight holds the jobs 0, 2 .. 32 -- from job 2 on a frame's place in the flight, which is its slot in the
    result array of the measuring launch, is not its job index --, the second the jobs 33 and 34.  Every number and every
    written target is its own frame's.  (The seeds: every 32 x 32 frame codes under that limit and all 34 sums differ,
    found with the oracle library; asserted again below.)"""
    o = gpu.cli_options()
    pnms = [pnm_of(synth.synth(32, 32, 400 + i)) for i in range(34)]
    pnms.insert(1, inputs.data("g256"))
    good = [i for i in range(35) if i != 1]
    try:
        gpu.set_limits(103, 22)
        b = fiasco_amd.Batch(gpu, pnms, 20.0, o)
        out = b.encode()
        assert out[1] is None and None not in [out[i] for i in good], gpu.error_message()
        want = {i: reference_of_batch(b, i) for i in good}
        sums = set(want[i][0][0] for i in good)
        assert 0 not in sums and len(sums) >= 20                # distinct frames, distinct numbers
        big = pattern(18, 40, 40)                               # the targets of the even frames, cut out of a pattern
        expect = big.clone()
        targets = [big[i // 2, 4:36, 4:36] if i % 2 == 0 else None for i in range(35)]
        count, sse, mx, _ = b.decode_distortion_device(targets)
        torch.cuda.synchronize()
        assert count == 34
        for i in good:
            assert (sse[i], mx[i]) == want[i], i
        assert sse[1] == [0, 0, 0] and mx[1] == [0, 0, 0]
        for i in range(0, 35, 2):
            expect[i // 2, 4:36, 4:36] = to_gpu(np.frombuffer(b.decode_plane(i, 0, 32, 32), dtype=np.uint8).reshape(32, 32))
        assert torch.equal(big, expect)                         # the frames' bytes inside, the pattern around them
        b.free()
    finally:
        gpu.set_limits(6000, 22)
        o.delete()


# ------------------------------------------------------------------ 6. repeats and partial outputs

def test_a_second_call_gives_the_same_numbers_and_every_output_is_optional(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(96, 64, 30 + i) for i in range(3)]
    b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in arrs], 20.0, o)
    assert None not in b.encode(), gpu.error_message()
    want_sse, want_max = reference(b)
    first = b.decode_distortion_device()
    assert first[1] == want_sse and first[2] == want_max
    assert b.decode_distortion_device() == first                # the result array is zeroed per flight
    assert raw_call(gpu, b) == (3, want_sse, want_max)
    assert raw_call(gpu, b, want_max=False) == (3, want_sse, None)
    assert raw_call(gpu, b, want_sse=False) == (3, None, want_max)
    ts = [torch.zeros((64, 96), dtype=torch.uint8, device="cuda") for _ in range(3)]
    assert raw_call(gpu, b, False, False, ts) == (3, None, None)
    torch.cuda.synchronize()
    for i in range(3):
        assert ts[i].cpu().numpy().tobytes() == b.decode_plane(i, 0, 96, 64)
    b.free(); o.delete()


# ------------------------------------------------------------------ 7. with targets: one decode serves both

def test_targets_get_the_bytes_of_decode_device_and_the_numbers_stay(gpu):
    o = gpu.cli_options()
    gray = [synth.synth(96, 64, 60 + i) for i in range(3)]
    col = [synth.synth_color_k(128, 96, 5), synth.synth_color_k(50, 34, 5)]
    b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in gray + col], 20.0, o)
    assert None not in b.encode(), gpu.error_message()
    plain = b.decode_distortion_device()
    assert plain[0] == 5 and (plain[1], plain[2]) == reference(b)

    def targets():
        """gray packed, gray cut out of a larger tensor (a pitch), one frame not written, interleaved, planar"""
        big = pattern(70, 120)
        return big, [torch.zeros((64, 96), dtype=torch.uint8, device="cuda"), big[3:67, 11:107], None,
                     torch.zeros((96, 128, 3), dtype=torch.uint8, device="cuda"), torch.zeros((3, 34, 50), dtype=torch.uint8, device="cuda")]

    bigw, want = targets()
    assert b.decode_device(want) == 4
    bigg, got = targets()
    assert got[1].stride(0) > 96
    spare = pattern(64, 96)                                     # frame 2 is measured, and nothing of it is written
    res = b.decode_distortion_device(got)
    torch.cuda.synchronize()
    assert res == plain
    for k in (0, 1, 3, 4):
        assert torch.equal(got[k], want[k]), k
    assert got[0].cpu().numpy().tobytes() == b.decode_plane(0, 0, 96, 64)
    assert torch.equal(bigg, bigw) and torch.equal(spare, pattern(64, 96))
    b.free(); o.delete()


# ------------------------------------------------------------------ 8. a device listed twice

def test_two_shares_on_one_gpu_give_the_same_numbers(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(96, 64, 70 + i) for i in range(4)] + [synth.synth_color_k(128, 96, 5)]
    want = {}
    for stage in (None, from_device):
        b = (stage or fiasco_amd.Batch)(gpu, [pnm_of(a) for a in arrs], 20.0, o)
        assert None not in b.encode(), gpu.error_message()
        want[stage] = b.decode_distortion_device()
        assert (want[stage][1], want[stage][2]) == reference(b)
        b.free()
    assert want[None] == want[from_device]
    gpu.set_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        for stage in (None, from_device):
            b = (stage or fiasco_amd.Batch)(gpu, [pnm_of(a) for a in arrs], 20.0, o)
            assert None not in b.encode(), gpu.error_message()
            assert b.decode_distortion_device() == want[stage]
            b.free()
    finally:
        gpu.set_devices([])
        o.delete()


# ------------------------------------------------------------------ 9. accounting

def test_accounting_is_the_decoders_plus_two_bytes_read_per_side(gpu):
    o = gpu.cli_options()
    arrs = [synth.synth(96, 64, 1), synth.synth_color_k(50, 34, 5), synth.synth(34, 40, 2)]
    vals = 96 * 64 + 3 * 50 * 34 + 34 * 40
    b = fiasco_amd.Batch(gpu, [pnm_of(a) for a in arrs], 20.0, o)
    assert None not in b.encode(), gpu.error_message()
    gpu.reset_stats()
    assert b.decode_psnr_all()[0] == 3
    st = gpu.get_stats()
    frames0, bytes0 = st.decoder_frames, st.decoder_bytes
    assert frames0 == 3 and bytes0 > 2 * vals
    assert b.decode_distortion_device()[0] == 3
    st = gpu.get_stats()
    frames1, bytes1 = st.decoder_frames, st.decoder_bytes
    assert frames1 - frames0 == 3 and bytes1 - bytes0 == bytes0 + 4 * vals
    # pixels written as well: 3 bytes more per value of the frames that have a target
    ts = [torch.zeros((64, 96), dtype=torch.uint8, device="cuda"), None, torch.zeros((40, 34), dtype=torch.uint8, device="cuda")]
    assert b.decode_distortion_device(ts)[0] == 3
    st = gpu.get_stats()
    assert st.decoder_frames - frames1 == 3 and st.decoder_bytes - bytes1 == bytes0 + 4 * vals + 3 * (96 * 64 + 34 * 40)
    b.free(); o.delete()


# ------------------------------------------------------------------ 10. refusals

def planes_call(gpu, pa, pb, bands, w, h):
    c = ctypes
    f = gpu.L.fiasco_amd_planes_distortion_device
    f.argtypes = [c.c_void_p, c.c_void_p, c.c_int, c.c_uint, c.c_uint, c.POINTER(c.c_ulonglong), c.POINTER(c.c_uint), c.c_void_p]
    f.restype = c.c_int
    s, m = (c.c_ulonglong * 3)(7, 7, 7), (c.c_uint * 3)(7, 7, 7)
    return f(pa, pb, bands, w, h, s, m, None), list(s), list(m)


def test_refusals_come_with_a_message_and_write_nothing(gpu):
    untouched = [7, 7, 7]
    dev = torch.zeros((64, 96), dtype=torch.int16, device="cuda")
    host = np.zeros((64, 96), dtype=np.int16)
    assert planes_call(gpu, dev.data_ptr(), dev.data_ptr(), 1, 96, 64) == (1, [0, 0, 0], [0, 0, 0])
    for args, msg in (((host.ctypes.data, dev.data_ptr(), 1, 96, 64), "`a' are not in device memory"),
                      ((dev.data_ptr(), host.ctypes.data, 1, 96, 64), "`b' are not in device memory"),
                      ((dev.data_ptr(), dev.data_ptr(), 3, 8192, 8192), "beyond the end of their device allocation"),
                      ((dev.data_ptr(), dev.data_ptr(), 2, 96, 64), "2 bands"),
                      ((dev.data_ptr(), dev.data_ptr(), 1, 0, 64), "0 x 64"),
                      ((dev.data_ptr(), dev.data_ptr(), 1, 96, 8193), "96 x 8193"),
                      ((None, dev.data_ptr(), 1, 96, 64), "no planes")):
        assert planes_call(gpu, *args) == (0, untouched, untouched), msg
        assert msg in gpu.error_message(), (msg, gpu.error_message())
    # the batch call: no batch, a batch before its first pass, nothing asked for, a bad target
    assert raw_call(gpu, None) == (0, [untouched], [untouched]) and "empty batch" in gpu.error_message()
    o = gpu.cli_options()
    b = fiasco_amd.Batch(gpu, [pnm_of(synth.synth(96, 64, 30 + i)) for i in range(2)], 20.0, o)
    assert raw_call(gpu, b) == (0, [untouched] * 2, [untouched] * 2) and "no finished pass" in gpu.error_message()
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_distortion_device()
    assert "no finished pass" in str(e.value)
    assert None not in b.encode(), gpu.error_message()
    assert raw_call(gpu, b, False, False)[0] == 0 and "no result arrays and no targets" in gpu.error_message()
    good, keep = pattern(64, 96), pattern(64, 96)
    for bad, msg in ((pattern(64, 64), "96 x 64"), (pattern(64, 96, 3), "colour model")):
        assert raw_call(gpu, b, targets=[good, bad]) == (0, [untouched] * 2, [untouched] * 2)
        assert msg in gpu.error_message() and "<device target 1>" in gpu.error_message()
        torch.cuda.synchronize()
        assert torch.equal(good, keep)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_distortion_device([good])                      # one target per frame
    assert b.decode_distortion_device()[0] == 2
    b.free(); o.delete()
