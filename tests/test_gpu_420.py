"""Decoding in 4:2:0 on the device (include/libfiasco_amd_420.h; csrc/hip/frame_decoder.inc dec_assemble420_kernel,
output_convert_420.inc oc420_convert_kernel): decode_planes_420 against the planes the reference's decoder makes with
fiasco_d_options_set_4_2_0_format, decode_420 into I420, NV12 and NV21 targets against the bytes computed from the reference's
planes (tests/golden/DECODED_420.json) at every recorded magnification and smoothing, packed and pitched on an odd base with
guard bytes; two flights with skipped frames and a frame that fails alone; the relations to the 4:4:4 decode; the kernel
alone on hand-made planes; the call twice and with the device listed twice."""
import hashlib
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import smooth_ref
import yuv420_ref

pytestmark = pytest.mark.gpu

CASES = sorted(n for n, e in yuv420_ref.fixture_cases().items() if not e["degenerate"])


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pattern(n):
    """bytes that no decoded frame looks like: what a call must leave alone is compared with them"""
    return ((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)


class Target:
    """a 4:2:0 target inside ONE flat buffer of pattern bytes: kind "i420", "nv12" or "nv21"; pitched: rows 7 (Y) and 5
    (chroma) bytes longer than they need to be and every plane on an odd address.  planes(): the bytes written, as Y, Cb,
    Cr arrays; untouched(): every other byte of the buffer kept its pattern"""

    def __init__(self, w, h, kind, pitched=False):
        self.w, self.h, self.kind = w, h, kind
        cw, ch = w // 2, h // 2
        crow = cw if kind == "i420" else 2 * cw
        yp, cp = (w + 7, crow + 5) if pitched else (w, crow)
        gap = 33 if pitched else 0                  # 16 n + 1: with the first plane at 1 every plane begins on an odd address
        at = 1 if pitched else 0
        spans = []
        for rows, row, pitch in [(h, w, yp)] + [(ch, crow, cp)] * (2 if kind == "i420" else 1):
            at += (-at) % 16 + 1 if pitched else 0
            spans.append((at, rows, row, pitch))
            at += (rows - 1) * pitch + row + gap
        self.spans = spans
        self.buf = to_gpu(pattern(at + 64))
        view = [torch.as_strided(self.buf, (rows, row), (pitch, 1), off) for off, rows, row, pitch in spans]
        if kind == "i420":
            self.arrays = tuple(view)
        else:
            off, rows, row, pitch = spans[1]
            self.arrays = (view[0], torch.as_strided(self.buf, (rows, cw, 2), (pitch, 2, 1), off))
        assert not pitched or all(off % 2 == 1 for off, _, _, _ in spans)

    def order(self):
        return "nv21" if self.kind == "nv21" else "nv12"

    def planes(self):
        host = self.buf.cpu().numpy()
        got = [np.lib.stride_tricks.as_strided(host[off:], (rows, row), (pitch, 1)).copy() for off, rows, row, pitch in self.spans]
        if self.kind == "i420":
            return got
        pairs = got[1].reshape(got[1].shape[0], -1, 2)
        first, second = pairs[:, :, 0], pairs[:, :, 1]
        return [got[0], first, second] if self.kind == "nv12" else [got[0], second, first]

    def untouched(self):
        host = self.buf.cpu().numpy()
        keep = np.ones(host.size, dtype=bool)
        for off, rows, row, pitch in self.spans:
            for r in range(rows):
                keep[off + r * pitch:off + r * pitch + row] = False
        return np.array_equal(host[keep], pattern(host.size)[keep])

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), pattern(self.buf.numel()))


def md5_i420(planes):
    return hashlib.md5(b"".join(np.ascontiguousarray(p).tobytes() for p in planes)).hexdigest()


def md5_nv12(planes):
    return hashlib.md5(np.ascontiguousarray(planes[0]).tobytes() + np.stack([planes[1], planes[2]], -1).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def coded(gpu, inputs):
    """per fixture case: the frame coded on the device, as a finished batch of one; computed once and left alone"""
    out, keep = {}, []
    for name, ent in yuv420_ref.fixture_cases().items():
        b, o = yuv420_ref.staged(gpu, inputs, ent)
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == ent["stream_md5"], (name, gpu.error_message())
        out[name] = (ent, b)
        keep.append(o)
    yield out
    for ent, b in out.values():
        b.free()
    for o in keep:
        o.delete()


# ------------------------------------------------------------------ 1. the reference's planes and bytes

@pytest.mark.parametrize("name", CASES)
def test_decode_planes_420_gives_the_references_planes(gpu, coded, name):
    ent, b = coded[name]
    for m, rec in yuv420_ref.accepted(ent):
        y, cb, cr = b.decode_planes_420(0, magnify=m)
        assert y.shape == (rec["height"], rec["width"]) and cb.shape == cr.shape == (rec["height"] // 2, rec["width"] // 2), (name, m)
        assert [yuv420_ref.md5(p.tobytes()) for p in (y, cb, cr)] == rec["planes_md5"], (name, m)
        assert cb.any() and cr.any(), (name, m)


@pytest.mark.parametrize("name", CASES)
def test_decode_420_gives_the_references_bytes_in_every_layout(gpu, coded, name):
    ent, b = coded[name]
    seen = 0
    for m, rec in yuv420_ref.accepted(ent):
        w, h = rec["width"], rec["height"]
        for k, s in enumerate(yuv420_ref.SMOOTHING):
            want = rec["md5"][str(s)]
            # packed I420 and NV12 at every smoothing; the pitched targets on odd bases and NV21 take turns
            for kind, pitched in (("i420", False), ("nv12", False), (("nv21", "i420", "nv12")[k], True)):
                t = Target(w, h, kind, pitched)
                assert b.decode_420([t.arrays], magnify=m, smoothing=s, order=t.order()) == 1, (name, m, s, kind, gpu.error_message())
                got = t.planes()
                assert yuv420_ref.md5(got[0].tobytes()) == want["y"], (name, m, s, kind, pitched)
                assert md5_i420(got) == want["i420"] and md5_nv12(got) == want["nv12"], (name, m, s, kind, pitched)
                assert t.untouched(), (name, m, s, kind, pitched)
                seen += 1
        # NV21 is NV12 with the pairs swapped, byte for byte in the buffer
        a, z = Target(w, h, "nv12"), Target(w, h, "nv21")
        assert b.decode_420([a.arrays], magnify=m) == 1 and b.decode_420([z.arrays], magnify=m, order="nv21") == 1      # the defaults: -1
        ha, hz = a.buf.cpu().numpy()[:w * h * 3 // 2], z.buf.cpu().numpy()[:w * h * 3 // 2]
        assert np.array_equal(ha[:w * h], hz[:w * h]) and np.array_equal(ha[w * h:].reshape(-1, 2), hz[w * h:].reshape(-1, 2)[:, ::-1])
        assert hashlib.md5(ha.tobytes()).hexdigest() == rec["md5"]["-1"]["nv12"], (name, m)
    assert seen >= 18
    if name == "c34":
        t = Target(34, 34, "i420")
        assert b.decode_420([t.arrays]) == 1
        raw = yuv420_ref.unpack(ent["decoded"]["0"]["i420_zlib_b64"])
        got = b"".join(p.tobytes() for p in t.planes())
        assert got == raw, [i for i in range(len(raw)) if raw[i] != got[i]][:20]
    # the size rule's refusals are the call's, nothing written
    if ent["decoded"]["0"]["below_refused"]:
        t = Target(ent["width"], ent["height"], "nv12")
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_420([t.arrays], magnify=-1)
        assert "Minimum value is 0." in str(e.value) and t.unchanged()


# ------------------------------------------------------------------ 2. flights

def test_two_flights_with_skipped_frames_and_one_that_fails_alone(gpu, inputs):
    """34 frames -- two flights of 32 -- of two small cases at `cfiasco' defaults, the flat frame in the middle: it fails
    alone with its message, its neighbours are written, None targets are skipped"""
    cases = yuv420_ref.fixture_cases()
    names = ["c34" if i % 2 else "c102x66" for i in range(34)]
    names[17] = "flat64"
    assert all(cases[n]["args"] == [] and cases[n]["smoothing"] == 70 for n in set(names))
    o = gpu.cli_options()
    o.set_smoothing(70)
    b = fiasco_amd.Batch(gpu, [yuv420_ref.synth_input(cases[n]["input"])[0] for n in names], 20.0, o)
    streams = b.encode()
    assert all(s is not None and hashlib.md5(s).hexdigest() == cases[n]["stream_md5"] for s, n in zip(streams, names)), gpu.error_message()
    skipped = {3, 16, 32}
    targets = [None if i in skipped else Target(cases[n]["width"], cases[n]["height"], "nv12" if i % 3 else "i420", pitched=i % 5 == 0)
               for i, n in enumerate(names)]
    good = b.decode_420([None if t is None else t.arrays for t in targets])
    assert good == 34 - len(skipped) - 1, gpu.error_message()
    msg = gpu.error_message()
    assert "<device target 17>" in msg and "max_level" in msg and "chroma root has level 12" in msg, msg
    for i, (t, n) in enumerate(zip(targets, names)):
        if t is None:
            continue
        if i == 17:
            assert t.unchanged()
            continue
        got = t.planes()
        assert md5_nv12(got) == cases[n]["decoded"]["0"]["md5"]["-1"]["nv12"] and t.untouched(), (i, n)
    # the flat frame alone: the call has nothing to write
    only = [None] * 34
    only[17] = targets[17].arrays
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_420(only)
    assert "max_level" in str(e.value) and targets[17].unchanged()
    b.free(); o.delete()


# ------------------------------------------------------------------ 3. against the 4:4:4 decode

def test_y_is_the_444_y_and_chroma_at_1_is_the_444_chroma_at_0(gpu, coded):
    ent, b = coded["c256sq"]
    full = b.decode_planes(0)                                   # 4:4:4, the coded size
    gray = to_gpu(pattern(256 * 256).reshape(256, 256))
    fiasco_amd.planes_to_pixels_device(gpu, to_gpu(full[0]), gray)      # the Y plane through decode_device()'s kernel, as a gray frame
    t = Target(256, 256, "i420")
    assert b.decode_420([t.arrays], smoothing=0) == 1
    got = t.planes()
    assert np.array_equal(got[0], gray.cpu().numpy()) and np.array_equal(got[0], yuv420_ref.to_bytes(full[0]))
    t = Target(512, 512, "i420")
    assert b.decode_420([t.arrays], magnify=1, smoothing=0) == 1
    got = t.planes()
    assert np.array_equal(got[1], yuv420_ref.to_bytes(full[1])) and np.array_equal(got[2], yuv420_ref.to_bytes(full[2]))
    # smoothed, the Y plane is NOT the smoothed 4:4:4 one
    y444 = yuv420_ref.to_bytes(smooth_ref.smooth(full[0], b.smoothing_borders(0), 70))
    t = Target(256, 256, "nv12")
    assert b.decode_420([t.arrays]) == 1 and np.count_nonzero(t.planes()[0] != y444) > 0


# ------------------------------------------------------------------ 4. the kernel alone

@pytest.mark.parametrize("kind", ["i420", "nv12", "nv21"])
def test_kernel_alone_on_the_handmade_planes_of_the_host_replay(gpu, kind):
    for w in (2, 30, 34, 50):
        for h in (2, 6):
            planes = yuv420_ref.handmade(w, h)
            for p in planes[:1] + ([planes[1]] if planes[1].size >= 4 else []):
                assert set(yuv420_ref.SPECIALS) <= set((p.astype(np.int32) >> 4).ravel().tolist())
            dev = [to_gpu(p) for p in planes]
            for pitched in (False, True):
                t = Target(w, h, kind, pitched)
                fiasco_amd.planes_to_420_device(gpu, dev[0], dev[1], dev[2], t.arrays, order=t.order())
                torch.cuda.synchronize()
                got = t.planes()
                for k in range(3):
                    assert np.array_equal(got[k], yuv420_ref.to_bytes(planes[k])), (w, h, kind, pitched, k)
                assert t.untouched(), (w, h, kind, pitched)


# ------------------------------------------------------------------ 5. again, and on two shares of one device

def test_the_call_twice_in_a_row_and_with_the_device_listed_twice(gpu, coded, inputs):
    ent, b = coded["carry74_a"]
    rec = ent["decoded"]["0"]
    for _ in range(2):
        t = Target(rec["width"], rec["height"], "nv12")
        assert b.decode_420([t.arrays]) == 1 and md5_nv12(t.planes()) == rec["md5"]["-1"]["nv12"]
    cases = yuv420_ref.fixture_cases()
    names = ["c34", "c102x66", "c34", "c102x66", "c34"]
    o = gpu.cli_options()
    o.set_smoothing(70)
    gpu.set_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        b2 = fiasco_amd.Batch(gpu, [yuv420_ref.synth_input(cases[n]["input"])[0] for n in names], 20.0, o)
        assert None not in b2.encode(), gpu.error_message()
        targets = [Target(cases[n]["width"], cases[n]["height"], "i420", pitched=i == 1) for i, n in enumerate(names)]
        assert b2.decode_420([t.arrays for t in targets], smoothing=35) == 5, gpu.error_message()
        for t, n in zip(targets, names):
            assert md5_i420(t.planes()) == cases[n]["decoded"]["0"]["md5"]["35"]["i420"] and t.untouched(), n
        y, cb, cr = b2.decode_planes_420(1)
        assert [yuv420_ref.md5(p.tobytes()) for p in (y, cb, cr)] == cases["c102x66"]["decoded"]["0"]["planes_md5"]
        b2.free()
    finally:
        gpu.set_devices([])
        o.delete()


def test_a_gray_batch_is_refused_frame_by_frame(gpu, inputs):
    o = gpu.cli_options()
    b = fiasco_amd.Batch(gpu, [inputs.data("g96x64")], 20.0, o)
    assert b.encode()[0] is not None
    t = Target(96, 64, "nv12")
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_420([t.arrays])
    assert "<device target 0>" in str(e.value) and "gray frame" in str(e.value) and t.unchanged()
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_planes_420(0)
    assert "gray frame" in str(e.value)
    b.free(); o.delete()
