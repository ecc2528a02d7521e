"""Decoded frames in the pixel formats of a display (include/libfiasco_amd_render.h; csrc/hip/render.inc), on the device:
the kernel alone against the REAL reference's bytes on the hand-made planes of tests/golden/RENDERED.json; against the numpy
restatement tests/render_ref.py at ragged widths, on pitched surfaces and on surfaces that begin one pixel into their
allocation, every byte outside the rows untouched; device == host loop == numpy on full-range planes; decode_rendered against
the reference's bytes for the coded cases at every recorded magnification and smoothing under all twelve renderers, and the
same bytes from decode_planes + numpy smoothing + numpy rendering; a flight of mixed sizes with a skipped frame; a frame the
shown path refuses beside frames that are written; refused calls write nothing; ordering against the caller's stream."""
import hashlib
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import render_ref
import shown_ref
import smooth_ref
import synth
from conftest import options_from_args

pytestmark = pytest.mark.gpu

NAMES = sorted(render_ref.RENDERERS)
WIDTHS, HEIGHTS = (1, 15, 16, 17, 33), (1, 3)


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


@pytest.fixture(scope="module")
def renderers(gpu):
    made = {n: fiasco_amd.Renderer(gpu, red, green, blue, bpp, doubled) for n, (bpp, red, green, blue, doubled) in render_ref.RENDERERS.items()}
    yield made
    for r in made.values():
        r.delete()


def to_gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pattern(n):
    """n bytes that no rendered frame looks like: what a call must leave alone is compared with it"""
    return ((np.arange(n, dtype=np.int64) * 37 + 11) % 251).astype(np.uint8)


class Surface:
    """a surface of sw x sh pixels of `px' bytes inside a flat allocation of pattern bytes: `lead' bytes before the first
    pixel, `extra' bytes between two rows, 32 behind the last"""

    def __init__(self, sw, sh, px, lead=0, extra=0):
        self.row, self.pitch, self.lead, self.sh = sw * px, sw * px + extra, lead, sh
        self.n = lead + (sh - 1) * self.pitch + self.row + 32
        self.buf = to_gpu(pattern(self.n))
        self.view = torch.as_strided(self.buf, (sh, sw, px), (self.pitch, px, 1), lead)

    def rows(self):
        """(the rows as bytes, whether every byte outside them kept the pattern)"""
        got, want = self.buf.cpu().numpy(), pattern(self.n)
        inside = np.zeros(self.n, dtype=bool)
        for y in range(self.sh):
            inside[self.lead + y * self.pitch:self.lead + y * self.pitch + self.row] = True
        return got[inside].tobytes(), bool(np.array_equal(got[~inside], want[~inside]))

    def untouched(self):
        return bool(np.array_equal(self.buf.cpu().numpy(), pattern(self.n)))


def surface_for(name, w, h, lead=0, extra=0):
    bpp, _, _, _, doubled = render_ref.RENDERERS[name]
    sw, sh, _ = render_ref.surface_size(bpp, doubled, w, h)
    return Surface(sw, sh, bpp // 8, lead, extra)


def md5(data):
    return hashlib.md5(bytes(data)).hexdigest()


# ------------------------------------------------------------------ 1. the kernel alone

def test_kernel_gives_the_references_bytes_on_the_handmade_planes(gpu, renderers):
    fx = render_ref.fixture()["handmade"]["planes"]
    for kind in ("gray", "color"):
        for n in NAMES:
            rec = fx[kind][n]
            planes = render_ref.handmade(rec["width"], rec["height"], kind == "color")
            assert md5(planes.tobytes()) == rec["planes_md5"], (kind, n)
            s = surface_for(n, rec["width"], rec["height"])
            fiasco_amd.render_planes_device(gpu, renderers[n], to_gpu(planes), s.view)
            got, clean = s.rows()
            assert md5(got) == rec["md5"] and clean, (kind, n)


@pytest.fixture(scope="module")
def ragged():
    """(w, h, color) -> full-range int16 planes on the host and on the device, made once and left alone"""
    rng = np.random.RandomState(7)
    out = {}
    for w in WIDTHS:
        for h in HEIGHTS:
            for color in (False, True):
                p = rng.randint(-4096, 4096, size=(3, h, w) if color else (h, w)).astype(np.int16)
                p.reshape(-1)[::5] = rng.randint(-32768, 32768, size=p.reshape(-1)[::5].shape)
                dev = to_gpu(p)
                p.setflags(write=False)
                out[w, h, color] = (p, dev)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_kernel_at_ragged_widths_on_packed_pitched_and_offset_surfaces(gpu, renderers, ragged, name):
    bpp, _, _, _, doubled = render_ref.RENDERERS[name]
    px = bpp // 8
    seen = refused = 0
    for (w, h, color), (planes, dev) in ragged.items():
        layouts = [(0, 0), (0, 7 if bpp == 24 else 2 * px), (px, 0)]         # packed; a pitch above the row; one pixel into the allocation
        if render_ref.refused(bpp, doubled, w, h, color):
            # the reference's loops would not fill this surface: refused through the return value, nothing written
            s = surface_for(name, w, h)
            with pytest.raises(fiasco_amd.FiascoError) as e:
                fiasco_amd.render_planes_device(gpu, renderers[name], dev, s.view)
            assert "unwritten" in str(e.value) and s.untouched(), (w, h, color)
            refused += 1
            continue
        want = render_ref.render_named(planes, name).tobytes()
        for lead, extra in layouts:
            s = surface_for(name, w, h, lead, extra)
            fiasco_amd.render_planes_device(gpu, renderers[name], dev, s.view)
            got, clean = s.rows()
            assert got == want and clean, (w, h, color, lead, extra)
            seen += 1
    assert seen + 3 * refused == 3 * len(ragged) and seen >= 6
    assert (refused > 0) == (bpp == 24 or (bpp == 16 and not doubled))


def test_device_host_and_numpy_agree_on_full_range_planes(gpu, renderers):
    rng = np.random.RandomState(64)
    for color in (False, True):
        planes = rng.randint(-32768, 32768, size=(3, 4, 64) if color else (4, 64)).astype(np.int16)
        planes.reshape(-1)[:6] = [-32768, 32767, -2049, 2047, -2064, 2048]
        dev = to_gpu(planes)
        for n in NAMES:
            s = surface_for(n, 64, 4)
            fiasco_amd.render_planes_device(gpu, renderers[n], dev, s.view)
            got, clean = s.rows()
            assert clean and got == renderers[n].render_planes(planes) == render_ref.render_named(planes, n).tobytes(), (color, n)


# ------------------------------------------------------------------ 2. staged batches

@pytest.fixture(scope="module")
def coded(gpu, inputs):
    """per coded case of the fixture: the frame coded on the device, as a finished batch of one; made once and left alone"""
    out, keep = {}, []
    shown = shown_ref.fixture_cases()
    for name, e in render_ref.fixture()["decoded"].items():
        b, o = shown_ref.staged(gpu, inputs, shown[name])
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == e["stream_md5"], (name, gpu.error_message())
        out[name] = (e, shown[name], b)
        keep.append(o)
    yield out
    for _, _, b in out.values():
        b.free()
    for o in keep:
        o.delete()


@pytest.mark.parametrize("name", sorted(render_ref.fixture()["decoded"]))
def test_decode_rendered_gives_the_references_bytes(gpu, renderers, coded, name):
    e, ent, b = coded[name]
    seen = 0
    for m, rec in sorted(e["rendered"].items()):
        w, h = rec["width"], rec["height"]
        planes = b.decode_planes(0, magnify=int(m))             # the unsmoothed decoder, on the host
        planes = planes if e["color"] else planes[0]
        for n in NAMES:
            for s in ("0", "-1"):
                want = rec["md5"][s][n]
                t = surface_for(n, w, h)
                if want == "refused":
                    with pytest.raises(fiasco_amd.FiascoError) as err:
                        b.decode_rendered(renderers[n], [t.view], magnify=int(m), smoothing=int(s))
                    assert "unwritten" in str(err.value) and t.untouched(), (name, m, n)
                    continue
                assert b.decode_rendered(renderers[n], [t.view], magnify=int(m), smoothing=int(s)) == 1, (name, m, n, s, gpu.error_message())
                got, clean = t.rows()
                assert md5(got) == want and clean, (name, m, n, s)
                seen += 1
            # the host loop on the device decoder's planes: the reference's bytes at every magnification
            if rec["md5"]["0"][n] != "refused":
                assert md5(renderers[n].render_planes(planes)) == rec["md5"]["0"][n], (name, m, n)
    assert seen >= 60


@pytest.mark.parametrize("name", ["g100x70", "carry74_a"])
def test_numpy_smoothing_and_numpy_rendering_give_the_same_bytes(gpu, coded, name):
    """independent of the smoothing and the rendering kernels: decode_planes(magnify) is the unsmoothed decoder, the blend and
    the pixels are numpy's"""
    e, ent, b = coded[name]
    for m, rec in sorted(e["rendered"].items()):
        planes = b.decode_planes(0, magnify=int(m))
        borders = b.smoothing_borders(0, magnify=int(m))
        smoothed = smooth_ref.smooth_planes(planes, borders, ent["smoothing"])
        for s, p in (("0", planes), ("-1", smoothed)):
            p = p if e["color"] else p[0]
            for n in NAMES:
                if rec["md5"][s][n] != "refused":
                    assert md5(render_ref.render_named(p, n).tobytes()) == rec["md5"][s][n], (name, m, s, n)


def test_one_flight_of_mixed_sizes_with_a_skipped_frame(gpu, renderers):
    rng = np.random.default_rng(5)
    frames = [synth.synth(96, 64, 31), rng.integers(0, 256, (96, 128, 3)).astype(np.uint8), synth.noise(100, 70, 9),
              rng.integers(0, 256, (64, 96, 3)).astype(np.uint8), synth.synth(64, 32, 33)]
    o = gpu.cli_options()
    b = fiasco_amd.Batch.from_device(gpu, [to_gpu(a) for a in frames], 20.0, o)
    assert None not in b.encode(), gpu.error_message()
    planes = [b.decode_planes(i) for i in range(5)]
    for n in ("rgb565", "xrgb8888_x2", "bgr24", "rgb24_x2", "xbgr8888_blue_quirk"):
        bpp = render_ref.RENDERERS[n][0]
        ts = [surface_for(n, w, h, lead=(bpp // 8 if i == 2 else 0), extra=(16 if i == 3 else 0)) for i, (w, h, _) in enumerate(b._geom)]
        assert b.decode_rendered(renderers[n], [t.view if i != 1 else None for i, t in enumerate(ts)], smoothing=0) == 4, (n, gpu.error_message())
        assert ts[1].untouched(), n
        for i in (0, 2, 3, 4):
            got, clean = ts[i].rows()
            p = planes[i] if planes[i].shape[0] == 3 else planes[i][0]
            assert clean and got == render_ref.render_named(p, n).tobytes(), (n, i)
    # smoothed at the header's value: what decode_shown writes, rendered
    ts = [surface_for("xrgb8888", w, h) for w, h, _ in b._geom]
    assert b.decode_rendered(renderers["xrgb8888"], [t.view for t in ts]) == 5
    for i in range(5):
        smoothed = smooth_ref.smooth_planes(planes[i], b.smoothing_borders(i), 70)
        p = smoothed if smoothed.shape[0] == 3 else smoothed[0]
        assert ts[i].rows() == (render_ref.render_named(p, "xrgb8888").tobytes(), True), i
    b.free(); o.delete()


def test_refused_frame_fails_alone_and_refused_calls_write_nothing(gpu, renderers, inputs):
    ent = shown_ref.fixture_cases()["g256_z1_q300"]
    q, o = options_from_args(gpu, ent["args"])
    y, x = np.mgrid[0:256, 0:256]
    ramp, diag = x.astype(np.uint8), ((x + y) // 2).astype(np.uint8)
    b = fiasco_amd.Batch(gpu, [synth.pgm_bytes(ramp), inputs.data("g256"), synth.pgm_bytes(diag)], q, o)
    assert None not in b.encode(), gpu.error_message()
    r = renderers["rgb565_x2"]
    ts = [surface_for("rgb565_x2", 32, 32) for _ in range(3)]
    assert b.decode_rendered(r, [t.view for t in ts], magnify=-3, smoothing=70) == 2
    msg = gpu.error_message()
    assert "<device target 1>" in msg and "magnification -3" in msg and "level 5 falls to level -1" in msg, msg
    assert ts[1].untouched()
    for i in (0, 2):
        planes = b.decode_planes(i, magnify=-3)
        want = render_ref.render_named(smooth_ref.smooth_planes(planes, b.smoothing_borders(i, magnify=-3), 70)[0], "rgb565_x2").tobytes()
        assert ts[i].rows() == (want, True), i
    # refused calls: every surface untouched
    ts = [surface_for("rgb565_x2", 64, 64), surface_for("rgb565_x2", 64, 64), surface_for("rgb565_x2", 32, 32)]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered(r, [t.view for t in ts], magnify=-2, smoothing=70)            # the last surface has another size
    assert "<device surface 2>" in str(e.value) and "128 x 128" in str(e.value) and all(t.untouched() for t in ts)
    not_doubled = [surface_for("rgb565", 64, 64) for _ in range(3)]                     # the size of the frame, not of the doubled surface
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered(r, [t.view for t in not_doubled], magnify=-2)
    assert "<device surface 0>" in str(e.value) and all(t.untouched() for t in not_doubled)
    ts = [surface_for("rgb565_x2", 64, 64) for _ in range(3)]
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered(renderers["xrgb8888_x2"], [t.view for t in ts], magnify=-2)   # a renderer of another depth
    assert "is not H x W x 4" in str(e.value)
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_rendered(r, [t.view for t in ts], magnify=-4)                          # the size rule
    with pytest.raises(fiasco_amd.FiascoError):
        b.decode_rendered(r, [t.view for t in ts], magnify=-2, smoothing=101)
    host = np.zeros((128, 128, 2), dtype=np.uint8)
    host[:] = 0x5a

    class Raw:
        __cuda_array_interface__ = {"shape": host.shape, "typestr": "|u1", "data": (host.ctypes.data, False), "version": 3, "strides": None}
    with pytest.raises(fiasco_amd.FiascoError) as e:
        b.decode_rendered(r, [ts[0].view, Raw(), ts[2].view], magnify=-2)
    assert "<device surface 1>" in str(e.value) and "not in device memory" in str(e.value)
    assert (host == 0x5a).all() and all(t.untouched() for t in ts)
    # a surface whose rows leave its allocation, a pitch below the row, an odd address at 16 bpp
    class Short:          # 512 GB claimed at a tensor of 32 KB
        __cuda_array_interface__ = {"shape": (128, 128, 2), "typestr": "|u1", "data": (ts[1].buf.data_ptr(), False), "version": 3, "strides": (1 << 32, 2, 1)}

    class Odd:
        __cuda_array_interface__ = {"shape": (128, 128, 2), "typestr": "|u1", "data": (ts[1].buf.data_ptr() + 1, False), "version": 3, "strides": None}

    class Narrow:
        __cuda_array_interface__ = {"shape": (128, 128, 2), "typestr": "|u1", "data": (ts[1].buf.data_ptr(), False), "version": 3, "strides": (254, 2, 1)}
    for bad, word in ((Short, "beyond the end of their device allocation"), (Odd, "aligned"), (Narrow, "smaller than a row")):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_rendered(r, [ts[0].view, bad(), ts[2].view], magnify=-2)
        assert "<device surface 1>" in str(e.value) and word in str(e.value), str(e.value)
    assert all(t.untouched() for t in ts)
    # the kernel alone refuses the same way
    planes = to_gpu(np.zeros((64, 64), dtype=np.int16))
    for bad in (Short, Odd, Narrow, Raw):
        with pytest.raises(fiasco_amd.FiascoError):
            fiasco_amd.render_planes_device(gpu, r, planes, bad())
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.render_planes_device(gpu, r, planes, surface_for("rgb565_x2", 64, 32).view)
    assert "<device surface 0>" in str(e.value)
    assert all(t.untouched() for t in ts) and (host == 0x5a).all()
    b.free(); o.delete()


def test_work_queued_behind_the_call_sees_the_pixels_without_host_synchronisation(gpu, renderers):
    o = gpu.cli_options()
    host = np.stack([synth.synth(96, 64, 70 + i) for i in range(4)])
    frames = list(to_gpu(host))
    torch.cuda.synchronize()
    b = fiasco_amd.Batch.from_device(gpu, frames, 20.0, o)
    assert None not in b.encode()
    r = renderers["xrgb8888"]
    want = [torch.empty((64, 96, 4), dtype=torch.uint8, device="cuda") for _ in range(4)]
    assert b.decode_rendered(r, want) == 4
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        targets = [torch.empty_like(t) for t in want]
        for t in targets:
            t.fill_(7)                                  # the rendering must wait for this
        assert b.decode_rendered(r, targets) == 4       # stream: torch's current one, the side stream
        got = [t.clone() for t in targets]              # reads on the side stream, no host synchronisation
    side.synchronize()
    for g, t in zip(got, want):
        assert torch.equal(g, t)
    with torch.cuda.stream(side):
        for t in targets:
            t.fill_(9)
    assert b.decode_rendered(r, targets, stream=side.cuda_stream) == 4      # an explicit stream handle does the same
    with torch.cuda.stream(side):
        got = [t.clone() for t in targets]
    side.synchronize()
    for g, t in zip(got, want):
        assert torch.equal(g, t)
    assert not any(bool((t == 9).all()) for t in got)
    b.free(); o.delete()
