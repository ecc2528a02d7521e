"""Frames decoded in 4:2:0 in the pixel formats of a display (include/libfiasco_amd_render_420.h; csrc/hip/render_420.inc), on
the device: the kernel alone against the REAL reference's bytes on the hand-made planes of tests/golden/RENDERED_420.json;
against the host loop at ragged widths on packed, pitched and offset surfaces, every byte outside the rows untouched; device
== host loop == numpy on full-range planes; decode_rendered_420 against the reference's bytes for the coded cases at every
recorded magnification and smoothing under all twelve renderers; two flights of mixed sizes with a skipped frame, the flat
frame and a gray frame failing alone; the relations to decode_planes_420 and decode_420; the call repeated and on two shares
of one device; ordering against the caller's stream."""
import hashlib
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import render420_ref
import render_ref
import yuv420_ref

pytestmark = pytest.mark.gpu

NAMES = sorted(render_ref.RENDERERS)
WIDTHS, HEIGHTS = (2, 4, 14, 16, 18, 30, 32, 34, 36, 66), (2, 6)


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
    seen = 0
    for key, e in render420_ref.fixture()["handmade"]["planes"].items():
        w, h = e["width"], e["height"]
        planes = render420_ref.handmade(w, h)
        assert [md5(p.tobytes()) for p in planes] == e["planes_md5"], key
        dev = [to_gpu(p) for p in planes]
        for n in NAMES:
            s = surface_for(n, w, h)
            if n not in e["renderers"]:
                with pytest.raises(fiasco_amd.FiascoError) as err:
                    fiasco_amd.render_planes_device_420(gpu, renderers[n], dev[0], dev[1], dev[2], s.view)
                assert "not a multiple of 4" in str(err.value) and s.untouched(), (key, n)
                continue
            fiasco_amd.render_planes_device_420(gpu, renderers[n], dev[0], dev[1], dev[2], s.view)
            got, clean = s.rows()
            rec = e["renderers"][n]
            if "bytes_zlib_b64" in rec:
                assert got == yuv420_ref.unpack(rec["bytes_zlib_b64"]), (key, n)
            assert md5(got) == rec["md5"] and clean, (key, n)
            seen += 1
    assert seen == 22


@pytest.fixture(scope="module")
def ragged():
    """(w, h) -> full-range int16 planes on the host and on the device, made once and left alone"""
    rng = np.random.RandomState(420)
    out = {}
    for w in WIDTHS:
        for h in HEIGHTS:
            planes = []
            for shape in ((h, w), (h // 2, w // 2), (h // 2, w // 2)):
                p = rng.randint(-4096, 4096, size=shape).astype(np.int16)
                p.reshape(-1)[::5] = rng.randint(-32768, 32768, size=p.reshape(-1)[::5].shape)
                planes.append(p)
            dev = [to_gpu(p) for p in planes]
            for p in planes:
                p.setflags(write=False)
            out[w, h] = (planes, dev)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_kernel_at_ragged_widths_on_packed_pitched_and_offset_surfaces(gpu, renderers, ragged, name):
    bpp, _, _, _, doubled = render_ref.RENDERERS[name]
    px = bpp // 8
    seen = refused = 0
    for (w, h), (planes, dev) in ragged.items():
        layouts = [(0, 0), (0, 7 if bpp == 24 else 2 * px), (px, 0)]         # packed; a pitch above the row; one pixel into the allocation
        if render420_ref.refused(bpp, doubled, w, h):
            s = surface_for(name, w, h)
            with pytest.raises(fiasco_amd.FiascoError) as e:
                fiasco_amd.render_planes_device_420(gpu, renderers[name], dev[0], dev[1], dev[2], s.view)
            assert "not a multiple of 4" in str(e.value) and s.untouched(), (w, h)
            refused += 1
            continue
        want = renderers[name].render_planes_420(*planes)
        assert want == render420_ref.render_named(*planes, name).tobytes(), (w, h)
        for lead, extra in layouts:
            s = surface_for(name, w, h, lead, extra)
            fiasco_amd.render_planes_device_420(gpu, renderers[name], dev[0], dev[1], dev[2], s.view)
            got, clean = s.rows()
            assert got == want and clean, (w, h, lead, extra)
            seen += 1
    assert seen + 3 * refused == 3 * len(ragged) and seen >= 24
    assert refused == (12 if bpp == 24 and not doubled else 0)


def test_odd_sizes_and_bad_planes_are_refused_and_nothing_is_written(gpu, renderers):
    r = renderers["xrgb8888"]
    y, c = to_gpu(np.zeros((6, 36), dtype=np.int16)), to_gpu(np.zeros((3, 18), dtype=np.int16))
    s = surface_for("xrgb8888", 36, 4)
    with pytest.raises(fiasco_amd.FiascoError) as e:
        fiasco_amd.render_planes_device_420(gpu, r, y, c, c, s.view)
    assert "<device surface 0>" in str(e.value) and s.untouched()
    L = gpu.L
    arr = fiasco_amd._device_surfaces([surface_for("xrgb8888", 35, 6).view], 32)
    assert L.fiasco_amd_planes_render_device_420(y.data_ptr(), c.data_ptr(), c.data_ptr(), 35, 6, r.handle, arr, None) == 0 and "is odd" in gpu.error_message()
    # a plane in host memory, whichever of the three it is
    host = np.zeros((6, 36), dtype=np.int16)
    s = surface_for("xrgb8888", 36, 6)
    arr = fiasco_amd._device_surfaces([s.view], 32)
    for k in range(3):
        ptrs = [y.data_ptr(), c.data_ptr(), c.data_ptr()]
        ptrs[k] = host.ctypes.data
        assert L.fiasco_amd_planes_render_device_420(ptrs[0], ptrs[1], ptrs[2], 36, 6, r.handle, arr, None) == 0
        assert "device memory" in gpu.error_message() and s.untouched(), (k, gpu.error_message())


def test_device_host_and_numpy_agree_on_full_range_planes(gpu, renderers):
    rng = np.random.RandomState(64)
    y = rng.randint(-32768, 32768, size=(4, 64)).astype(np.int16)
    cb, cr = (rng.randint(-32768, 32768, size=(2, 32)).astype(np.int16) for _ in range(2))
    for p in (y, cb, cr):
        p.reshape(-1)[:6] = [-32768, 32767, -2049, 2047, -2064, 2048]
    dev = [to_gpu(p) for p in (y, cb, cr)]
    for n in NAMES:
        s = surface_for(n, 64, 4)
        fiasco_amd.render_planes_device_420(gpu, renderers[n], dev[0], dev[1], dev[2], s.view)
        got, clean = s.rows()
        assert clean and got == renderers[n].render_planes_420(y, cb, cr) == render420_ref.render_named(y, cb, cr, n).tobytes(), n


# ------------------------------------------------------------------ 2. staged batches

@pytest.fixture(scope="module")
def coded(gpu, inputs):
    """per coded case of the fixture: the frame coded on the device, as a finished batch of one; made once and left alone"""
    out, keep = {}, []
    cases = yuv420_ref.fixture_cases()
    for name, e in render420_ref.fixture()["decoded"].items():
        b, o = yuv420_ref.staged(gpu, inputs, cases[name])
        stream = b.encode()[0]
        assert stream is not None and hashlib.md5(stream).hexdigest() == e["stream_md5"], (name, gpu.error_message())
        out[name] = (e, cases[name], b)
        keep.append(o)
    yield out
    for _, _, b in out.values():
        b.free()
    for o in keep:
        o.delete()


@pytest.mark.parametrize("name", sorted(n for n, e in render420_ref.fixture()["decoded"].items() if not e["degenerate"]))
def test_decode_rendered_420_gives_the_references_bytes(gpu, renderers, coded, name):
    e, ent, b = coded[name]
    seen = refused = 0
    for m, rec in sorted(e["rendered"].items()):
        w, h = rec["width"], rec["height"]
        planes = b.decode_planes_420(0, magnify=int(m))         # the unsmoothed decoder, on the host
        for n in NAMES:
            for s in ("0", "-1"):
                want = rec["md5"][s][n]
                t = surface_for(n, w, h)
                if want == "refused":
                    with pytest.raises(fiasco_amd.FiascoError) as err:
                        b.decode_rendered_420(renderers[n], [t.view], magnify=int(m), smoothing=int(s))
                    assert "not a multiple of 4" in str(err.value) and t.untouched(), (name, m, n)
                    refused += 1
                    continue
                assert b.decode_rendered_420(renderers[n], [t.view], magnify=int(m), smoothing=int(s)) == 1, (name, m, n, s, gpu.error_message())
                got, clean = t.rows()
                assert md5(got) == want and clean, (name, m, n, s)
                seen += 1
            # at smoothing 0 the surface is the host loop on decode_planes_420
            if rec["md5"]["0"][n] != "refused":
                assert md5(renderers[n].render_planes_420(*planes)) == rec["md5"]["0"][n], (name, m, n)
    assert seen >= 40 and (refused > 0) == (name != "carry48_a")
    # the size rule's refusals are the call's, nothing written
    if ent["decoded"]["0"]["below_refused"]:
        t = surface_for("xrgb8888", ent["width"], ent["height"])
        with pytest.raises(fiasco_amd.FiascoError) as err:
            b.decode_rendered_420(renderers["xrgb8888"], [t.view], magnify=-1)
        assert "Minimum value is 0." in str(err.value) and t.untouched()


def test_the_flat_frame_and_a_surface_of_the_wrong_size_are_refused(gpu, renderers, coded):
    e, ent, b = coded["flat64"]
    t = surface_for("xrgb8888", 64, 64)
    with pytest.raises(fiasco_amd.FiascoError) as err:
        b.decode_rendered_420(renderers["xrgb8888"], [t.view])
    assert "max_level" in str(err.value) and t.untouched()
    _, _, b = coded["c34"]
    for n, (w, h) in (("xrgb8888_x2", (34, 34)), ("xrgb8888", (36, 34)), ("rgb565", (34, 36))):
        bpp, doubled = render_ref.RENDERERS[n][0], render_ref.RENDERERS[n][4]
        t = Surface(w, h, bpp // 8)                 # the frame's size where the doubled one is due; a wrong width; a wrong height
        with pytest.raises(fiasco_amd.FiascoError) as err:
            b.decode_rendered_420(renderers[n], [t.view])
        assert "<device surface 0>" in str(err.value) and ("68 x 68" if doubled else "34 x 34") in str(err.value) and t.untouched(), str(err.value)


def test_two_flights_of_mixed_sizes_with_a_skipped_a_flat_and_a_gray_frame(gpu, renderers, inputs):
    """34 frames -- two flights of 32 -- of two small cases at `cfiasco' defaults; frame 17 is the flat one and frame 20 a gray
    one: each fails alone with its message, the others are written, the None surface is skipped"""
    cases = yuv420_ref.fixture_cases()
    fx = render420_ref.fixture()["decoded"]
    names = ["c34" if i % 2 else "c102x66" for i in range(34)]
    names[17] = "flat64"
    frames = [yuv420_ref.synth_input(cases[n]["input"])[0] for n in names]
    frames[20] = inputs.data("g96x64")
    sizes = [(cases[n]["width"], cases[n]["height"]) for n in names]
    sizes[20] = (96, 64)
    o = gpu.cli_options()
    o.set_smoothing(70)
    b = fiasco_amd.Batch(gpu, frames, 20.0, o)
    streams = b.encode()
    assert all(s is not None for s in streams), gpu.error_message()
    assert all(hashlib.md5(s).hexdigest() == cases[n]["stream_md5"] for i, (s, n) in enumerate(zip(streams, names)) if i != 20)
    skipped, failing = {3, 32}, {17, 20}
    for n in ("xrgb8888", "rgb565_x2"):
        bpp = render_ref.RENDERERS[n][0]
        ts = [surface_for(n, w, h, lead=(bpp // 8 if i % 7 == 2 else 0), extra=(16 if i % 5 == 0 else 0)) for i, (w, h) in enumerate(sizes)]
        good = b.decode_rendered_420(renderers[n], [None if i in skipped else t.view for i, t in enumerate(ts)])
        assert good == 34 - len(skipped) - len(failing), (n, good, gpu.error_message())
        msg = gpu.error_message()
        assert "<device target 20>" in msg and "gray frame" in msg, msg         # the last frame that failed is named
        for i, (t, name) in enumerate(zip(ts, names)):
            if i in skipped or i in failing:
                assert t.untouched(), (n, i)
                continue
            got, clean = t.rows()
            assert md5(got) == fx[name]["rendered"]["0"]["md5"]["-1"][n] and clean, (n, i, name)
    # each failing frame alone: the call has nothing to write and says why
    for i, word in ((17, "max_level"), (20, "gray frame")):
        only = [None] * 34
        t = surface_for("xrgb8888", *sizes[i])
        only[i] = t.view
        with pytest.raises(fiasco_amd.FiascoError) as e:
            b.decode_rendered_420(renderers["xrgb8888"], only)
        assert word in str(e.value) and "<device target %d>" % i in str(e.value) and t.untouched(), str(e.value)
    b.free(); o.delete()


# ------------------------------------------------------------------ 3. against the other 4:2:0 paths

@pytest.mark.parametrize("smoothing", [0, -1, 35])
def test_y_bytes_agree_with_decode_420_through_the_numpy_model(gpu, renderers, coded, smoothing):
    """decode_420 into I420 and decode_rendered_420 of the same batch, through the numpy model on planes rebuilt from the
    I420 bytes as (byte - 128) << 4.  The renderer drops the four fraction bits first and clamps the chroma to -128 .. 127,
    which is the clip of the chroma bytes, so the rebuilt planes render to the same pixel wherever the Y byte was not
    clipped (0 < byte < 255); the pixels are compared there, and most pixels must be of that kind"""
    e, ent, b = coded["c102x66"]
    w, h = ent["width"], ent["height"]
    y8 = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    cb8, cr8 = (torch.empty((h // 2, w // 2), dtype=torch.uint8, device="cuda") for _ in range(2))
    assert b.decode_420([(y8, cb8, cr8)], smoothing=smoothing) == 1
    planes = [(p.cpu().numpy().astype(np.int16) - 128) << 4 for p in (y8, cb8, cr8)]
    told = (y8.cpu().numpy() > 0) & (y8.cpu().numpy() < 255)
    assert told.mean() > 0.5
    for n in ("xrgb8888", "rgb565_x2", "bgr24_x2"):
        bpp, doubled = render_ref.RENDERERS[n][0], render_ref.RENDERERS[n][4]
        t = surface_for(n, w, h)
        assert b.decode_rendered_420(renderers[n], [t.view], smoothing=smoothing) == 1
        got, clean = t.rows()
        want = render420_ref.render_named(planes[0], planes[1], planes[2], n)
        got = np.frombuffer(got, dtype=np.uint8).reshape(want.shape)
        mask = told.repeat(2, 0).repeat(2, 1) if doubled else told
        assert clean and np.array_equal(got[mask], want[mask]), (n, smoothing)


# ------------------------------------------------------------------ 4. again, on two shares of one device, and the stream

def test_the_call_twice_in_a_row_and_with_the_device_listed_twice(gpu, renderers, coded):
    e, ent, b = coded["carry74_a"]
    rec = e["rendered"]["0"]
    for _ in range(2):
        t = surface_for("rgb565_x2", rec["width"], rec["height"])
        assert b.decode_rendered_420(renderers["rgb565_x2"], [t.view]) == 1
        got, clean = t.rows()
        assert md5(got) == rec["md5"]["-1"]["rgb565_x2"] and clean
    cases = yuv420_ref.fixture_cases()
    fx = render420_ref.fixture()["decoded"]
    names = ["c34", "c102x66", "c34", "c102x66", "c34"]
    o = gpu.cli_options()
    o.set_smoothing(70)
    gpu.set_devices([0, 0])
    try:
        assert gpu.device_count() == 2
        b2 = fiasco_amd.Batch(gpu, [yuv420_ref.synth_input(cases[n]["input"])[0] for n in names], 20.0, o)
        assert None not in b2.encode(), gpu.error_message()
        for n in ("xrgb8888_x2", "rgb555"):
            ts = [surface_for(n, cases[c]["width"], cases[c]["height"], extra=8 if i == 1 else 0) for i, c in enumerate(names)]
            assert b2.decode_rendered_420(renderers[n], [t.view for t in ts], smoothing=0) == 5, gpu.error_message()
            for t, c in zip(ts, names):
                got, clean = t.rows()
                assert md5(got) == fx[c]["rendered"]["0"]["md5"]["0"][n] and clean, (n, c)
        b2.free()
    finally:
        gpu.set_devices([])
        o.delete()


def test_work_queued_behind_the_call_sees_the_pixels_without_host_synchronisation(gpu, renderers):
    cases = yuv420_ref.fixture_cases()
    o = gpu.cli_options()
    o.set_smoothing(70)
    b = fiasco_amd.Batch(gpu, [yuv420_ref.synth_input(cases["c102x66"]["input"])[0] for _ in range(4)], 20.0, o)
    assert None not in b.encode()
    r = renderers["xrgb8888"]
    want = [torch.empty((66, 102, 4), dtype=torch.uint8, device="cuda") for _ in range(4)]
    assert b.decode_rendered_420(r, want) == 4
    torch.cuda.synchronize()
    assert md5(want[0].cpu().numpy().tobytes()) == render420_ref.fixture()["decoded"]["c102x66"]["rendered"]["0"]["md5"]["-1"]["xrgb8888"]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        targets = [torch.empty_like(t) for t in want]
        for t in targets:
            t.fill_(7)                                  # the rendering must wait for this
        assert b.decode_rendered_420(r, targets) == 4   # stream: torch's current one, the side stream
        got = [t.clone() for t in targets]              # reads on the side stream, no host synchronisation
    side.synchronize()
    for g, t in zip(got, want):
        assert torch.equal(g, t)
    with torch.cuda.stream(side):
        for t in targets:
            t.fill_(9)
    assert b.decode_rendered_420(r, targets, stream=side.cuda_stream) == 4      # an explicit stream handle does the same
    with torch.cuda.stream(side):
        got = [t.clone() for t in targets]
    side.synchronize()
    for g, t in zip(got, want):
        assert torch.equal(g, t)
    b.free(); o.delete()
