"""The decoder half of fiasco.h on the device -- run on a real MI355X: -m gpu.  (include/libfiasco_amd_decoder.h;
csrc/host/fa_decoder.c, the cursor of fa_stream.c, csrc/hip/decoder_outlet.inc and the planes outlet of frame_decoder.inc.)

Yardsticks, all compared with ==:
  tests/golden/DECODED_STREAMS.json: per stream, display frame, magnification, format and smoothing the md5 of the 12.4 planes
    the REFERENCE's fiasco_decoder_get_frame hands out -- here for EVERY tuple, the smoothed ones (-1 and 35) included, which
    no outlet before this one could be compared with -- and of the bytes its PNM writer writes;
  tests/golden/DECODER_API.json (tests/golden/make_decoder_api.py): the whole PNM files of fiasco_decoder_write_frame and the
    XImages of fiasco_renderer_render;
  the library's own host renderer on the planes of the same image.
No frame is larger than 256 x 256 (512 x 512 magnified), no video longer than 5 frames."""
import hashlib
import json
import os
import threading

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch            # before the product library is loaded: one HIP runtime for both

import fiasco_amd
import render_ref
import stream_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FIX = sc.fixture()
API = json.load(open(os.path.join(GOLDEN, "DECODER_API.json")))


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def md5(data):
    return hashlib.md5(data).hexdigest()


def planes_md5(image):
    p = image.planes()
    return md5(b"".join(np.ascontiguousarray(a, "<i2").tobytes() for a in (p if isinstance(p, tuple) else [p])))


def play(lib, data, **options):
    """[planes md5 of every display frame] through a get_frame loop"""
    d = fiasco_amd.Decoder(lib, data, **options)
    got = []
    for image in d:
        got.append(planes_md5(image))
        image.delete()
    assert len(got) == d.length
    d.delete()
    return got


def test_the_fixture_leaves_nothing_out():
    assert FIX["left_out"] == {} and API["left_out"] == {}
    assert sum(len(FIX["streams"][n]["decoded"]) for n in sc.NAMES) == 207 and len(sc.NAMES) == 17


@pytest.mark.parametrize("name", sc.NAMES)
def test_every_tuple_as_the_reference_decoder_hands_it_out(gpu, name, tmp_path):
    """every (magnification, format, smoothing) of the fixture through a get_frame loop: the planes of every frame; the
    4:4:4 tuples through write_frame as well: the payload and, where DECODER_API.json has it, the whole file"""
    rec = FIX["streams"][name]
    data = sc.stream_bytes(name)
    seen = 0
    for key, ent in sorted(rec["decoded"].items()):
        m, fmt, smoothing = sc.parse_key(key)
        if "refused" in ent:
            with pytest.raises(fiasco_amd.FiascoError) as e:
                fiasco_amd.Decoder(gpu, data, smoothing=smoothing, magnify=m, format_420=fmt == "420")
            assert str(e.value) == ent["refused"], (name, key)
            continue
        assert play(gpu, data, smoothing=smoothing, magnify=m, format_420=fmt == "420") == [f["planes_md5"] for f in ent["frames"]], (name, key)
        seen += 1
        if fmt != "444":
            continue
        d = fiasco_amd.Decoder(gpu, data, smoothing=smoothing, magnify=m, format_420=True)       # write_frame decodes 4:4:4 whatever the options say
        whole = API["written"].get(name, {}).get("%d:%d" % (m, smoothing))
        for k, f in enumerate(ent["frames"]):
            path = tmp_path / ("%s.%d.pnm" % (key.replace(":", "_"), k))
            d.write_frame(path)
            got = path.read_bytes()
            header = b"%s\n%d %d\n255\n" % (b"P6" if d.color else b"P5", ent["width"], ent["height"])
            assert got.startswith(header) and md5(got[len(header):]) == f["pixels_md5"], (name, key, k)
            if whole:
                assert (md5(got), len(got)) == (whole["files"][k]["md5"], whole["files"][k]["bytes"]), (name, key, k)
        with pytest.raises(fiasco_amd.FiascoError, match="no such frame"):
            d.write_frame(tmp_path / "behind_the_end.pnm")
        d.delete()
    assert seen, name


def test_a_gray_stream_with_the_420_option_set(gpu):
    """the reference hands out a gray frame of the coded size that is neither the 4:4:4 frame nor any other tuple's (it shrinks
    every state by a level, the initial basis included): recorded in the fixture, refused here as the stream entries refuse
    it; nothing is consumed, and write_frame, which decodes 4:4:4, goes on"""
    theirs = API["gray_420"]["seq4_gray_ibbp"]["frames"]
    known = {f["planes_md5"] for ent in FIX["streams"]["seq4_gray_ibbp"]["decoded"].values() for f in ent.get("frames", [])}
    assert len(theirs) == 4 and all(f["format"] == 0 and f["color"] == 0 and f["planes_md5"] not in known for f in theirs)
    d = fiasco_amd.Decoder(gpu, sc.stream_bytes("seq4_gray_ibbp"), smoothing=-1, format_420=True)
    for _ in range(2):
        with pytest.raises(fiasco_amd.FiascoError, match="4:2:0: a gray frame has no chroma bands"):
            d.get_frame()
    assert d.position == 0
    d.delete()


@pytest.mark.parametrize("name", [sc.IPBBP, sc.IBBP_B0, "seq3_color_carry74"])
def test_read_ahead_changes_nothing(gpu, name):
    """1: one display frame per device call; 2: windows that end inside a run of B frames (and, for the all-intra stream,
    before an I frame); 32: the whole stream in the walk's flights"""
    data = sc.stream_bytes(name)
    for m, fmt, s in ((0, "444", -1), (1, "420", 35), (0, "420", 0)):
        want = [f["planes_md5"] for f in FIX["streams"][name]["decoded"][sc.key_of(m, fmt, s)]["frames"]]
        for ahead in (1, 2, 32):
            assert play(gpu, data, smoothing=s, magnify=m, format_420=fmt == "420", read_ahead=ahead) == want, (name, m, fmt, s, ahead)


@pytest.mark.parametrize("case", sorted(API["rendered"]))
def test_renderer_on_device_images(gpu, case):
    """fiasco_renderer_render on the images of get_frame: the reference's XImage (the fixture), and the host renderer of this
    library on the planes of the same image"""
    name, fmt = case.split(":")
    for rname, rec in sorted(API["rendered"][case].items()):
        bpp, red, green, blue, doubled = render_ref.RENDERERS[rname]
        r = fiasco_amd.Renderer(gpu, red, green, blue, bpp, doubled)
        d = fiasco_amd.Decoder(gpu, sc.stream_bytes(name), smoothing=-1, format_420=fmt == "420")
        assert len(rec["frames"]) == d.length and all(rec["frames"])
        for k, image in enumerate(d):
            got = image.render(r)
            planes = image.planes()
            host = r.render_planes_420(*planes) if image.format_420 else r.render_planes(planes if image.color else planes[0])
            assert got == host and md5(got) == rec["frames"][k], (case, rname, k)
            image.delete()
        d.delete(); r.delete()


def test_render_device_is_ordered_on_the_callers_stream(gpu):
    """the surface of render_device holds the bytes of render(), and so does a copy queued behind it on the caller's stream.
    The entry runs on that stream and waits for it on the host before it returns (fiasco_amd_planes_render_device), so this
    checks the bytes and that the caller's stream is the one used; a wrong ORDER could not show here"""
    r = fiasco_amd.Renderer(gpu, 0xff0000, 0x00ff00, 0x0000ff, 32)
    for fmt in (False, True):
        d = fiasco_amd.Decoder(gpu, sc.stream_bytes(sc.IPBBP), format_420=fmt)
        image = d.get_frame()
        sw, sh, row = image._surface_size(r)
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            surface = torch.full((sh, sw, 4), 7, dtype=torch.uint8, device="cuda")
            image.render_device(r, surface, stream=stream)
            behind = surface.clone()
        stream.synchronize()
        assert behind.cpu().numpy().tobytes() == image.render(r) == surface.cpu().numpy().tobytes()
        planes, device = image.device_planes()
        assert planes[0] and planes[1] and planes[2] and device == torch.cuda.current_device()
        image.delete(); d.delete()
    # an image that was read from a file is uploaded by the first call that needs its device planes
    im = fiasco_amd.Image.open(gpu, os.path.join(GOLDEN, "carry48_c.ppm"))
    surface = torch.zeros((im.height, im.width, 4), dtype=torch.uint8, device="cuda")
    im.render_device(r, surface)
    torch.cuda.synchronize()
    assert md5(surface.cpu().numpy().tobytes()) == API["images"]["carry48_c.ppm"]["ximage_md5"]["xrgb8888"] == md5(im.render(r))
    im.delete(); r.delete()


def test_images_outlive_their_decoder_and_a_decoder_goes_with_frames_outstanding(gpu):
    want = [f["planes_md5"] for f in FIX["streams"][sc.IPBBP]["decoded"][sc.key_of(0, "444", -1)]["frames"]]
    d = fiasco_amd.Decoder(gpu, sc.stream_bytes(sc.IPBBP), smoothing=-1, read_ahead=32)
    first, second = d.get_frame(), d.get_frame()        # the other three are decoded and never handed out
    d.delete()
    assert [planes_md5(first), planes_md5(second)] == want[:2]
    first.delete(); second.delete()
    d = fiasco_amd.Decoder(gpu, sc.stream_bytes(sc.IPBBP), smoothing=-1, read_ahead=1)
    held = d.get_frame()
    del d                                               # ... and collected with an image alive
    assert planes_md5(held) == want[0]
    held.delete()


def test_orphaned_b_frames_fail_and_are_consumed(gpu):
    d = fiasco_amd.Decoder(gpu, sc.orphaned_b_stream(), smoothing=0)
    assert d.length == 4
    d.get_frame().delete()
    with pytest.raises(fiasco_amd.FiascoError, match="display frame 1: .*motion vector without its reference frame"):
        d.get_frame()
    with pytest.raises(fiasco_amd.FiascoError, match="display frame 2: display frame 2 is predicted from frame 1, which failed"):
        d.get_frame()
    last = d.get_frame()
    assert (last.width, last.height) == (d.width, d.height)
    last.delete()
    assert d.position == 4                      # the failed frames were consumed
    with pytest.raises(fiasco_amd.FiascoError, match="no such frame"):
        d.get_frame()
    assert d.position == 4
    d.delete()


def test_images_that_went_give_their_buffers_to_the_frames_to_come(gpu):
    """a decoder played with one image alive at a time decodes into the buffer of the image before: the planes of a frame
    live at an address an earlier image had, and are the reference's all the same"""
    name = "seq3_color_carry74"
    want = [f["planes_md5"] for f in FIX["streams"][name]["decoded"][sc.key_of(0, "444", -1)]["frames"]]
    d = fiasco_amd.Decoder(gpu, sc.stream_bytes(name), smoothing=-1, read_ahead=1)
    got, seen = [], []
    for image in d:
        seen.append(image.device_planes()[0][0])
        got.append(planes_md5(image))
        image.delete()
    assert got == want and len(set(seen)) == 1, seen
    d.delete()


def test_two_decoders_on_two_threads_over_one_file(gpu):
    want = [f["planes_md5"] for f in FIX["streams"][sc.IBBP_B0]["decoded"][sc.key_of(0, "444", 35)]["frames"]]
    got, errors = [None, None], []

    def work(t):
        try:
            got[t] = play(gpu, sc.stream_path(sc.IBBP_B0), smoothing=35, read_ahead=1 + t)
        except Exception as e:          # noqa: BLE001
            errors.append(repr(e))
    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors and got == [want, want], errors
