"""Every refusal the Python binding raises on its own, before the C library is asked: the array descriptors
(fiasco_amd._device_frames, _device_targets, _device_targets_420, _ycbcr_frames, _device_surfaces, _packed_planes), the
module-level planes_* / render_planes_device* functions (called with lib=None: a refusal that touched the library would be an
AttributeError) and the argument checks of a Batch staged on the CPU oracle.  One table of (call, exact message): callers
match on these texts, so the descriptors may be restructured but the messages, and which of two refusals comes first, may
not move.  No device and no product library are needed."""
import types

import pytest

import fiasco_amd
from fiasco_amd import FiascoError

CUDA, HOST = "__cuda_array_interface__", "__array_interface__"


class Fake:
    """An object that shows one chosen array interface; strides="omit" leaves the key out."""
    def __init__(self, shape, typestr="|u1", strides=None, ptr=0x10000, readonly=False, iface=CUDA):
        d = {"shape": shape, "typestr": typestr, "data": (ptr, readonly), "version": 3, "strides": strides}
        if strides == "omit":
            del d["strides"]
        setattr(self, iface, d)


def I16(shape, **kw):
    return Fake(shape, "<i2", **kw)


Y, CB, CR, CBCR = Fake((4, 6)), Fake((2, 3), ptr=0x20000), Fake((2, 3), ptr=0x30000), Fake((2, 3, 2), ptr=0x20000)
HY, HCB, HCR = Fake((4, 6), iface=HOST), Fake((2, 3), iface=HOST), Fake((2, 3), iface=HOST)
PY, PCB, PCR = I16((4, 6)), I16((2, 3)), I16((2, 3))
R16, R32 = types.SimpleNamespace(bpp=16, handle=None), types.SimpleNamespace(bpp=32, handle=None)
S16, S32 = Fake((4, 6, 2)), Fake((4, 6, 4))

frames, targets, targets420 = fiasco_amd._device_frames, fiasco_amd._device_targets, fiasco_amd._device_targets_420
ycbcr, surfaces, packed = fiasco_amd._ycbcr_frames, fiasco_amd._device_surfaces, fiasco_amd._packed_planes

NO_CUDA = "not in device memory (no __cuda_array_interface__)"
ORDER = "order 'yv12' is neither \"nv12\" nor \"nv21\""
ADJACENT = "(the bytes of a pixel and the pixels of a row must be adjacent)"

REFUSALS = [
    # ---- _describe: frames and targets
    (lambda: frames([object()]), "frame 0 is " + NO_CUDA),
    (lambda: frames([Y, Fake((4, 6), iface=HOST)]), "frame 1 is " + NO_CUDA),
    (lambda: targets([None, object()]), "target 1 is " + NO_CUDA),
    (lambda: frames([Fake((4, 6), "<f4")]), "frame 0: 8-bit unsigned pixels expected, not <f4"),
    (lambda: targets([Fake((4, 6), "|i1")]), "target 0: 8-bit unsigned pixels expected, not |i1"),
    (lambda: frames([Fake((24,))]), "frame 0: shape (24,) is neither H x W, H x W x 3 nor 3 x H x W"),
    (lambda: frames([Fake((4, 6, 4))]), "frame 0: shape (4, 6, 4) is neither H x W, H x W x 3 nor 3 x H x W"),
    (lambda: targets([Fake((1, 3, 4, 6))]), "target 0: shape (1, 3, 4, 6) is neither H x W, H x W x 3 nor 3 x H x W"),
    (lambda: frames([Fake((4, 6), strides=(1, 4))]),
     "frame 0: strides (1, 4) cannot be described by pitch and plane stride (pixels of a row must be adjacent)"),
    (lambda: frames([Fake((4, 6, 3), strides=(24, 4, 1))]),
     "frame 0: strides (24, 4, 1) cannot be described by pitch and plane stride (R, G, B of a pixel and the pixels of a row "
     "must be adjacent)"),
    (lambda: frames([Fake((4, 6, 3), strides=(36, 3, 2))]),
     "frame 0: strides (36, 3, 2) cannot be described by pitch and plane stride (R, G, B of a pixel and the pixels of a row "
     "must be adjacent)"),
    (lambda: targets([Fake((3, 4, 6), strides=(48, 12, 2))]),
     "target 0: strides (48, 12, 2) cannot be described by pitch and plane stride (pixels of a row must be adjacent)"),
    (lambda: frames([Fake((4, 6), strides=(0, 1))]),
     "frame 0: strides (0, 1) cannot be described by pitch and plane stride (strides must be positive)"),
    (lambda: targets([Fake((4, 6), strides=(-6, 1))]),
     "target 0: strides (-6, 1) cannot be described by pitch and plane stride (strides must be positive)"),
    (lambda: frames([Fake((3, 4, 6), strides=(0, 6, 1))]),
     "frame 0: strides (0, 6, 1) cannot be described by pitch and plane stride (strides must be positive)"),
    (lambda: targets([Y, Fake((4, 6), readonly=True)]), "target 1 is read-only"),
    # ---- one plane of a 4:2:0 target
    (lambda: targets420([(object(), CB, CR)]), "target 0: the Y plane is " + NO_CUDA),
    (lambda: targets420([None, (Y, Fake((2, 3), iface=HOST), CR)]), "target 1: the Cb plane is " + NO_CUDA),
    (lambda: targets420([(Y, object())]), "target 0: the chroma plane is " + NO_CUDA),
    (lambda: targets420([(Y, Fake((2, 3), "<i2"), CR)]), "target 0: the Cb plane holds <i2, not bytes (uint8)"),
    (lambda: targets420([(Fake((4, 6, 1)), CB, CR)]), "target 0: the Y plane has shape (4, 6, 1), 2 dimensions expected"),
    (lambda: targets420([(Y, CB, Fake((6,)))]), "target 0: the Cr plane has shape (6,), 2 dimensions expected"),
    (lambda: targets420([(Y, Fake((2, 3)))]), "target 0: the chroma plane has shape (2, 3), 3 dimensions expected"),
    (lambda: targets420([(Fake((4, 6), strides=(12, 2)), CB, CR)]),
     "target 0: the strides (12, 2) of the Y plane cannot be described by a pitch"),
    (lambda: targets420([(Y, Fake((2, 3, 2), strides=(6, 1, 1)))]),
     "target 0: the strides (6, 1, 1) of the chroma plane cannot be described by a pitch"),
    (lambda: targets420([(Y, Fake((2, 3, 2), strides=(12, 4, 1)))]),
     "target 0: the strides (12, 4, 1) of the chroma plane cannot be described by a pitch"),
    (lambda: targets420([(Y, Fake((2, 3), strides=(0, 1)), CR)]),
     "target 0: the strides (0, 1) of the Cb plane cannot be described by a pitch"),
    (lambda: targets420([(Y, CB, Fake((2, 3), strides=(-3, 1)))]),
     "target 0: the strides (-3, 1) of the Cr plane cannot be described by a pitch"),
    (lambda: targets420([(Fake((4, 6), readonly=True), CB, CR)]), "target 0: the Y plane is read-only"),
    (lambda: targets420([(Y, CB, Fake((2, 3), readonly=True))]), "target 0: the Cr plane is read-only"),
    (lambda: targets420([(Y, Fake((2, 3, 2), readonly=True))]), "target 0: the chroma plane is read-only"),
    # ---- one plane of a YCbCr frame, in host and in device memory
    (lambda: ycbcr([(Y, CB, CR)], "nv12", HOST), "frame 0: the Y plane is not in host memory (no __array_interface__)"),
    (lambda: ycbcr([(HY, HCB, HCR)], "nv12", CUDA), "frame 0: the Y plane is " + NO_CUDA),
    (lambda: ycbcr([(Y, CB, CR), (Y, CB, object())], "nv12", CUDA), "frame 1: the Cr plane is " + NO_CUDA),
    (lambda: ycbcr([(HY, object())], "nv12", HOST), "frame 0: the chroma plane is not in host memory (no __array_interface__)"),
    (lambda: ycbcr([(Fake((4, 6), "<u2", iface=HOST), HCB, HCR)], "nv12", HOST), "frame 0: the Y plane holds <u2, not bytes (uint8)"),
    (lambda: ycbcr([(Y, Fake((2, 3, 1)), CR)], "nv12", CUDA), "frame 0: the Cb plane has shape (2, 3, 1), 2 dimensions expected"),
    (lambda: ycbcr([(Y, Fake((2, 3)))], "nv12", CUDA), "frame 0: the chroma plane has shape (2, 3), 3 dimensions expected"),
    (lambda: ycbcr([(Fake((4, 6), strides=(1, 4)), CB, CR)], "nv12", CUDA),
     "frame 0: the strides (1, 4) of the Y plane cannot be described by a pitch"),
    (lambda: ycbcr([(Y, Fake((2, 3, 2), strides=(6, 1, 1)))], "nv12", CUDA),
     "frame 0: the strides (6, 1, 1) of the chroma plane cannot be described by a pitch"),
    (lambda: ycbcr([(HY, HCB, Fake((2, 3), strides=(0, 1), iface=HOST))], "nv12", HOST),
     "frame 0: the strides (0, 1) of the Cr plane cannot be described by a pitch"),
    # ---- the (y, cb, cr) / (y, cbcr) tuples
    (lambda: targets420([(Y,)]), "target 0: (y, cb, cr) or (y, cbcr) expected, not 1 arrays"),
    (lambda: targets420([None, (Y, CB, CR, CR)]), "target 1: (y, cb, cr) or (y, cbcr) expected, not 4 arrays"),
    (lambda: ycbcr([(Y,)], "nv12", CUDA), "frame 0: (y, cb, cr) or (y, cbcr) expected, not 1 arrays"),
    (lambda: ycbcr([(HY, HCB, HCR), (HY, HCB, HCR, HCR)], "nv12", HOST), "frame 1: (y, cb, cr) or (y, cbcr) expected, not 4 arrays"),
    (lambda: targets420([(Y, Fake((2, 2)), CR)]), "target 0: chroma planes of (2, 2) and (3, 2) for a Y plane of 6 x 4 (3 x 2 expected)"),
    (lambda: targets420([(Y, CB, Fake((3, 3)))]), "target 0: chroma planes of (3, 2) and (3, 3) for a Y plane of 6 x 4 (3 x 2 expected)"),
    (lambda: targets420([(Y, Fake((4, 6)), Fake((4, 6)))]),           # 4:4:4 is no target
     "target 0: chroma planes of (6, 4) and (6, 4) for a Y plane of 6 x 4 (3 x 2 expected)"),
    (lambda: ycbcr([(Y, Fake((2, 2)), CR)], "nv12", CUDA),
     "frame 0: chroma planes of (2, 2) and (3, 2) for a Y plane of 6 x 4 (6 x 4 for 4:4:4 or 3 x 2 for 4:2:0 expected)"),
    (lambda: ycbcr([(Y, Fake((4, 6)), CR)], "nv12", CUDA),
     "frame 0: chroma planes of (6, 4) and (3, 2) for a Y plane of 6 x 4 (6 x 4 for 4:4:4 or 3 x 2 for 4:2:0 expected)"),
    (lambda: ycbcr([(Y, Fake((4, 3)), Fake((4, 3)))], "nv12", CUDA),  # 4:2:2 is not taken
     "frame 0: chroma planes of (3, 4) and (3, 4) for a Y plane of 6 x 4 (6 x 4 for 4:4:4 or 3 x 2 for 4:2:0 expected)"),
    (lambda: targets420([(Y, CB, Fake((2, 3), strides=(8, 1)))]), "target 0: the chroma planes have pitches 3 and 8 (one pitch expected)"),
    (lambda: ycbcr([(Y, Fake((2, 3), strides=(16, 1)), CR)], "nv12", CUDA),
     "frame 0: the chroma planes have pitches 16 and 3 (one pitch expected)"),
    (lambda: targets420([(Y, Fake((2, 2, 2)))]),
     "target 0: an interleaved chroma plane of shape (2, 2, 2) for a Y plane of 6 x 4 (2 x 3 x 2 expected)"),
    (lambda: ycbcr([(Y, Fake((4, 6, 2)))], "nv21", CUDA),
     "frame 0: an interleaved chroma plane of shape (4, 6, 2) for a Y plane of 6 x 4 (2 x 3 x 2 expected)"),
    (lambda: targets420([(Y, CBCR)], "yv12"), ORDER),
    (lambda: targets420([object()], "yv12"), ORDER),                   # the order before the first target
    (lambda: targets420([], "NV12"), "order 'NV12' is neither \"nv12\" nor \"nv21\""),
    (lambda: targets420([(Y, CBCR)], None), "order None is neither \"nv12\" nor \"nv21\""),
    (lambda: ycbcr([(Y, CBCR)], "yv12", CUDA), ORDER),
    (lambda: ycbcr([(object(),)], "yv12", CUDA), ORDER),               # a frame's order before the frame
    (lambda: ycbcr([(Y, CBCR), (Y, CBCR)], ["nv21", "yv12"], CUDA), ORDER),
    (lambda: ycbcr([(Y,), (Y, CBCR)], ["nv21", "yv12"], CUDA),         # ... and after the frames before it
     "frame 0: (y, cb, cr) or (y, cbcr) expected, not 1 arrays"),
    (lambda: ycbcr([(Y, CBCR), (Y, CBCR)], ["nv12"], CUDA), "1 orders for 2 frames"),
    (lambda: ycbcr([(Y, CBCR)], [], CUDA), "0 orders for 1 frames"),
    (lambda: ycbcr([(object(),)], ["nv12", "nv12", "nv12"], HOST), "3 orders for 1 frames"),
    # ---- display surfaces, at 16 and at 32 bits per pixel
    (lambda: surfaces([object()], 16), "surface 0 is " + NO_CUDA),
    (lambda: surfaces([None, Fake((4, 6, 4), iface=HOST)], 32), "surface 1 is " + NO_CUDA),
    (lambda: surfaces([Fake((4, 6, 2), "<i2")], 16), "surface 0: bytes (uint8) expected, not <i2"),
    (lambda: surfaces([S32], 16), "surface 0: shape (4, 6, 4) is not H x W x 2 (the bytes of a pixel at 16 bpp)"),
    (lambda: surfaces([S16], 32), "surface 0: shape (4, 6, 2) is not H x W x 4 (the bytes of a pixel at 32 bpp)"),
    (lambda: surfaces([S32], 24), "surface 0: shape (4, 6, 4) is not H x W x 3 (the bytes of a pixel at 24 bpp)"),
    (lambda: surfaces([Fake((4, 12))], 16), "surface 0: shape (4, 12) is not H x W x 2 (the bytes of a pixel at 16 bpp)"),
    (lambda: surfaces([S32, Fake((4, 24))], 32), "surface 1: shape (4, 24) is not H x W x 4 (the bytes of a pixel at 32 bpp)"),
    (lambda: surfaces([Fake((4, 6, 2), strides=(24, 4, 1))], 16), "surface 0: strides (24, 4, 1) cannot be described by a pitch " + ADJACENT),
    (lambda: surfaces([Fake((4, 6, 2), strides=(24, 2, 2))], 16), "surface 0: strides (24, 2, 2) cannot be described by a pitch " + ADJACENT),
    (lambda: surfaces([Fake((4, 6, 4), strides=(24, 2, 1))], 32), "surface 0: strides (24, 2, 1) cannot be described by a pitch " + ADJACENT),
    (lambda: surfaces([Fake((4, 6, 4), strides=(0, 4, 1))], 32), "surface 0: strides (0, 4, 1) cannot be described by a pitch " + ADJACENT),
    (lambda: surfaces([Fake((4, 6, 2), strides=(-12, 2, 1))], 16), "surface 0: strides (-12, 2, 1) cannot be described by a pitch " + ADJACENT),
    (lambda: surfaces([Fake((4, 6, 2), readonly=True)], 16), "surface 0 is read-only"),
    (lambda: surfaces([S32, None, Fake((4, 6, 4), readonly=True)], 32), "surface 2 is read-only"),
    # ---- packed int16 planes
    (lambda: packed(None, object()), "the planes are " + NO_CUDA),
    (lambda: packed("a", Fake((4, 6), "<i2", iface=HOST)), "the planes `a' are " + NO_CUDA),
    (lambda: packed(None, Y), "planes: int16 H x W or 3 x H x W expected, not |u1 (4, 6)"),
    (lambda: packed(None, Fake((4, 6), ">i2")), "planes: int16 H x W or 3 x H x W expected, not >i2 (4, 6)"),
    (lambda: packed("cb", I16((2, 4, 6))), "planes `cb': int16 H x W or 3 x H x W expected, not <i2 (2, 4, 6)"),
    (lambda: packed(None, I16((24,))), "planes: int16 H x W or 3 x H x W expected, not <i2 (24,)"),
    (lambda: packed(None, I16((4, 6), strides=(24, 2))), "planes: strides (24, 2) are not those of a packed array"),
    (lambda: packed("y", I16((4, 6), strides=(6, 1))), "planes `y': strides (6, 1) are not those of a packed array"),
    (lambda: packed(None, I16((3, 4, 6), strides=(64, 12, 2))), "planes: strides (64, 12, 2) are not those of a packed array"),
    (lambda: packed(None, I16((4, 6), strides=(0, 2))), "planes: strides (0, 2) are not those of a packed array"),
    # ---- the functions of the module, before they touch the library
    (lambda: fiasco_amd.planes_to_pixels_device(None, object(), Y), "the planes are " + NO_CUDA),
    (lambda: fiasco_amd.planes_to_pixels_device(None, Y, Y), "planes: int16 H x W or 3 x H x W expected, not |u1 (4, 6)"),
    (lambda: fiasco_amd.planes_to_pixels_device(None, PY, object()), "target 0 is " + NO_CUDA),
    (lambda: fiasco_amd.planes_to_pixels_device(None, PY, Fake((4, 6), readonly=True)), "target 0 is read-only"),
    (lambda: fiasco_amd.planes_to_pixels_device(None, PY, Fake((4, 8))), "target of 8 x 4 pixels for planes of 6 x 4"),
    (lambda: fiasco_amd.planes_to_pixels_device(None, I16((3, 4, 6)), Fake((6, 4, 3))), "target of 4 x 6 pixels for planes of 6 x 4"),
    (lambda: fiasco_amd.planes_to_pixels_device(None, PY, None), "target of 0 x 0 pixels for planes of 6 x 4"),
    (lambda: fiasco_amd.planes_to_420_device(None, PY, object(), PCR, (Y, CB, CR)), "the planes `cb' are " + NO_CUDA),
    (lambda: fiasco_amd.planes_to_420_device(None, PY, PCB, I16((2, 3), strides=(8, 2)), (Y, CB, CR)),
     "planes `cr': strides (8, 2) are not those of a packed array"),
    (lambda: fiasco_amd.planes_to_420_device(None, I16((3, 4, 6)), PCB, PCR, (Y, CB, CR)),
     "planes_to_420_device: three int16 arrays of two dimensions expected"),
    (lambda: fiasco_amd.planes_to_420_device(None, PY, I16((2, 2)), PCR, (Y, CB, CR)),
     "planes_to_420_device: chroma planes of (2, 2) and (3, 2) for a Y plane of 6 x 4"),
    (lambda: fiasco_amd.planes_to_420_device(None, PY, PCB, I16((4, 6)), (Y, CB, CR)),
     "planes_to_420_device: chroma planes of (3, 2) and (6, 4) for a Y plane of 6 x 4"),
    (lambda: fiasco_amd.planes_to_420_device(None, PY, PCB, PCR, None, order="yv12"), "planes_to_420_device: no target"),
    (lambda: fiasco_amd.planes_to_420_device(None, PY, PCB, PCR, (Y, CBCR), order="yv12"), ORDER),
    (lambda: fiasco_amd.planes_to_420_device(None, PY, PCB, PCR, (Y, CB)), "target 0: the chroma plane has shape (2, 3), 3 dimensions expected"),
    (lambda: fiasco_amd.render_planes_device_420(None, R16, PY, PCB, Y, S16), "planes `cr': int16 H x W or 3 x H x W expected, not |u1 (4, 6)"),
    (lambda: fiasco_amd.render_planes_device_420(None, R16, PY, I16((3, 2, 3)), PCR, S16),
     "render_planes_device_420: three int16 arrays of two dimensions expected"),
    (lambda: fiasco_amd.render_planes_device_420(None, R16, PY, PCB, I16((3, 2)), S16),
     "render_planes_device_420: chroma planes of (3, 2) and (2, 3) for a Y plane of 6 x 4"),
    (lambda: fiasco_amd.render_planes_device_420(None, R16, PY, PCB, PCR, S32),
     "surface 0: shape (4, 6, 4) is not H x W x 2 (the bytes of a pixel at 16 bpp)"),
    (lambda: fiasco_amd.render_planes_device_420(None, R32, PY, PCB, PCR, Fake((4, 6, 4), readonly=True)), "surface 0 is read-only"),
    (lambda: fiasco_amd.render_planes_device_420(None, R32, PY, PCB, PCR, None), "render_planes_device_420: no surface"),
    (lambda: fiasco_amd.render_planes_device(None, R32, object(), S32), "the planes are " + NO_CUDA),
    (lambda: fiasco_amd.render_planes_device(None, R32, PY, S16), "surface 0: shape (4, 6, 2) is not H x W x 4 (the bytes of a pixel at 32 bpp)"),
    (lambda: fiasco_amd.render_planes_device(None, R16, PY, object()), "surface 0 is " + NO_CUDA),
    (lambda: fiasco_amd.render_planes_device(None, R16, PY, None), "render_planes_device: no surface"),
    (lambda: fiasco_amd.planes_distortion_device(None, PY, object()), "the planes `b' are " + NO_CUDA),
    (lambda: fiasco_amd.planes_distortion_device(None, Y, PY), "planes `a': int16 H x W or 3 x H x W expected, not |u1 (4, 6)"),
    (lambda: fiasco_amd.planes_distortion_device(None, PY, I16((3, 4, 6))), "planes of (4, 6) against planes of (3, 4, 6)"),
    (lambda: fiasco_amd.planes_distortion_device(None, PY, I16((6, 4))), "planes of (4, 6) against planes of (6, 4)"),
    (lambda: fiasco_amd.smooth_planes_device(None, Y, [], 50), "planes: int16 H x W or 3 x H x W expected, not |u1 (4, 6)"),
    (lambda: fiasco_amd.smooth_planes_device(None, I16((4, 6), strides=(16, 2)), [], 50, fused=True),
     "planes: strides (16, 2) are not those of a packed array"),
]


@pytest.mark.parametrize("k", range(len(REFUSALS)))
def test_descriptor_refuses_with_its_message(k):
    call, message = REFUSALS[k]
    with pytest.raises(FiascoError) as e:
        call()
    assert str(e.value) == message and type(e.value) is FiascoError


def fields(d):
    return tuple(getattr(d, name) for name, _ in d._fields_)


def test_what_the_descriptors_accept_and_fill_in():
    """The other side of the table: no strides (the key missing, or None) means packed; a source may be read-only, and so may
    the planes of a frame; the pitches come from the strides; nv12 / nv21 decide which chroma byte comes first."""
    for strides in ("omit", None):
        f = frames([Fake((4, 6), strides=strides, readonly=True), Fake((4, 6, 3), strides=strides), Fake((3, 4, 6), strides=strides)])
        assert [fields(d) for d in f] == [(0x10000, 6, 0, 6, 4, 0), (0x10000, 18, 0, 6, 4, 1), (0x10000, 6, 24, 6, 4, 2)]
        t = targets420([(Fake((4, 6), strides=strides), Fake((2, 3), strides=strides, ptr=0x20000), CR), None,
                        (Y, Fake((2, 3, 2), strides=strides, ptr=0x20000))], "nv21")
        assert [fields(d) for d in t] == [(0x10000, 6, 0x20000, 0x30000, 3, 1, 6, 4), (None, 0, None, None, 0, 0, 0, 0),
                                          (0x10000, 6, 0x20001, 0x20000, 6, 2, 6, 4)]
        s = surfaces([Fake((4, 6, 2), strides=strides), None], 16)
        assert [fields(d) for d in s] == [(0x10000, 12, 6, 4), (None, 0, 0, 0)]
        assert fields(surfaces([Fake((4, 6, 4), strides=strides)], 32)[0]) == (0x10000, 24, 6, 4)
        assert packed(None, I16((3, 4, 6), strides=strides, readonly=True)) == (0x10000, (3, 4, 6))
    assert packed("y", I16((4, 6), strides=(12, 2))) == (0x10000, (4, 6)) == packed(None, Fake((4, 6), "=i2"))
    assert isinstance(targets([Y])[0], fiasco_amd.DeviceTarget) and isinstance(frames([Y])[0], fiasco_amd.DeviceFrame)
    assert fields(targets([Fake((3, 4, 6), strides=(100, 16, 1))])[0]) == (0x10000, 16, 100, 6, 4, 2)
    assert fields(surfaces([Fake((4, 6, 4), strides=(64, 4, 1))], 32)[0]) == (0x10000, 64, 6, 4)
    assert fields(targets420([(Fake((4, 6), strides=(32, 1)), Fake((2, 3), strides=(16, 1)), Fake((2, 3), strides=(16, 1)))])[0]) \
        == (0x10000, 32, 0x10000, 0x10000, 16, 1, 6, 4)
    # frames: host or device memory, read-only planes, 4:2:0 and 4:4:4, one order per frame
    ro = Fake((4, 6), readonly=True)
    y = ycbcr([(ro, CB, CR), (Y, Fake((4, 6), ptr=0x20000), Fake((4, 6), ptr=0x30000)), (Y, CBCR), (Y, CBCR)],
              ["nv12", "nv21", "nv12", "nv21"], CUDA)
    assert isinstance(y[0], fiasco_amd.YCbCrFrame)
    assert [fields(d) for d in y] == [(0x10000, 6, 0x20000, 0x30000, 3, 1, 1, 6, 4), (0x10000, 6, 0x20000, 0x30000, 6, 1, 0, 6, 4),
                                      (0x10000, 6, 0x20000, 0x20001, 6, 2, 1, 6, 4), (0x10000, 6, 0x20001, 0x20000, 6, 2, 1, 6, 4)]
    h = ycbcr([(HY, HCB, Fake((2, 3), strides="omit", iface=HOST))], "nv12", HOST)
    assert fields(h[0]) == (0x10000, 6, 0x10000, 0x10000, 3, 1, 1, 6, 4)
    assert len(ycbcr([], "nv12", HOST)) == 1 and len(frames([])) == 1 and len(targets420([])) == 1


# ------------------------------------------------------------------ a Batch on the CPU oracle

@pytest.fixture(scope="module")
def batch(oracle, inputs):
    """two staged frames of 96 x 64; nothing is encoded"""
    o = oracle.cli_options()
    b = fiasco_amd.Batch(oracle, [inputs.data("g96x64")] * 2, 20.0, o)
    yield b
    b.free(); o.delete()


T = Fake((64, 96))
T420 = (Fake((64, 96)), Fake((32, 48)), Fake((32, 48)))

BATCH_REFUSALS = [
    (lambda b: b.decode_device([T]), "decode_device: 1 targets for a batch of 2"),
    (lambda b: b.decode_device(iter([T, T, None])), "decode_device: 3 targets for a batch of 2"),
    (lambda b: b.decode_device([T], magnify=1), "decode_device: 1 targets for a batch of 2"),
    (lambda b: b.decode_device([T], smoothing=-1), "decode_device: 1 targets for a batch of 2"),
    (lambda b: b.decode_device([T], magnify=1, smoothing=50),         # together: refused before the count
     "decode_device: smoothing and magnify together (decode_shown writes the smoothed magnified frame)"),
    (lambda b: b.decode_device([T, T], None, -1, -1),
     "decode_device: smoothing and magnify together (decode_shown writes the smoothed magnified frame)"),
    (lambda b: b.decode_device([None, object()]), "target 1 is " + NO_CUDA),
    (lambda b: b.decode_device([T, Fake((64, 96), readonly=True)], smoothing=30), "target 1 is read-only"),
    (lambda b: b.decode_shown([T, T, T]), "decode_shown: 3 targets for a batch of 2"),
    (lambda b: b.decode_shown([]), "decode_shown: 0 targets for a batch of 2"),
    (lambda b: b.decode_shown([Fake((64, 96), "<i2"), None]), "target 0: 8-bit unsigned pixels expected, not <i2"),
    (lambda b: b.decode_420([T420]), "decode_420: 1 targets for a batch of 2"),
    (lambda b: b.decode_420([T420], order="yv12"), "decode_420: 1 targets for a batch of 2"),
    (lambda b: b.decode_420([T420, None], order="yv12"), ORDER),
    (lambda b: b.decode_420([None, T420[:1]]), "target 1: (y, cb, cr) or (y, cbcr) expected, not 1 arrays"),
    (lambda b: b.decode_rendered(R16, [S16]), "decode_rendered: 1 surfaces for a batch of 2"),
    (lambda b: b.decode_rendered(R16, [S16, S32]), "surface 1: shape (4, 6, 4) is not H x W x 2 (the bytes of a pixel at 16 bpp)"),
    (lambda b: b.decode_rendered_420(R32, [S32, S32, None]), "decode_rendered_420: 3 surfaces for a batch of 2"),
    (lambda b: b.decode_rendered_420(R32, [None, S16]), "surface 1: shape (4, 6, 2) is not H x W x 4 (the bytes of a pixel at 32 bpp)"),
    (lambda b: b.decode_thumbnails(None, 0, [T]), "decode_thumbnails: reduce = 0 (1 halves the side length)"),
    (lambda b: b.decode_thumbnails([T], -2, [T, T]), "decode_thumbnails: reduce = -2 (1 halves the side length)"),
    (lambda b: b.decode_thumbnails(None, 1, [T]), "decode_thumbnails: 1 thumbs for a batch of 2"),
    (lambda b: b.decode_thumbnails([T], 1, [T, T, T]), "decode_thumbnails: 3 thumbs for a batch of 2"),
    (lambda b: b.decode_thumbnails([T, T, T], 1, [T, T]), "decode_thumbnails: 3 targets for a batch of 2"),
    (lambda b: b.decode_thumbnails([T], 2, [None, None], smoothing=-1), "decode_thumbnails: 1 targets for a batch of 2"),
    (lambda b: b.decode_thumbnails([T, object()], 1, [object(), T]), "target 1 is " + NO_CUDA),
    (lambda b: b.decode_thumbnails(None, 1, [T, Fake((32, 48), readonly=True)]), "target 1 is read-only"),
    (lambda b: b.decode_distortion_device([T]), "decode_distortion_device: 1 targets for a batch of 2"),
    (lambda b: b.decode_distortion_device([T, T, T], smoothing=-1), "decode_distortion_device: 3 targets for a batch of 2"),
    (lambda b: b.decode_distortion_device([T, Fake((64, 96, 2))]), "target 1: shape (64, 96, 2) is neither H x W, H x W x 3 nor 3 x H x W"),
    (lambda b: b.upload_device([T]), "upload_device: 1 frames for a batch of 2"),
    (lambda b: b.upload_device([T, object()]), "frame 1 is " + NO_CUDA),
    (lambda b: b.upload_device_ycbcr([]), "upload_device_ycbcr: 0 frames for a batch of 2"),
    (lambda b: b.upload_device_ycbcr([T420, T420, T420], order="yv12"), "upload_device_ycbcr: 3 frames for a batch of 2"),
    (lambda b: b.upload_device_ycbcr([T420, T420], order="yv12"), ORDER),
    (lambda b: b.upload_device_ycbcr([T420, T420], order=["nv12"]), "1 orders for 2 frames"),
    (lambda b: b.upload_device_ycbcr([T420, (HY, HCB, HCR)]), "frame 1: the Y plane is " + NO_CUDA),
    # entries only the HIP library has, asked of the oracle
    (lambda b: fiasco_amd.Batch.from_device_ycbcr(b.lib, [T420]),
     "%s has no fiasco_amd_batch_stage_device_ycbcr: frames in device memory need the HIP library"),
    (lambda b: fiasco_amd.Sequence.from_device(b.lib, [T]),
     "%s has no fiasco_amd_seq_open_device: videos in device memory need the HIP library"),
    (lambda b: fiasco_amd.Sequence.from_device_ycbcr(b.lib, [T420]),
     "%s has no fiasco_amd_seq_open_device_ycbcr: videos in device memory need the HIP library"),
    # host frames: the descriptor's refusals come before the library is asked
    (lambda b: fiasco_amd.Batch.from_ycbcr(b.lib, [T420]), "frame 0: the Y plane is not in host memory (no __array_interface__)"),
    (lambda b: fiasco_amd.Sequence.from_ycbcr(b.lib, [(HY, HCB, HCR)], order="yv12"), ORDER),
]


@pytest.mark.parametrize("k", range(len(BATCH_REFUSALS)))
def test_batch_refuses_with_its_message(batch, k):
    call, message = BATCH_REFUSALS[k]
    with pytest.raises(FiascoError) as e:
        call(batch)
    assert str(e.value) == (message % batch.lib.path if "%s" in message else message) and type(e.value) is FiascoError


def test_what_is_not_a_fiasco_error(batch, inputs):
    """upload() asserts its count; stats() of a band no frame has is None, not a refusal."""
    with pytest.raises(AssertionError):
        batch.upload([inputs.data("g96x64")])
    assert batch.stats(0, band=3) is None
    assert batch.n == 2 and batch._geom == [(96, 64, 1)] * 2 and batch._keep is None
