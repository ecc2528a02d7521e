"""Arrays into the structures of the C ABI: one reader of __cuda_array_interface__ / __array_interface__ (_interface), and on
top of it the descriptors of frames, targets, 4:2:0 tuples, display surfaces and packed int16 planes, each with the wording
of its own refusals.  Importing this module imports neither numpy nor torch: numpy is imported by the one function that
allocates, torch is only looked up in sys.modules."""
import ctypes

from ._abi import (FIASCO_AMD_GRAY8, FIASCO_AMD_RGB8_INTERLEAVED, FIASCO_AMD_RGB8_PLANAR, DeviceFrame, DeviceSurface,
                   DeviceTarget, DeviceTarget420, FiascoError, YCbCrFrame)

_CUDA = "__cuda_array_interface__"
_UINT8 = ("|u1", "<u1", ">u1", "=u1")


def _packed_strides(shape):
    out, n = [], 1
    for v in reversed(shape):
        out.append(n)
        n *= v
    return reversed(out)


def _interface(a, iface=_CUDA, itemsize=1):
    """(address, typestr, shape, strides, read-only flag) of the array `a` shows through `iface`; where the interface gives no
    strides, those of a packed array of `itemsize` bytes an element.  None where `a` has no such interface: the refusal is
    the caller's."""
    d = getattr(a, iface, None)
    if d is None:
        return None
    shape = tuple(int(v) for v in d["shape"])
    strides = d.get("strides")
    strides = tuple(int(v) for v in strides) if strides is not None else tuple(itemsize * v for v in _packed_strides(shape))
    return int(d["data"][0]), d["typestr"], shape, strides, bool(d["data"][1])


def _byte_plane(who, what, a, ndim, iface=_CUDA, writable=False):
    """(address, shape, strides) of one uint8 array of `ndim` dimensions whose innermost elements are adjacent and whose pitch
    is positive, read through `iface` (__array_interface__: host memory, __cuda_array_interface__: device memory); the
    refusals speak of "`who`: the `what`" ("target 3: the Y plane")."""
    got = _interface(a, iface)
    if got is None:
        raise FiascoError("%s: the %s is not in %s memory (no %s)" % (who, what, "device" if "cuda" in iface else "host", iface))
    address, typestr, shape, strides, readonly = got
    if typestr not in _UINT8:
        raise FiascoError("%s: the %s holds %s, not bytes (uint8)" % (who, what, typestr))
    if len(shape) != ndim:
        raise FiascoError("%s: the %s has shape %s, %d dimensions expected" % (who, what, shape, ndim))
    if strides[-1] != 1 or (ndim == 3 and strides[1] != 2) or strides[0] <= 0:
        raise FiascoError("%s: the strides %s of the %s cannot be described by a pitch" % (who, strides, what))
    if writable and readonly:
        raise FiascoError("%s: the %s is read-only" % (who, what))
    return address, shape, strides


def _check_order(order):
    if order not in ("nv12", "nv21"):
        raise FiascoError("order %r is neither \"nv12\" nor \"nv21\"" % (order,))


def _yuv_tuple(who, t, order, iface, writable, full_size_chroma):
    """One (y, cb, cr) or (y, cbcr) tuple of byte planes as the 4:2:0 structures hold it: (y, y pitch, cb, cr, chroma pitch,
    c_step, width, height, chroma shape (h, w)).  Cb and Cr have H/2 x W/2 samples and share one pitch -- with
    `full_size_chroma` H x W will do as well --; cbcr has the shape H/2 x W/2 x 2, Cb first for `order` "nv12"."""
    if len(t) not in (2, 3):
        raise FiascoError("%s: (y, cb, cr) or (y, cbcr) expected, not %d arrays" % (who, len(t)))
    y, (h, w), ys = _byte_plane(who, "Y plane", t[0], 2, iface, writable)
    if len(t) == 3:
        cb, sb, stb = _byte_plane(who, "Cb plane", t[1], 2, iface, writable)
        cr, sr, str_ = _byte_plane(who, "Cr plane", t[2], 2, iface, writable)
        if sr != sb or not (sb == (h // 2, w // 2) or (full_size_chroma and sb == (h, w))):
            expected = ("%d x %d for 4:4:4 or %d x %d for 4:2:0" % (w, h, w // 2, h // 2) if full_size_chroma
                        else "%d x %d" % (w // 2, h // 2))
            raise FiascoError("%s: chroma planes of %s and %s for a Y plane of %d x %d (%s expected)"
                              % (who, sb[::-1], sr[::-1], w, h, expected))
        if stb[0] != str_[0]:
            raise FiascoError("%s: the chroma planes have pitches %d and %d (one pitch expected)" % (who, stb[0], str_[0]))
        return y, ys[0], cb, cr, stb[0], 1, w, h, sb
    c, sc, stc = _byte_plane(who, "chroma plane", t[1], 3, iface, writable)
    if sc != (h // 2, w // 2, 2):
        raise FiascoError("%s: an interleaved chroma plane of shape %s for a Y plane of %d x %d (%d x %d x 2 expected)"
                          % (who, sc, w, h, h // 2, w // 2))
    cb, cr = (c, c + 1) if order == "nv12" else (c + 1, c)
    return y, ys[0], cb, cr, stc[0], 2, w, h, sc[:2]


def _describe(what, i, fr, d):
    """One GPU array (a torch tensor, anything with __cuda_array_interface__) into the DeviceFrame / DeviceTarget d:
    layout from the shape, pitch and plane stride from the strides.  Returns the interface's read-only flag."""
    got = _interface(fr)
    if got is None:
        raise FiascoError("%s %d is not in device memory (no __cuda_array_interface__)" % (what, i))
    d.data, typestr, shape, strides, readonly = got
    if typestr not in _UINT8:
        raise FiascoError("%s %d: 8-bit unsigned pixels expected, not %s" % (what, i, typestr))
    bad = None
    if len(shape) == 2:
        d.layout, (d.height, d.width) = FIASCO_AMD_GRAY8, shape
        if strides[1] != 1:
            bad = "pixels of a row must be adjacent"
        d.pitch, d.plane_stride = strides[0], 0
    elif len(shape) == 3 and shape[2] == 3:
        d.layout, (d.height, d.width) = FIASCO_AMD_RGB8_INTERLEAVED, shape[:2]
        if strides[2] != 1 or strides[1] != 3:
            bad = "R, G, B of a pixel and the pixels of a row must be adjacent"
        d.pitch, d.plane_stride = strides[0], 0
    elif len(shape) == 3 and shape[0] == 3:
        d.layout, (d.height, d.width) = FIASCO_AMD_RGB8_PLANAR, shape[1:]
        if strides[2] != 1:
            bad = "pixels of a row must be adjacent"
        d.pitch, d.plane_stride = strides[1], strides[0]
    else:
        raise FiascoError("%s %d: shape %s is neither H x W, H x W x 3 nor 3 x H x W" % (what, i, shape))
    if bad is None and (min(strides) <= 0):
        bad = "strides must be positive"
    if bad:
        raise FiascoError("%s %d: strides %s cannot be described by pitch and plane stride (%s)" % (what, i, strides, bad))
    return readonly


def _device_frames(frames):
    """The fiasco_amd_device_frame array of a list of GPU arrays (_describe)."""
    arr = (DeviceFrame * max(len(frames), 1))()
    for i, fr in enumerate(frames):
        _describe("frame", i, fr, arr[i])
    return arr


def _device_targets(targets):
    """The fiasco_amd_device_target array of a list of writable GPU arrays (_describe); None: data = NULL, skipped."""
    arr = (DeviceTarget * max(len(targets), 1))()
    for i, t in enumerate(targets):
        if t is not None and _describe("target", i, t, arr[i]):
            raise FiascoError("target %d is read-only" % i)
    return arr


def _device_targets_420(targets, order="nv12"):
    """The fiasco_amd_device_target_420 array of a list of 4:2:0 targets: (y, cb, cr), three 2-D arrays, or (y, cbcr) with
    cbcr of shape H/2 x W/2 x 2 and `order` "nv12" (Cb first) or "nv21"; None: y = NULL, skipped."""
    _check_order(order)
    arr = (DeviceTarget420 * max(len(targets), 1))()
    for i, t in enumerate(targets):
        if t is not None:
            d = arr[i]
            d.y, d.y_pitch, d.cb, d.cr, d.c_pitch, d.c_step, d.width, d.height, _ = _yuv_tuple(
                "target %d" % i, tuple(t), order, _CUDA, writable=True, full_size_chroma=False)
    return arr


def _ycbcr_frames(frames, order, iface):
    """The fiasco_amd_ycbcr_frame array of a list of frames: (y, cb, cr), three 2-D arrays, or (y, cbcr) with cbcr of shape
    H/2 x W/2 x 2 and `order` "nv12" (Cb first) or "nv21" -- what _device_targets_420 accepts; `order` may also be a list, one
    entry per frame.  The subsampling is inferred from the chroma shape: full size is 4:4:4, half size 4:2:0, anything else
    raises."""
    orders = [order] * len(frames) if isinstance(order, str) else list(order)
    if len(orders) != len(frames):
        raise FiascoError("%d orders for %d frames" % (len(orders), len(frames)))
    arr = (YCbCrFrame * max(len(frames), 1))()
    for i, t in enumerate(frames):
        _check_order(orders[i])
        d = arr[i]
        d.y, d.y_pitch, d.cb, d.cr, d.c_pitch, d.c_step, d.width, d.height, chroma = _yuv_tuple(
            "frame %d" % i, t, orders[i], iface, writable=False, full_size_chroma=True)
        d.subsampling = 0 if d.c_step == 1 and chroma == (d.height, d.width) else 1
    return arr


def _device_surfaces(surfaces, bpp):
    """The fiasco_amd_device_surface array of a list of writable uint8 GPU arrays of shape (H, W, bpp // 8); the pitch is the
    first stride, the other two must be bpp // 8 and 1; None: data = NULL, skipped."""
    arr = (DeviceSurface * max(len(surfaces), 1))()
    for i, t in enumerate(surfaces):
        if t is None:
            continue
        got = _interface(t)
        if got is None:
            raise FiascoError("surface %d is not in device memory (no __cuda_array_interface__)" % i)
        address, typestr, shape, strides, readonly = got
        if typestr not in _UINT8:
            raise FiascoError("surface %d: bytes (uint8) expected, not %s" % (i, typestr))
        if len(shape) != 3 or shape[2] != bpp // 8:
            raise FiascoError("surface %d: shape %s is not H x W x %d (the bytes of a pixel at %d bpp)"
                              % (i, shape, bpp // 8, bpp))
        if strides[2] != 1 or strides[1] != bpp // 8 or strides[0] <= 0:
            raise FiascoError("surface %d: strides %s cannot be described by a pitch (the bytes of a pixel and the pixels of a "
                              "row must be adjacent)" % (i, strides))
        if readonly:
            raise FiascoError("surface %d is read-only" % i)
        arr[i].data, arr[i].pitch, (arr[i].height, arr[i].width) = address, strides[0], shape[:2]
    return arr


def _packed_planes(name, p):
    """(address, shape) of packed int16 planes on the GPU, H x W or 3 x H x W; `name' tells the planes of a call apart in
    the refusals (None: it has one set)."""
    what = "planes" if name is None else "planes `%s'" % name
    got = _interface(p, itemsize=2)
    if got is None:
        raise FiascoError("the %s are not in device memory (no __cuda_array_interface__)" % what)
    address, typestr, shape, strides, _ = got
    if typestr not in ("<i2", "=i2") or len(shape) not in (2, 3) or (len(shape) == 3 and shape[0] != 3):
        raise FiascoError("%s: int16 H x W or 3 x H x W expected, not %s %s" % (what, typestr, shape))
    if strides != tuple(2 * v for v in _packed_strides(shape)):
        raise FiascoError("%s: strides %s are not those of a packed array" % (what, strides))
    return address, shape


def _planes_420(call, y, cb, cr):
    """([address of y, cb, cr], width, height) of three packed int16 planes on the GPU: Y of H x W, Cb and Cr of H/2 x W/2;
    the refusals begin with the name of the `call`."""
    planes = [_packed_planes(n, p) for n, p in (("y", y), ("cb", cb), ("cr", cr))]
    if any(len(shape) != 2 for _, shape in planes):
        raise FiascoError("%s: three int16 arrays of two dimensions expected" % call)
    (h, w), sb, sr = planes[0][1], planes[1][1], planes[2][1]
    if sb != (h // 2, w // 2) or sr != sb:
        raise FiascoError("%s: chroma planes of %s and %s for a Y plane of %d x %d" % (call, sb[::-1], sr[::-1], w, h))
    return [address for address, _ in planes], w, h


def _empty_planes_420(w, h):
    """One int16 numpy buffer for a frame decoded in 4:2:0, and its three views: Y [h, w], then Cb and Cr [h / 2, w / 2]."""
    import numpy
    y, c = w * h, (w // 2) * (h // 2)
    out = numpy.empty(y + 2 * c, dtype=numpy.int16)
    return out, (out[:y].reshape(h, w), out[y:y + c].reshape(h // 2, w // 2), out[y + c:].reshape(h // 2, w // 2))


def _stream_of(frames, stream):
    """The hipStream_t to order against: the caller's, else torch's current stream when the frames are torch
    tensors (torch is looked up, never imported, here), else the default stream."""
    import sys
    if stream is not None:
        return ctypes.c_void_p(int(getattr(stream, "cuda_stream", stream)))
    torch = sys.modules.get("torch")
    if torch is not None and frames and isinstance(frames[0], torch.Tensor):
        return ctypes.c_void_p(torch.cuda.current_stream(frames[0].device).cuda_stream)
    return None


def _stream_over(items, stream, tuples=False):
    """_stream_of for the items that are not None (`items` may be None itself); tuples: every item is a tuple of arrays."""
    live = [t for t in items or [] if t is not None]
    return _stream_of([a for t in live for a in t] if tuples else live, stream)
