"""fiasco_amd -- MI355X-native FIASCO encoder hot path behind the libfiasco C API.

Python here is plumbing only: a ctypes mirror of the C-ABI shared library
``libfiasco_amd.so`` (host C + hand-written HIP for gfx950).  The names follow the
reference interface (``fiasco_coder``, ``fiasco_c_options_set_*``; reference fiasco.h:303-398)
so that tests read like calls into the reference library.

There is no CPU fallback: ``fiasco_coder`` / ``encode_batch`` fail (return 0 / raise) when
the HIP device coder cannot run.

The structures and the table of the C ABI are in _abi.py, the descriptors that turn arrays into those structures in
_arrays.py; this module holds the classes.
"""
import ctypes
import os
import subprocess

from ._abi import *  # noqa: F401,F403  (FiascoError, the enum values, the structures, ABI and the ten *_SYMBOLS lists)
from ._abi import (_SIGNATURES, _VIDEO_SIGNATURES, _SMOOTH_SIGNATURES, _DISPLAY_SIGNATURES, _RENDER_SIGNATURES,  # noqa: F401
                   _YUV420_SIGNATURES, _YCBCR_SIGNATURES, _RENDER420_SIGNATURES, _STREAM_SIGNATURES, _DECODER_SIGNATURES)
from ._arrays import (_describe, _device_frames, _device_surfaces, _device_targets, _device_targets_420,  # noqa: F401
                      _empty_planes_420, _packed_planes, _packed_strides, _planes_420, _stream_of, _stream_over, _ycbcr_frames)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfiasco_amd.so")
CSRC = os.path.join(_HERE, "csrc")


def build(verbose=False):
    """Compile libfiasco_amd.so (gcc for the host C, hipcc --offload-arch=gfx950 for the
    device coder).  Works without a GPU (cross compilation)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC], stdout=out)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("build did not produce %s" % LIB_PATH)


# What the classes below share.  A `lib` is a Library, or whatever has its L, path and error_message().

def _check(lib, result):
    """What a C entry returned, if it is not 0 / NULL; FiascoError with the library's message if it is."""
    if not result:
        raise FiascoError(lib.error_message())
    return result


def _need(lib, symbol, what=None):
    """FiascoError unless the library has `symbol`; `what` says what it would take."""
    if not hasattr(lib.L, symbol):
        raise FiascoError("%s has no %s" % (lib.path, symbol) + (": %s" % what if what else ""))


def _take_bytes(lib, address, length):
    """The bytes of a buffer a C entry handed out; the C side's copy is freed."""
    try:
        return ctypes.string_at(address, length)
    finally:
        lib.L.fiasco_amd_free(address)


def _one_stream(lib, call):
    """The byte string call(out, length) leaves behind the two pointers."""
    out, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(lib, call(ctypes.byref(out), ctypes.byref(n)))
    return _take_bytes(lib, out.value, n.value)


def _streams(lib, n, call):
    """The n streams call(outs, olen) leaves in the two arrays, as bytes (None for a frame that failed); the C side's
    copies are freed."""
    outs = (ctypes.c_void_p * n)()
    olen = (ctypes.c_size_t * n)()
    call(outs, olen)
    return [_take_bytes(lib, outs[i], olen[i]) if outs[i] else None for i in range(n)]


def _borders(lib, call):
    """The borders call(out, cap) -> count lists, as (x, y, len, level, pass) tuples: asked once for the count, once for the
    list."""
    n = _check(lib, call(None, 0))
    arr = (Border * n)()
    if call(arr, n) != n:
        raise FiascoError(lib.error_message())
    return [(b.x, b.y, b.len, b.level, b.pass_) for b in arr]


def _handle(options):
    return options.handle if options else None


def _pnm_arrays(pnm_list):
    """The two arrays the C entries take raw PNM buffers in: the buffers and their lengths."""
    n = len(pnm_list)
    return (ctypes.c_char_p * n)(*pnm_list), (ctypes.c_size_t * n)(*[len(b) for b in pnm_list])


class Library:
    """ctypes binding of one libfiasco-compatible shared library."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise FiascoError("%s is missing: run fiasco_amd.build() (there is no fallback)" % path)
        self.path = path
        self.L = ctypes.CDLL(path)
        for signatures in ABI.values():                  # the one place that declares the ABI to ctypes
            for name, (restype, argtypes) in signatures.items():
                if hasattr(self.L, name):
                    fn = getattr(self.L, name)
                    fn.restype, fn.argtypes = restype, argtypes

    # -- misc ------------------------------------------------------------------
    def error_message(self):
        return self.L.fiasco_get_error_message().decode("latin-1")

    def core_name(self):
        return self.L.fiasco_amd_core_name().decode()

    def set_verbosity(self, level):
        self.L.fiasco_set_verbosity(level)

    def set_limits(self, max_states, max_level):
        _check(self, self.L.fiasco_amd_set_limits(max_states, max_level))

    def get_limits(self):
        a, b = ctypes.c_uint(), ctypes.c_uint()
        self.L.fiasco_amd_get_limits(ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def set_devices(self, ids):
        """fiasco_amd_set_devices: the devices the batch entries spread their frames over ([] = automatic)."""
        arr = (ctypes.c_int * max(len(ids), 1))(*ids)
        _check(self, self.L.fiasco_amd_set_devices(arr, len(ids)))

    def device_count(self):
        return self.L.fiasco_amd_device_count()

    def set_device(self, device):
        _check(self, self.L.fiasco_amd_set_device(device))

    def get_stats(self):
        st = Stats()
        self.L.fiasco_amd_get_stats(ctypes.byref(st))
        return st

    def reset_stats(self):
        self.L.fiasco_amd_reset_stats()

    # -- options ---------------------------------------------------------------
    def c_options_new(self):
        return COptions(self)

    def cli_options(self, optimize=0, dictionary_size=10000, progress=FIASCO_PROGRESS_NONE, **kw):
        """Options object configured like reference bin/cwfa.c:252-393 does for the CLI
        defaults (block levels [6,10] and 3 elements at --optimize 0; [4,12] / 5 above)."""
        o = self.c_options_new()
        o.set_frame_pattern(kw.get("pattern", "ippppppppp"))
        o.set_chroma_quality(kw.get("chroma_qfactor", 2.0), kw.get("chroma_dictionary", 40))
        o.set_smoothing(kw.get("smooth", 70))
        o.set_progress_meter(progress)
        o.set_tiling({"desc-variance": FIASCO_TILING_VARIANCE_DSC, "asc-variance": FIASCO_TILING_VARIANCE_ASC,
                      "asc-spiral": FIASCO_TILING_SPIRAL_ASC, "desc-spiral": FIASCO_TILING_SPIRAL_DSC}
                     [kw.get("tiling_method", "desc-variance")], kw.get("tiling_exponent", 4))
        if optimize <= 0:
            o.set_optimizations(6, 10, 3, dictionary_size, 0)
        else:
            o.set_optimizations(4, 12, 5, dictionary_size, optimize - 1)
        o.set_prediction(0, kw.get("min_level", 6), kw.get("max_level", 10))
        o.set_quantization(3, FIASCO_RPF_RANGE_1_50, 5, FIASCO_RPF_RANGE_1_00)
        return o

    # -- coder -----------------------------------------------------------------
    def fiasco_coder(self, inputnames, outputname, quality=20.0, options=None):
        """int fiasco_coder(inputname[], outputname, quality, options): 1 ok / 0 failure."""
        arr = (ctypes.c_char_p * (len(inputnames) + 1))()
        for i, n in enumerate(inputnames):
            arr[i] = os.fsencode(n)
        arr[len(inputnames)] = None
        return self.L.fiasco_coder(arr, os.fsencode(outputname) if outputname else None,
                                   ctypes.c_float(quality), _handle(options))

    def encode_batch(self, pnm_list, quality=20.0, options=None):
        """fiasco_amd_encode_batch: independent stills (raw PNM bytes) -> list of .fco bytes
        (None for a frame that failed)."""
        n = len(pnm_list)
        bufs, lens = _pnm_arrays(pnm_list)
        return _streams(self, n, lambda outs, olen: self.L.fiasco_amd_encode_batch(
            n, bufs, lens, ctypes.c_float(quality), _handle(options), outs, olen))


class Batch:
    """Staged batch (fiasco_amd_batch_stage / _encode / _free): inputs stay resident in HBM
    between encode() calls."""

    def __init__(self, lib, pnm_list, quality=20.0, options=None):
        bufs, lens = _pnm_arrays(pnm_list)
        self._staged(lib, lib.L.fiasco_amd_batch_stage(len(pnm_list), bufs, lens, ctypes.c_float(quality), _handle(options)),
                     [_pnm_geometry(p) for p in pnm_list])

    def _staged(self, lib, handle, geom, keep=None):
        """What every constructor ends in: the handle a stage entry gave (FiascoError if it gave none), (width, height, bands)
        of every frame, and the objects whose memory the C side borrows."""
        self.lib, self.n, self._keep, self._geom = lib, len(geom), keep, geom
        self.handle = _check(lib, handle)
        return self

    @classmethod
    def from_device(cls, lib, frames, quality=20.0, options=None, stream=None):
        """fiasco_amd_batch_stage_device: a batch of frames that already live in device memory.  A frame is a
        torch uint8 tensor on the GPU or any object with __cuda_array_interface__: H x W is gray, H x W x 3
        interleaved R, G, B, 3 x H x W planar; pitch and plane stride come from the strides (a slice of a larger
        tensor is read in place, a stride pattern the C struct cannot express raises FiascoError).  `stream`: the
        hipStream_t (integer) on which the pixels become ready; None = torch's current stream for torch tensors,
        else the default stream.  The objects are kept alive until the next upload or free()."""
        frames = list(frames)
        arr = _device_frames(frames)
        handle = lib.L.fiasco_amd_batch_stage_device(len(frames), arr, _stream_of(frames, stream), ctypes.c_float(quality),
                                                     _handle(options))
        geom = [(a.width, a.height, 1 if a.layout == FIASCO_AMD_GRAY8 else 3) for a in arr[:len(frames)]]
        return cls.__new__(cls)._staged(lib, handle, geom, frames)

    @classmethod
    def from_ycbcr(cls, lib, frames, quality=20.0, options=None, order="nv12"):
        """fiasco_amd_batch_stage_ycbcr: a batch of frames that are YCbCr already, in host memory (every build of the
        library).  A frame is (y, cb, cr), three 2-D numpy uint8 arrays -- chroma of H/2 x W/2 is 4:2:0 (I420; YV12 with cb
        and cr exchanged), of H x W 4:4:4 --, or (y, cbcr) with cbcr of shape H/2 x W/2 x 2: interleaved pairs, Cb first for
        order="nv12", Cr first for order="nv21".  Pitches come from the strides.  The planes the coder sees are
        (byte - 128) * 16, a 4:2:0 chroma sample replicated over its 2 x 2 pixels; the frames are converted during the call."""
        frames = [tuple(f) for f in frames]
        arr = _ycbcr_frames(frames, order, "__array_interface__")
        _need(lib, "fiasco_amd_batch_stage_ycbcr")
        handle = lib.L.fiasco_amd_batch_stage_ycbcr(len(frames), arr, ctypes.c_float(quality), _handle(options))
        return cls.__new__(cls)._staged(lib, handle, [(a.width, a.height, 3) for a in arr[:len(frames)]])

    @classmethod
    def from_device_ycbcr(cls, lib, frames, quality=20.0, options=None, stream=None, order="nv12"):
        """fiasco_amd_batch_stage_device_ycbcr: from_ycbcr with frames that live in device memory -- torch uint8 tensors on
        the GPU or anything with __cuda_array_interface__, for instance what decode_420 filled -- read in place by one
        kernel launch per device share.  `stream` as from_device.  The objects are kept alive until the next upload or
        free()."""
        _need(lib, "fiasco_amd_batch_stage_device_ycbcr", "frames in device memory need the HIP library")
        frames = [tuple(f) for f in frames]
        arr = _ycbcr_frames(frames, order, "__cuda_array_interface__")
        handle = lib.L.fiasco_amd_batch_stage_device_ycbcr(len(frames), arr, _stream_over(frames, stream, tuples=True),
                                                           ctypes.c_float(quality), _handle(options))
        return cls.__new__(cls)._staged(lib, handle, [(a.width, a.height, 3) for a in arr[:len(frames)]], frames)

    def _expect(self, what, items, noun="targets"):
        """`items` as a list, of one entry per frame of the batch; `what` is the method that refuses any other number."""
        items = list(items)
        if len(items) != self.n:
            raise FiascoError("%s: %d %s for a batch of %d" % (what, len(items), noun, self.n))
        return items

    def upload_device_ycbcr(self, frames, stream=None, order="nv12"):
        """fiasco_amd_batch_upload_device_ycbcr: upload_device with YCbCr frames (see from_device_ycbcr); may follow and be
        followed by upload() and upload_device()."""
        frames = self._expect("upload_device_ycbcr", [tuple(f) for f in frames], "frames")
        arr = _ycbcr_frames(frames, order, "__cuda_array_interface__")
        on = _stream_over(frames, stream, tuples=True)
        _check(self.lib, self.lib.L.fiasco_amd_batch_upload_device_ycbcr(self.handle, arr, on))
        self._keep = frames

    def upload_device(self, frames, stream=None):
        """fiasco_amd_batch_upload_device: new frames for every slot, converted on the device from where they lie
        (see from_device); not waited for, the next submit / collect(resubmit=True) encodes them."""
        frames = self._expect("upload_device", frames, "frames")
        arr = _device_frames(frames)
        _check(self.lib, self.lib.L.fiasco_amd_batch_upload_device(self.handle, arr, _stream_of(frames, stream)))
        self._keep = frames

    def input_planes(self, i):
        """fiasco_amd_batch_input_planes: the planes the coder sees for frame i, int16 [bands, h, w] (12.4 fixed point)."""
        import numpy
        w, h, bands = self._geom[i]          # replacement frames keep the size and colour model of the batch
        out = numpy.empty((bands, h, w), dtype=numpy.int16)
        _check(self.lib, self.lib.L.fiasco_amd_batch_input_planes(self.handle, i, out.ctypes.data))
        return out

    def upload(self, pnm_list):
        """fiasco_amd_batch_upload: new frames for every slot (host PNM buffers -> pinned ->
        HBM, not waited for); the next submit / collect(resubmit=True) encodes them."""
        assert len(pnm_list) == self.n
        bufs, lens = _pnm_arrays(pnm_list)
        _check(self.lib, self.lib.L.fiasco_amd_batch_upload(self.handle, bufs, lens))

    def submit(self):
        """fiasco_amd_batch_submit: start a pass over the resident inputs, do not wait."""
        return self.lib.L.fiasco_amd_batch_submit(self.handle)

    def collect(self, resubmit=False):
        """fiasco_amd_batch_collect: streams of the submitted pass; with resubmit the next pass
        is started before the host writes them (writer of pass i overlaps search of pass i+1)."""
        L, again = self.lib.L, 1 if resubmit else 0
        return _streams(self.lib, self.n, lambda outs, olen: L.fiasco_amd_batch_collect(self.handle, outs, olen, again))

    def encode(self):
        L = self.lib.L
        return _streams(self.lib, self.n, lambda outs, olen: L.fiasco_amd_batch_encode(self.handle, outs, olen))

    def stats(self, i, band=0):
        """fiasco_amd_batch_stats: root-range costs / squared error of frame i (band 0..2) of the
        last finished pass and the coder-side PSNR the reference reports (codec/coder.c:918-923)."""
        import math
        c = ctypes
        costs, err, w, h = c.c_float(), c.c_float(), c.c_uint(), c.c_uint()
        if not self.lib.L.fiasco_amd_batch_stats(self.handle, i, band, costs, err, w, h):
            return None
        mse = err.value / w.value / h.value
        return {"costs": costs.value, "err": err.value, "width": w.value, "height": h.value,
                "psnr_db": 10.0 * math.log10(255.0 * 255.0 / mse) if mse > 0 else float("inf")}

    def decode_plane(self, i, band, width, height):
        """fiasco_amd_batch_decode_plane: the decoded band as bytes (the payload of dfiasco -s 0's PGM for gray)."""
        buf = ctypes.create_string_buffer(width * height)
        _check(self.lib, self.lib.L.fiasco_amd_batch_decode_plane(self.handle, i, band, buf))
        return buf.raw

    def _size(self, i, magnify):
        w, h, bands = self._geom[i]
        return (magnified_size(self.lib, w, h, magnify) if magnify else (w, h)) + (bands,)

    def decode_planes(self, i, magnify=0):
        """fiasco_amd_batch_decode_planes: the decoded planes of frame i before any smoothing, int16 [bands, h, w]
        (12.4 fixed point).  magnify != 0: fiasco_amd_batch_decode_planes_magnified, the frame at 2^magnify times its
        side length as `dfiasco -m` shows it; h, w are those of magnified_size()."""
        import numpy
        L = self.lib.L
        w, h, bands = self._size(i, magnify)
        out = numpy.empty((bands, h, w), dtype=numpy.int16)
        _check(self.lib, L.fiasco_amd_batch_decode_planes_magnified(self.handle, i, magnify, out.ctypes.data) if magnify
               else L.fiasco_amd_batch_decode_planes(self.handle, i, out.ctypes.data))
        return out

    def smoothing_borders(self, i, magnify=0):
        """fiasco_amd_batch_smoothing_borders: the borders the reference's decoder smooths frame i along, as a list of
        (x, y, len, level, pass) sorted by pass -- odd level: rows y - 1 and y, columns x .. x + len - 1; even level:
        columns x - 1 and x, rows y .. y + len - 1.  The borders of one pass share no pixel.
        magnify != 0: fiasco_amd_batch_smoothing_borders_magnified, the borders of the frame as `dfiasco -m magnify`
        shows it, against the size magnified_size() gives.  FiascoError where the size rule refuses the magnification and
        where a state the reference smooths along falls below level 1 (the reference's own result is undefined there)."""
        L, b = self.lib.L, self.handle
        if magnify:
            return _borders(self.lib, lambda out, cap: L.fiasco_amd_batch_smoothing_borders_magnified(b, i, magnify, out, cap))
        return _borders(self.lib, lambda out, cap: L.fiasco_amd_batch_smoothing_borders(b, i, out, cap))

    def decode_device(self, targets, stream=None, magnify=0, smoothing=0):
        """fiasco_amd_batch_decode_device: the frames of the last finished pass, decoded on the device and written as
        8-bit pixels into `targets` -- the bytes of the PGM / PPM `dfiasco -s 0 -o` writes.  A target is a torch uint8
        tensor on the GPU or any writable object with __cuda_array_interface__, of the frame's size: H x W for a gray
        frame, H x W x 3 or 3 x H x W for a colour frame (pitch and plane stride from the strides, as from_device);
        None skips the frame.  `stream`: the hipStream_t (integer) the targets were last used on; None = torch's
        current stream for torch tensors, else the default stream.  That stream waits for the conversion: what is
        queued on it afterwards sees the pixels, no host synchronisation needed.  Returns the number of frames written.
        magnify != 0: fiasco_amd_batch_decode_device_magnified, the bytes of `dfiasco -s 0 -m magnify -o`; every target
        has the size magnified_size() gives for its frame.
        smoothing != 0: fiasco_amd_batch_decode_device_smoothed, the frame smoothed along the borders of its partition as
        `dfiasco -s smoothing -o` writes it (1 .. 100 per cent); -1: at the value of the frame's own stream header, what
        `dfiasco` shows when no -s is given.  Not together with magnify."""
        if smoothing and magnify:
            raise FiascoError("decode_device: smoothing and magnify together (decode_shown writes the smoothed magnified frame)")
        targets = self._expect("decode_device", targets)
        L, arr, on = self.lib.L, _device_targets(targets), _stream_over(targets, stream)
        if smoothing:
            return _check(self.lib, L.fiasco_amd_batch_decode_device_smoothed(self.handle, smoothing, arr, on))
        if magnify:
            return _check(self.lib, L.fiasco_amd_batch_decode_device_magnified(self.handle, magnify, arr, on))
        return _check(self.lib, L.fiasco_amd_batch_decode_device(self.handle, arr, on))

    def decode_shown(self, targets, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_batch_decode_device_shown: the frames of the last finished pass as `dfiasco -m magnify -s smoothing
        -o` writes them, into `targets` (as decode_device takes them; every target has the size magnified_size() gives
        for its frame).  The defaults give what plain `dfiasco -m magnify -o` writes: smoothed at the value of each frame's
        own stream header.  smoothing: -1, 0 (none) or 1 .. 100 per cent.  A frame that cannot be smoothed at `magnify`
        (a state of its partition falls below level 1) fails alone: the others are written, the return value counts them
        and lib.error_message() names the frame.  Returns the number of frames written."""
        targets = self._expect("decode_shown", targets)
        arr = _device_targets(targets)
        return _check(self.lib, self.lib.L.fiasco_amd_batch_decode_device_shown(
            self.handle, magnify, smoothing, arr, _stream_over(targets, stream)))

    def decode_420(self, targets, magnify=0, smoothing=-1, stream=None, order="nv12"):
        """fiasco_amd_batch_decode_device_420: the frames of the last finished pass decoded in 4:2:0, as the reference's
        decoder does with fiasco_d_options_set_4_2_0_format -- the chroma bands come from the automaton at half the side
        length, they are not subsampled -- at `-m magnify -s smoothing`, as 8-bit Y, Cb, Cr into `targets`.  A target is
        (y, cb, cr), three writable 2-D uint8 GPU arrays of H x W, H/2 x W/2 and H/2 x W/2 (I420; the chroma planes share one
        pitch), or (y, cbcr) with cbcr of shape H/2 x W/2 x 2: interleaved pairs, Cb first for order="nv12", Cr first for
        order="nv21"; W x H is magnified_size() of the frame; None skips the frame.  Flights, smoothing, per-frame refusals
        and `stream` as decode_shown; a gray frame and a frame whose chroma the reference leaves zero fail alone.  Returns
        the number of frames written."""
        targets = self._expect("decode_420", targets)
        arr = _device_targets_420(targets, order)
        return _check(self.lib, self.lib.L.fiasco_amd_batch_decode_device_420(
            self.handle, magnify, smoothing, arr, _stream_over(targets, stream, tuples=True)))

    def decode_planes_420(self, i, magnify=0):
        """fiasco_amd_batch_decode_planes_420: the unsmoothed planes of frame i decoded in 4:2:0 at `magnify`, three int16
        arrays (12.4 fixed point): Y [h, w], Cb and Cr [h / 2, w / 2]; h, w are those of magnified_size()."""
        w, h, _ = self._size(i, magnify)
        out, planes = _empty_planes_420(w, h)
        _check(self.lib, self.lib.L.fiasco_amd_batch_decode_planes_420(self.handle, i, magnify, out.ctypes.data))
        return planes

    def smoothing_borders_420(self, i, magnify=0):
        """fiasco_amd_batch_smoothing_borders_420: the borders the reference smooths the Y plane of frame i along when it
        decodes in 4:2:0, (x, y, len, level, pass) as smoothing_borders() lists them: the Y passes at shift `magnify`, then
        the Cb passes at shift `magnify` - 1, against the size magnified_size() gives."""
        L = self.lib.L
        return _borders(self.lib, lambda out, cap: L.fiasco_amd_batch_smoothing_borders_420(self.handle, i, magnify, out, cap))

    def decode_rendered(self, renderer, surfaces, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_batch_decode_device_rendered: the frames of the last finished pass as the reference's viewer puts them
        on the screen at `-m magnify -s smoothing`, through `renderer` into `surfaces` -- one per frame, a writable uint8 GPU
        array of shape (H, W, bpp // 8) with H, W from renderer.surface_size() for the frame at magnified_size(); the pitch is
        the first stride; None skips the frame.  Flights, smoothing, per-frame refusals and `stream` as decode_shown.
        Returns the number of frames written."""
        surfaces = self._expect("decode_rendered", surfaces, "surfaces")
        arr = _device_surfaces(surfaces, renderer.bpp)
        return _check(self.lib, self.lib.L.fiasco_amd_batch_decode_device_rendered(
            self.handle, renderer.handle, magnify, smoothing, arr, _stream_over(surfaces, stream)))

    def decode_rendered_420(self, renderer, surfaces, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_batch_decode_device_rendered_420: the frames of the last finished pass as the reference's viewer shows
        them on a screen -- decoded in 4:2:0 as decode_420 decodes them, at `-m magnify -s smoothing`, and rendered through
        `renderer` with every chroma sample standing for its 2 x 2 pixels -- into `surfaces`, one per frame as
        decode_rendered takes them, of the size renderer.surface_size_420() gives for the frame at magnified_size(); None
        skips the frame.  A gray frame and a frame whose chroma the reference leaves zero fail alone.  Returns the number
        of frames written."""
        surfaces = self._expect("decode_rendered_420", surfaces, "surfaces")
        arr = _device_surfaces(surfaces, renderer.bpp)
        return _check(self.lib, self.lib.L.fiasco_amd_batch_decode_device_rendered_420(
            self.handle, renderer.handle, magnify, smoothing, arr, _stream_over(surfaces, stream)))

    def decode_thumbnails(self, targets, reduce, thumbs, stream=None, smoothing=0):
        """fiasco_amd_batch_decode_device_thumbnails: ONE decode of the frames of the last finished pass that writes
        every frame into `targets` as decode_device does (None, or a list in which None skips the full-size frame) and
        the same frame at 1 / 2^reduce of its side length (reduce >= 1) into `thumbs` -- the bytes
        decode_device(magnify=-reduce) gives; a thumb has the size magnified_size(lib, w, h, -reduce), None skips it.
        `stream` as decode_device.  Returns the number of frames decoded.
        smoothing != 0: fiasco_amd_batch_decode_device_thumbnails_shown, both outputs smoothed (-1: at the value of the
        frame's stream header, 1 .. 100 per cent) -- the frame as decode_device(smoothing=...) writes it, the thumb as
        decode_shown(magnify=-reduce, smoothing=...) does."""
        thumbs = list(thumbs)
        if reduce < 1:
            raise FiascoError("decode_thumbnails: reduce = %d (1 halves the side length)" % reduce)
        self._expect("decode_thumbnails", thumbs, "thumbs")
        arr = None
        if targets is not None:
            targets = self._expect("decode_thumbnails", targets)
            arr = _device_targets(targets)
        L, b, tarr, on = self.lib.L, self.handle, _device_targets(thumbs), _stream_over((targets or []) + thumbs, stream)
        if smoothing:
            return _check(self.lib, L.fiasco_amd_batch_decode_device_thumbnails_shown(b, smoothing, arr, reduce, tarr, on))
        return _check(self.lib, L.fiasco_amd_batch_decode_device_thumbnails(b, arr, reduce, tarr, on))

    def decode_distortion_device(self, targets=None, stream=None, smoothing=0):
        """fiasco_amd_batch_decode_distortion_device: the frames of the last finished pass, decoded on the device and
        compared with their originals there.  Returns (n measured, sse, maxdiff, psnr_db), each [[per band] per frame]:
        the exact integer sum of the squared byte differences, the largest absolute byte difference, and
        10 log10(255^2 W H / sse) in double (inf for sse == 0; the mean is over the pixels of the image, as
        decode_psnr).  Bands a frame does not have read 0 / 0 / 0.0; a skipped frame reads as sse 0.  `targets`: None, or
        one target per frame as decode_device takes them (None: measured, not written) -- one decode serves both;
        `stream` as decode_device.  smoothing != 0: fiasco_amd_batch_decode_distortion_device_smoothed, the distortion
        (and the pixels) of the frame smoothed as decode_device(smoothing=...) smooths it."""
        import math
        c = ctypes
        L, n = self.lib.L, self.n
        arr = None
        if targets is not None:
            targets = self._expect("decode_distortion_device", targets)
            arr = _device_targets(targets)
        s, m = (c.c_ulonglong * (3 * n))(), (c.c_uint * (3 * n))()
        on = _stream_over(targets, stream)
        if smoothing:
            good = _check(self.lib, L.fiasco_amd_batch_decode_distortion_device_smoothed(self.handle, smoothing, s, m, arr, on))
        else:
            good = _check(self.lib, L.fiasco_amd_batch_decode_distortion_device(self.handle, s, m, arr, on))
        psnr = []
        for i in range(n):
            w, h, bands = self._geom[i]
            psnr.append([0.0 if k >= bands else float("inf") if not s[3 * i + k]
                         else 10.0 * math.log10(255.0 * 255.0 * w * h / s[3 * i + k]) for k in range(3)])
        return good, [list(s[3 * i:3 * i + 3]) for i in range(n)], [list(m[3 * i:3 * i + 3]) for i in range(n)], psnr

    def decode_psnr_all(self):
        """fiasco_amd_batch_decode_psnr_all: (n decoded, [[psnr dB per band]], [[mse per band]]) of all frames,
        decoded by one call of the device decoder."""
        n = self.n
        p = (ctypes.c_double * (3 * n))(); m = (ctypes.c_double * (3 * n))()
        good = self.lib.L.fiasco_amd_batch_decode_psnr_all(self.handle, p, m)
        return good, [list(p[3 * i:3 * i + 3]) for i in range(n)], [list(m[3 * i:3 * i + 3]) for i in range(n)]

    def decode_psnr(self, i):
        """fiasco_amd_batch_decode_psnr: decoded PSNR in dB per band of frame i (what `dfiasco -s 0` +
        `pnmpsnr` print for a gray frame), and the mean squared errors."""
        ps, ms = (ctypes.c_double * 3)(), (ctypes.c_double * 3)()
        _check(self.lib, self.lib.L.fiasco_amd_batch_decode_psnr(self.handle, i, ps, ms))
        return list(ps), list(ms)

    def free(self):
        if self.handle:
            self.lib.L.fiasco_amd_batch_free(self.handle)
            self.handle = None
        self._keep = None


def _pnm_geometry(buf):
    """(width, height, bands) of raw PGM / PPM bytes (what the C reader finds; a broken header never gets here)."""
    import re
    m = re.match(rb"P([56])(?:\s|#[^\n]*\n)*(\d+)(?:\s|#[^\n]*\n)+(\d+)", buf[:4096])
    return (int(m.group(2)), int(m.group(3)), 1 if m.group(1) == b"5" else 3) if m else None


class Renderer:
    """fiasco_amd_renderer_*: the reference's renderer (fiasco_renderer_new) restated -- colour masks, 16, 24 or 32 bits per
    pixel, optionally every pixel doubled in both directions.  Immutable; delete() frees it."""

    def __init__(self, lib, red_mask, green_mask, blue_mask, bpp, double_resolution=False):
        self.lib, self.bpp, self.double_resolution = lib, bpp, bool(double_resolution)
        self.masks = (red_mask, green_mask, blue_mask)
        self._fiasco = None
        self.handle = lib.L.fiasco_amd_renderer_new(red_mask, green_mask, blue_mask, bpp, 1 if double_resolution else 0)
        _check(lib, self.handle)

    def fiasco_renderer(self):
        """The fiasco_renderer_t of the same parameters (fiasco_renderer_new, include/libfiasco_amd_decoder.h), which renders
        Images; made on first use, freed by delete().  It keeps a staging surface: one thread at a time."""
        if not self._fiasco:
            _need(self.lib, "fiasco_renderer_new", "the decoder half of fiasco.h")
            self._fiasco = _check(self.lib, self.lib.L.fiasco_renderer_new(*self.masks, self.bpp, 1 if self.double_resolution else 0))
        return self._fiasco

    def surface_size(self, width, height, color):
        """fiasco_amd_renderer_surface_size: (surface width, surface height, bytes of a packed row) for a frame of
        width x height; FiascoError where the reference's loops would not fill the surface."""
        w, h, row = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_size_t()
        _check(self.lib, self.lib.L.fiasco_amd_renderer_surface_size(self.handle, width, height, 1 if color else 0, w, h, row))
        return w.value, h.value, row.value

    def render_planes(self, planes):
        """fiasco_amd_renderer_render_planes, the host loop: int16 numpy planes (H x W gray, 3 x H x W for Y, Cb, Cr; 12.4
        fixed point) -> the bytes of the packed surface."""
        import numpy
        planes = numpy.ascontiguousarray(planes, dtype=numpy.int16)
        if planes.ndim not in (2, 3) or (planes.ndim == 3 and planes.shape[0] not in (1, 3)):
            raise FiascoError("render_planes: int16 H x W or 3 x H x W expected, not %s" % (planes.shape,))
        color = planes.ndim == 3 and planes.shape[0] == 3
        h, w = planes.shape[-2:]
        _, sh, row = self.surface_size(w, h, color)
        buf = ctypes.create_string_buffer(sh * row)
        _check(self.lib, self.lib.L.fiasco_amd_renderer_render_planes(
            self.handle, planes.ctypes.data, 1 if color else 0, w, h, buf))
        return buf.raw

    def surface_size_420(self, width, height):
        """fiasco_amd_renderer_surface_size_420: (surface width, surface height, bytes of a packed row) for a 4:2:0 frame of
        width x height; FiascoError for an odd side, and at 24 bpp not doubled for a width that is no multiple of 4."""
        w, h, row = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_size_t()
        _check(self.lib, self.lib.L.fiasco_amd_renderer_surface_size_420(self.handle, width, height, w, h, row))
        return w.value, h.value, row.value

    def render_planes_420(self, y, cb, cr):
        """fiasco_amd_renderer_render_planes_420, the host loop: int16 numpy planes (12.4 fixed point) Y of H x W, Cb and Cr
        of H/2 x W/2 -> the bytes of the packed surface."""
        import numpy
        y, cb, cr = (numpy.ascontiguousarray(p, dtype=numpy.int16) for p in (y, cb, cr))
        if y.ndim != 2 or cb.shape != (y.shape[0] // 2, y.shape[1] // 2) or cr.shape != cb.shape:
            raise FiascoError("render_planes_420: int16 planes of H x W, H/2 x W/2 and H/2 x W/2 expected, not %s, %s, %s"
                              % (y.shape, cb.shape, cr.shape))
        h, w = y.shape
        _, sh, row = self.surface_size_420(w, h)
        buf = ctypes.create_string_buffer(sh * row)
        _check(self.lib, self.lib.L.fiasco_amd_renderer_render_planes_420(
            self.handle, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, w, h, buf))
        return buf.raw

    def delete(self):
        if self._fiasco:
            self.lib.L.fiasco_renderer_delete(self._fiasco)
            self._fiasco = None
        if self.handle:
            self.lib.L.fiasco_amd_renderer_delete(self.handle)
            self.handle = None


def render_planes_device_420(lib, renderer, y, cb, cr, surface, stream=None):
    """fiasco_amd_planes_render_device_420: the 4:2:0 rendering kernel alone.  `y`, `cb`, `cr`: packed int16 arrays on the GPU
    (12.4 fixed point) of H x W, H/2 x W/2 and H/2 x W/2; `surface`: as Batch.decode_rendered_420.  Runs on `stream`
    (default as decode_device) and waits for it."""
    (py, pcb, pcr), w, h = _planes_420("render_planes_device_420", y, cb, cr)
    arr = _device_surfaces([surface], renderer.bpp)
    if surface is None:
        raise FiascoError("render_planes_device_420: no surface")
    _check(lib, lib.L.fiasco_amd_planes_render_device_420(
        py, pcb, pcr, w, h, renderer.handle, arr, _stream_of([surface], stream)))


def render_planes_device(lib, renderer, planes, surface, stream=None):
    """fiasco_amd_planes_render_device: the rendering kernel alone.  `planes`: a packed int16 array on the GPU (12.4 fixed
    point), H x W or 3 x H x W; `surface`: as Batch.decode_rendered.  Runs on `stream` (default as decode_device) and waits
    for it."""
    address, shape = _packed_planes(None, planes)
    arr = _device_surfaces([surface], renderer.bpp)
    if surface is None:
        raise FiascoError("render_planes_device: no surface")
    _check(lib, lib.L.fiasco_amd_planes_render_device(
        address, 1 if len(shape) == 3 else 0, shape[-1], shape[-2], renderer.handle, arr, _stream_of([surface], stream)))


def magnified_size(lib, width, height, magnify):
    """fiasco_amd_magnified_size: (width, height) at which `dfiasco -m magnify` shows a frame of width x height --
    << magnify, or >> -magnify rounded up to even.  FiascoError with the reference's limit ("Maximum value is N." /
    "Minimum value is -N.") where the reference refuses.  A pure function; no device needed."""
    w, h = ctypes.c_uint(), ctypes.c_uint()
    _check(lib, lib.L.fiasco_amd_magnified_size(width, height, magnify, w, h))
    return w.value, h.value


def planes_to_pixels_device(lib, planes, target, stream=None):
    """fiasco_amd_planes_to_pixels_device: the decoder's last step alone.  `planes`: a packed int16 array on the GPU
    (12.4 fixed point), H x W for gray or 3 x H x W for Y, Cb, Cr; `target`: as Batch.decode_device.  The conversion
    runs on `stream` (default as decode_device)."""
    address, shape = _packed_planes(None, planes)
    arr = _device_targets([target])
    if (arr[0].height, arr[0].width) != shape[-2:]:
        raise FiascoError("target of %d x %d pixels for planes of %d x %d" % (arr[0].width, arr[0].height, shape[-1], shape[-2]))
    _check(lib, lib.L.fiasco_amd_planes_to_pixels_device(
        address, 1 if len(shape) == 3 else 0, arr, _stream_of([target], stream)))


def planes_to_420_device(lib, y, cb, cr, target, stream=None, order="nv12"):
    """fiasco_amd_planes_to_420_device: the 4:2:0 conversion kernel alone.  `y`, `cb`, `cr`: packed int16 arrays on the GPU
    (12.4 fixed point) of H x W, H/2 x W/2 and H/2 x W/2; `target` and `order` as Batch.decode_420.  Runs on `stream`
    (default as decode_device) and waits for it."""
    (py, pcb, pcr), w, h = _planes_420("planes_to_420_device", y, cb, cr)
    if target is None:
        raise FiascoError("planes_to_420_device: no target")
    arr = _device_targets_420([target], order)
    _check(lib, lib.L.fiasco_amd_planes_to_420_device(py, pcb, pcr, w, h, arr, _stream_of(list(target), stream)))


def planes_distortion_device(lib, a, b, stream=None):
    """fiasco_amd_planes_distortion_device: the measuring kernel alone.  `a`, `b`: two packed int16 arrays of one shape
    on the GPU (12.4 fixed point; torch tensors or anything with __cuda_array_interface__), H x W or 3 x H x W.  Returns
    (sse, maxdiff), three integers each (0 for bands the planes do not have).  Runs on `stream` (default as
    decode_device) and waits for the result."""
    (pa, shape), (pb, shape_b) = _packed_planes("a", a), _packed_planes("b", b)
    if shape != shape_b:
        raise FiascoError("planes of %s against planes of %s" % (shape, shape_b))
    s, m = (ctypes.c_ulonglong * 3)(), (ctypes.c_uint * 3)()
    _check(lib, lib.L.fiasco_amd_planes_distortion_device(
        pa, pb, 3 if len(shape) == 3 else 1, shape[-1], shape[-2], s, m, _stream_of([a], stream)))
    return list(s), list(m)


def smooth_planes_device(lib, planes, borders, smoothing, stream=None, fused=False):
    """fiasco_amd_smooth_planes_device: the smoothing step alone.  `planes`: a packed int16 array on the GPU (12.4 fixed
    point), H x W or 3 x H x W; its Y plane (the first) is changed in place along `borders`, (x, y, len, level, pass)
    tuples in the order of Batch.smoothing_borders(); `smoothing`: 0 .. 100 per cent.  Runs on `stream` (default as
    decode_device) and waits for it.  fused: fiasco_amd_smooth_planes_device_fused, all passes in one launch of the
    fused kernel (one workgroup) instead of one launch per pass; the same result."""
    address, shape = _packed_planes(None, planes)
    borders = list(borders)
    arr = (Border * max(len(borders), 1))()
    for k, b in enumerate(borders):
        arr[k].x, arr[k].y, arr[k].len, arr[k].level, arr[k].pass_ = b
    f = lib.L.fiasco_amd_smooth_planes_device_fused if fused else lib.L.fiasco_amd_smooth_planes_device
    _check(lib, f(address, shape[-1], shape[-2], arr, len(borders), smoothing, _stream_of([planes], stream)))


class Sequence:
    """fiasco_amd_seq_*: one video, this process searching and writing every world-th group of
    pictures (include/libfiasco_amd.h).  Frames: raw PNM bytes in display order."""

    def __init__(self, lib, pnm_list, quality=20.0, options=None, rank=0, world=1):
        n = len(pnm_list)
        self._bufs, self._lens = _pnm_arrays(pnm_list)              # borrowed by the C side, as the buffers in _keep are
        handle = lib.L.fiasco_amd_seq_open(n, self._bufs, self._lens, ctypes.c_float(quality), _handle(options), rank, world)
        self._opened(lib, handle, n, _pnm_geometry(pnm_list[0]) if n else None, (list(pnm_list), options), rank, world)

    def _opened(self, lib, handle, n, geom, keep, rank, world):
        """What every constructor ends in: the handle an open entry gave (FiascoError if it gave none), the number of frames,
        (width, height, bands) of a frame, and what the C side borrows until free()."""
        L = self.L = lib.L
        self.lib, self._keep, self._geom = lib, keep, geom
        self.handle = _check(lib, handle)
        self.n = n                                                  # frames in display order
        self.rank, self.world = rank, world
        self.gops = L.fiasco_amd_seq_gops(self.handle)
        self.frames = L.fiasco_amd_seq_frames(self.handle)
        self.ycol_size = L.fiasco_amd_seq_ycol_size(self.handle)
        self.initial_level = L.fiasco_amd_seq_initial_level(self.handle)
        self._outputs = None                                        # what set_outputs lent to the C side
        return self

    @classmethod
    def from_device(cls, lib, frames, quality=20.0, options=None, rank=0, world=1, stream=None):
        """fiasco_amd_seq_open_device: a video whose frames already live in device memory, in display order; frames
        as Batch.from_device takes them (torch uint8 tensors or anything with __cuda_array_interface__; pitch and
        plane stride come from the strides).  Open converts the frames this rank searches and waits for that: the
        sources may be overwritten right after the call.  The objects are kept alive until free()."""
        _need(lib, "fiasco_amd_seq_open_device", "videos in device memory need the HIP library")
        frames = list(frames)
        arr = _device_frames(frames)
        handle = lib.L.fiasco_amd_seq_open_device(len(frames), arr, _stream_of(frames, stream), ctypes.c_float(quality),
                                                  _handle(options), rank, world)
        geom = (arr[0].width, arr[0].height, 1 if arr[0].layout == FIASCO_AMD_GRAY8 else 3)
        return cls.__new__(cls)._opened(lib, handle, len(frames), geom, (frames, options), rank, world)

    @classmethod
    def from_ycbcr(cls, lib, frames, quality=20.0, options=None, rank=0, world=1, order="nv12"):
        """fiasco_amd_seq_open_ycbcr: a video of frames that are YCbCr already, in host memory and display order; frames as
        Batch.from_ycbcr takes them.  The frames are converted during the call."""
        _need(lib, "fiasco_amd_seq_open_ycbcr")
        frames = [tuple(f) for f in frames]
        arr = _ycbcr_frames(frames, order, "__array_interface__")
        handle = lib.L.fiasco_amd_seq_open_ycbcr(len(frames), arr, ctypes.c_float(quality), _handle(options), rank, world)
        return cls.__new__(cls)._opened(lib, handle, len(frames), (arr[0].width, arr[0].height, 3), (None, options), rank, world)

    @classmethod
    def from_device_ycbcr(cls, lib, frames, quality=20.0, options=None, rank=0, world=1, stream=None, order="nv12"):
        """fiasco_amd_seq_open_device_ycbcr: from_device with frames that are YCbCr already, as Batch.from_device_ycbcr takes
        them.  Open converts the frames this rank searches and waits for that."""
        _need(lib, "fiasco_amd_seq_open_device_ycbcr", "videos in device memory need the HIP library")
        frames = [tuple(f) for f in frames]
        arr = _ycbcr_frames(frames, order, "__cuda_array_interface__")
        handle = lib.L.fiasco_amd_seq_open_device_ycbcr(len(frames), arr, _stream_over(frames, stream, tuples=True),
                                                        ctypes.c_float(quality), _handle(options), rank, world)
        geom = (arr[0].width, arr[0].height, 3)
        return cls.__new__(cls)._opened(lib, handle, len(frames), geom, (frames, options), rank, world)

    def set_outputs(self, targets=None, distortion=False, stream=None):
        """fiasco_amd_seq_set_outputs_device: from now on every search reconstructs every frame of the GOPs it searches
        and delivers it on the device.  targets: one writable GPU array per display frame as Batch.decode_device takes
        them (None entries: not this frame), or None; distortion: measure every frame against its original
        (distortion() hands the sums out).  Neither: no outputs again.  The arrays live in this object."""
        import numpy
        _need(self.lib, "fiasco_amd_seq_set_outputs_device", "device outputs need the HIP library")
        if targets is None and not distortion:
            _check(self.lib, self.L.fiasco_amd_seq_set_outputs_device(self.handle, None))
            self._outputs = None
            return
        c = ctypes
        o = SeqOutputs()
        keep = {"struct": o, "targets": None, "arr": None, "sse": None, "maxdiff": None}
        if targets is not None:
            targets = list(targets)
            if len(targets) != self.n:
                raise FiascoError("set_outputs: %d targets for a sequence of %d frames" % (len(targets), self.n))
            keep["targets"], keep["arr"] = targets, _device_targets(targets)
            o.targets = keep["arr"]
        if distortion:
            keep["sse"] = numpy.zeros((self.n, 3), dtype=numpy.uint64)
            keep["maxdiff"] = numpy.zeros((self.n, 3), dtype=numpy.uint32)
            o.sse = keep["sse"].ctypes.data_as(c.POINTER(c.c_ulonglong))
            o.maxdiff = keep["maxdiff"].ctypes.data_as(c.POINTER(c.c_uint))
        keep["written"] = numpy.zeros(self.n, dtype=numpy.uint8)
        o.written = keep["written"].ctypes.data_as(c.POINTER(c.c_ubyte))
        st = _stream_over(targets, stream)
        o.stream = st.value if st is not None else None
        # where this is refused nothing was set: what was lent before stays lent
        _check(self.lib, self.L.fiasco_amd_seq_set_outputs_device(self.handle, c.byref(o)))
        self._outputs = keep

    def distortion(self):
        """(sse, maxdiff, written) of the last searches: numpy arrays [n, 3], [n, 3] and [n] by display frame (copies).
        sse and maxdiff are None unless set_outputs(distortion=True)."""
        if self._outputs is None:
            raise FiascoError("distortion: no outputs are set (set_outputs)")
        k = self._outputs
        return (None if k["sse"] is None else k["sse"].copy(), None if k["maxdiff"] is None else k["maxdiff"].copy(),
                k["written"].copy())

    def encode(self):
        """fiasco_amd_seq_encode: probe, search, verify and write in one process (world == 1); the whole stream, the
        bytes fiasco_coder() writes."""
        return _one_stream(self.lib, lambda out, n: self.L.fiasco_amd_seq_encode(self.handle, out, n))

    def keep_reconstructed(self, keep=True):
        """fiasco_amd_seq_keep_reconstructed: the searches keep the coder's reconstruction of every frame on the host."""
        _check(self.lib, self.L.fiasco_amd_seq_keep_reconstructed(self.handle, 1 if keep else 0))

    def reconstructed_planes(self, display):
        """fiasco_amd_seq_reconstructed_planes: (int16 [bands, h, w] 12.4 fixed point, frame type 0 I / 1 P / 2 B)."""
        import numpy
        w, h, bands = self._geom
        out = numpy.empty((bands, h, w), dtype=numpy.int16)
        t = ctypes.c_int(-1)
        _check(self.lib, self.L.fiasco_amd_seq_reconstructed_planes(self.handle, display, out.ctypes.data, t))
        return out, t.value

    def gop_of(self, frame):
        return self.L.fiasco_amd_seq_gop_of(self.handle, frame)

    def probe(self):
        """Level to speculate for the GOPs behind the first: what frame 0 alone leaves."""
        lv = ctypes.c_uint()
        _check(self.lib, self.L.fiasco_amd_seq_probe(self.handle, lv))
        return lv.value

    def search(self, carry_in, todo):
        c = ctypes
        ci = (c.c_uint * self.gops)(*carry_in)
        td = (c.c_ubyte * self.gops)(*[1 if t else 0 for t in todo])
        _check(self.lib, self.L.fiasco_amd_seq_search(self.handle, ci, td))

    def gop_result(self, gop):
        """(minimum level the GOP left, failed, message) -- None if the GOP was not searched here."""
        c = ctypes
        out, failed = c.c_uint(), c.c_int()
        if not self.L.fiasco_amd_seq_gop_result(self.handle, gop, out, failed):
            return None
        return out.value, bool(failed.value), self.lib.error_message() if failed.value else ""

    def ycol(self, frame):
        p = self.L.fiasco_amd_seq_ycol(self.handle, frame)
        return ctypes.string_at(p, self.ycol_size) if p and self.ycol_size else None

    def write(self, frame, ycol=None):
        return _one_stream(self.lib, lambda out, n: self.L.fiasco_amd_seq_write(self.handle, frame, ycol, out, n))

    def free(self):
        if self.handle:
            self.L.fiasco_amd_seq_free(self.handle)
            self.handle = None


class Stream:
    """A .fco stream that was read (include/libfiasco_amd_stream.h): `data` is the stream as bytes, or -- with
    filename=True -- the name of its file.  Opening parses and validates every frame; a stream that fails raises
    FiascoError with the reader's message."""

    def __init__(self, lib, data, filename=False):
        self.lib = lib
        if not hasattr(lib.L, "fiasco_amd_stream_open"):
            raise FiascoError("%s has no stream reader" % lib.path)
        if filename:
            self.handle = lib.L.fiasco_amd_stream_open_file(os.fsencode(data))
        else:
            data = bytes(data)
            self.handle = lib.L.fiasco_amd_stream_open(data, len(data))
        _check(lib, self.handle)
        raw = StreamInfo()
        _check(lib, lib.L.fiasco_amd_stream_get_info(self.handle, ctypes.byref(raw)))
        self.info = {name: getattr(raw, name) for name, _ in StreamInfo._fields_}
        for name in ("title", "comment", "basis_name"):
            self.info[name] = (self.info[name] or b"").decode("latin-1")
        self.n = raw.frames
        self.frame_types = [lib.L.fiasco_amd_stream_frame_type(self.handle, d) for d in range(self.n)]
        order = (ctypes.c_uint * max(self.n, 1))()
        if lib.L.fiasco_amd_stream_coding_order(self.handle, order, self.n) != self.n:
            raise FiascoError(lib.error_message())
        self.coding_order = list(order[:self.n])

    def _size(self, magnify):
        w, h = self.info["width"], self.info["height"]
        return magnified_size(self.lib, w, h, magnify) if magnify else (w, h)

    def rewrite(self):
        """fiasco_amd_stream_rewrite: every frame through the writer again; for a stream a coder wrote, its bytes."""
        return _one_stream(self.lib, lambda out, n: self.lib.L.fiasco_amd_stream_rewrite(self.handle, out, n))

    def smoothing_borders(self, display, magnify=0, format_420=False):
        """fiasco_amd_stream_smoothing_borders: the borders `dfiasco -m magnify` smooths display frame `display` along,
        (x, y, len, level, pass) as Batch.smoothing_borders() lists them; format_420: as Batch.smoothing_borders_420()."""
        return _borders(self.lib, lambda out, cap: self.lib.L.fiasco_amd_stream_smoothing_borders(
            self.handle, display, magnify, int(bool(format_420)), out, cap))

    def decode_device(self, targets, first=0, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_stream_decode_device: display frames first .. first + len(targets) - 1 as `dfiasco -m magnify -s
        smoothing -o` writes them, P and B frames included, into `targets` (as Batch.decode_shown takes them; None: not
        this frame).  Returns the number of frames written; a frame that fails takes the frames predicted from it along
        and lib.error_message() names the first and the cause."""
        targets = list(targets)
        arr = _device_targets(targets)
        return _check(self.lib, self.lib.L.fiasco_amd_stream_decode_device(
            self.handle, first, len(targets), magnify, smoothing, arr, _stream_over(targets, stream)))

    def decode_420(self, targets, first=0, magnify=0, smoothing=-1, stream=None, order="nv12"):
        """fiasco_amd_stream_decode_device_420: the same in 4:2:0, into targets as Batch.decode_420 takes them."""
        targets = list(targets)
        arr = _device_targets_420(targets, order)
        return _check(self.lib, self.lib.L.fiasco_amd_stream_decode_device_420(
            self.handle, first, len(targets), magnify, smoothing, arr, _stream_over(targets, stream, tuples=True)))

    def decode_planes(self, display, magnify=0):
        """fiasco_amd_stream_decode_planes: the unsmoothed planes of display frame `display` at `magnify`, int16
        [bands, h, w] (12.4 fixed point); the frames it is predicted from are decoded on the way."""
        import numpy
        w, h = self._size(magnify)
        out = numpy.empty((3 if self.info["color"] else 1, h, w), dtype=numpy.int16)
        _check(self.lib, self.lib.L.fiasco_amd_stream_decode_planes(self.handle, display, magnify, out.ctypes.data))
        return out

    def decode_planes_420(self, display, magnify=0):
        """fiasco_amd_stream_decode_planes_420: the same decoded in 4:2:0: Y [h, w], Cb and Cr [h / 2, w / 2]."""
        out, planes = _empty_planes_420(*self._size(magnify))
        _check(self.lib, self.lib.L.fiasco_amd_stream_decode_planes_420(self.handle, display, magnify, out.ctypes.data))
        return planes

    def free(self):
        if self.handle:
            self.lib.L.fiasco_amd_stream_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Image:
    """fiasco_image_t (include/libfiasco_amd_decoder.h): a frame Decoder.get_frame() handed out, whose 12.4 planes live in
    device memory, or a PNM file (Image.open), whose planes live on the host until device_planes() uploads them.  delete()
    releases it; an image may outlive its decoder."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle
        # fiasco_image_get_height returns the width, as the reference's does
        self.width, self.height = lib.L.fiasco_image_get_width(handle), lib.L.fiasco_amd_image_get_height(handle)
        self.color = bool(lib.L.fiasco_image_is_color(handle))
        self.format_420 = lib.L.fiasco_amd_image_format(handle) == 1

    @classmethod
    def open(cls, lib, path):
        """fiasco_image_new: a raw PGM / PPM file (looked up in FIASCO_IMAGES) as an image."""
        _need(lib, "fiasco_image_new", "the decoder half of fiasco.h")
        return cls(lib, _check(lib, lib.L.fiasco_image_new(os.fsencode(path))))

    def planes(self):
        """fiasco_amd_image_planes: the planes on the host, int16 12.4 fixed point: [bands, h, w], or for a 4:2:0 image the
        tuple Y [h, w], Cb and Cr [h / 2, w / 2] -- what the reference's fiasco_decoder_get_frame() hands out."""
        import numpy
        if self.format_420:
            out, planes = _empty_planes_420(self.width, self.height)
        else:
            out = planes = numpy.empty((3 if self.color else 1, self.height, self.width), dtype=numpy.int16)
        _check(self.lib, self.lib.L.fiasco_amd_image_planes(self.handle, out.ctypes.data))
        return planes

    def device_planes(self):
        """fiasco_amd_image_planes_device: ([address of Y, Cb, Cr or None], device) of the planes where they live; the
        memory belongs to the image."""
        planes, device = (ctypes.c_void_p * 3)(), ctypes.c_int(-1)
        _check(self.lib, self.lib.L.fiasco_amd_image_planes_device(self.handle, planes, ctypes.byref(device)))
        return [planes[b] for b in range(3)], device.value

    def _surface_size(self, renderer):
        return renderer.surface_size_420(self.width, self.height) if self.format_420 else renderer.surface_size(self.width, self.height, self.color)

    def render(self, renderer):
        """fiasco_renderer_render with the fiasco_renderer_t of `renderer` (a Renderer): the bytes of the packed XImage."""
        _, sh, row = self._surface_size(renderer)
        buf = ctypes.create_string_buffer(sh * row)
        _check(self.lib, self.lib.L.fiasco_renderer_render(renderer.fiasco_renderer(), buf, self.handle))
        return buf.raw

    def render_device(self, renderer, surface, stream=None):
        """fiasco_amd_renderer_render_device: into `surface`, a writable uint8 GPU array as Batch.decode_rendered takes it,
        on `stream` (default as decode_device)."""
        if surface is None:
            raise FiascoError("render_device: no surface")
        arr = _device_surfaces([surface], renderer.bpp)
        _check(self.lib, self.lib.L.fiasco_amd_renderer_render_device(renderer.fiasco_renderer(), arr, self.handle, _stream_of([surface], stream)))

    def delete(self):
        if self.handle:
            self.lib.L.fiasco_image_delete(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass


class Decoder:
    """fiasco_decoder_t (include/libfiasco_amd_decoder.h): a .fco stream played display frame by display frame on the
    device.  `source`: the stream as bytes, or the name of its file (looked up in FIASCO_DATA).  smoothing: -1 the header's
    value, 0 none, 1 .. 100 per cent, None: the default of fiasco_d_options_new (70); read_ahead: how many display frames
    one call may decode (fiasco_amd_decoder_set_read_ahead).  Iterating yields the remaining frames as Images."""

    def __init__(self, lib, source, smoothing=None, magnify=0, format_420=False, read_ahead=32):
        self.lib, self.handle = lib, None
        _need(lib, "fiasco_decoder_new", "the decoder half of fiasco.h")
        options = _check(lib, lib.L.fiasco_d_options_new())
        try:
            if smoothing is not None:
                _check(lib, lib.L.fiasco_d_options_set_smoothing(options, smoothing))
            _check(lib, lib.L.fiasco_d_options_set_magnification(options, magnify))
            _check(lib, lib.L.fiasco_d_options_set_4_2_0_format(options, 1 if format_420 else 0))
            if isinstance(source, (bytes, bytearray, memoryview)):
                source = bytes(source)
                self.handle = lib.L.fiasco_amd_decoder_new_memory(source, len(source), options)
            else:
                self.handle = lib.L.fiasco_decoder_new(os.fsencode(source), options)
            _check(lib, self.handle)
        finally:
            lib.L.fiasco_d_options_delete(options)
        _check(lib, lib.L.fiasco_amd_decoder_set_read_ahead(self.handle, read_ahead))
        L, h = lib.L, self.handle
        self.width, self.height, self.color = L.fiasco_decoder_get_width(h), L.fiasco_decoder_get_height(h), bool(L.fiasco_decoder_is_color(h))
        self.rate, self.length = L.fiasco_decoder_get_rate(h), L.fiasco_decoder_get_length(h)
        self.title = (L.fiasco_decoder_get_title(h) or b"").decode("latin-1")
        self.comment = (L.fiasco_decoder_get_comment(h) or b"").decode("latin-1")

    def get_frame(self):
        """fiasco_decoder_get_frame: the next display frame as an Image.  FiascoError for a frame that fails -- it is
        consumed, the next call goes on behind it -- and behind the last frame."""
        return Image(self.lib, _check(self.lib, self.lib.L.fiasco_decoder_get_frame(self.handle)))

    def write_frame(self, path):
        """fiasco_decoder_write_frame: the next display frame, decoded in 4:4:4, as a raw PGM / PPM file."""
        _check(self.lib, self.lib.L.fiasco_decoder_write_frame(self.handle, os.fsencode(path)))

    @property
    def position(self):
        """fiasco_amd_decoder_position: the display frames consumed so far -- handed out, written or failed; a call that is
        refused as a whole consumes nothing."""
        return self.lib.L.fiasco_amd_decoder_position(self.handle)

    def __iter__(self):
        while self.position < self.length:
            yield self.get_frame()

    def delete(self):
        if self.handle:
            self.lib.L.fiasco_decoder_delete(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.delete()
        except Exception:
            pass


class COptions:
    """fiasco_c_options_t with the reference's setter names (fiasco.h:132-174)."""

    def __init__(self, lib):
        self.lib = lib
        self.handle = lib.L.fiasco_c_options_new()
        _check(lib, self.handle)

    def _call(self, name, *args):
        conv = [a.encode() if isinstance(a, str) else a for a in args]
        return _check(self.lib, getattr(self.lib.L, "fiasco_c_options_" + name)(self.handle, *conv))

    def delete(self):
        if self.handle:
            self.lib.L.fiasco_c_options_delete(self.handle)
            self.handle = None

    def __getattr__(self, name):
        if name.startswith("set_"):
            return lambda *a: self._call(name, *a)
        raise AttributeError(name)


_default = None


def library():
    """The product library (HIP hot path).  Raises if it has not been built."""
    global _default
    if _default is None:
        _default = Library(LIB_PATH)
        if _default.core_name() != "hip-gfx950":
            raise FiascoError("libfiasco_amd.so is not linked against the HIP device coder")
    return _default


def fiasco_coder(inputnames, outputname, quality=20.0, options=None):
    return library().fiasco_coder(inputnames, outputname, quality, options)


def encode_batch(pnm_list, quality=20.0, options=None):
    return library().encode_batch(pnm_list, quality, options)
