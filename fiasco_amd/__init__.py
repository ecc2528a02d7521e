"""fiasco_amd -- MI355X-native FIASCO encoder hot path behind the libfiasco C API.

Python here is plumbing only: a ctypes mirror of the C-ABI shared library
``libfiasco_amd.so`` (host C + hand-written HIP for gfx950).  The names follow the
reference interface (``fiasco_coder``, ``fiasco_c_options_set_*``; reference fiasco.h:303-398)
so that tests read like calls into the reference library.

There is no CPU fallback: ``fiasco_coder`` / ``encode_batch`` fail (return 0 / raise) when
the HIP device coder cannot run.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfiasco_amd.so")
CSRC = os.path.join(_HERE, "csrc")

# enums (values are ABI, include/libfiasco_amd.h)
FIASCO_NO_VERBOSITY, FIASCO_SOME_VERBOSITY, FIASCO_ULTIMATE_VERBOSITY = 0, 1, 2
FIASCO_TILING_SPIRAL_ASC, FIASCO_TILING_SPIRAL_DSC = 0, 1
FIASCO_TILING_VARIANCE_ASC, FIASCO_TILING_VARIANCE_DSC = 2, 3
FIASCO_RPF_RANGE_0_75, FIASCO_RPF_RANGE_1_00, FIASCO_RPF_RANGE_1_50, FIASCO_RPF_RANGE_2_00 = 0, 1, 2, 3
FIASCO_PROGRESS_NONE, FIASCO_PROGRESS_BAR, FIASCO_PROGRESS_PERCENT = 0, 1, 2

# pixel layouts of a frame in device memory (include/libfiasco_amd_hip.h)
FIASCO_AMD_GRAY8, FIASCO_AMD_RGB8_INTERLEAVED, FIASCO_AMD_RGB8_PLANAR = 0, 1, 2


class DeviceFrame(ctypes.Structure):
    """struct fiasco_amd_device_frame (include/libfiasco_amd_hip.h)."""
    _fields_ = [("data", ctypes.c_void_p), ("pitch", ctypes.c_size_t), ("plane_stride", ctypes.c_size_t),
                ("width", ctypes.c_uint), ("height", ctypes.c_uint), ("layout", ctypes.c_int)]


class Border(ctypes.Structure):
    """struct fiasco_amd_border (include/libfiasco_amd.h): one border smooth_image blends, 8 bytes."""
    _fields_ = [("x", ctypes.c_uint16), ("y", ctypes.c_uint16), ("len", ctypes.c_uint16),
                ("level", ctypes.c_uint8), ("pass_", ctypes.c_uint8)]


class DeviceTarget(ctypes.Structure):
    """struct fiasco_amd_device_target (include/libfiasco_amd_hip.h): a DeviceFrame whose memory is written."""
    _fields_ = DeviceFrame._fields_


class DeviceSurface(ctypes.Structure):
    """struct fiasco_amd_device_surface (include/libfiasco_amd_render.h): a display surface in device memory."""
    _fields_ = [("data", ctypes.c_void_p), ("pitch", ctypes.c_size_t), ("width", ctypes.c_uint), ("height", ctypes.c_uint)]


class DeviceTarget420(ctypes.Structure):
    """struct fiasco_amd_device_target_420 (include/libfiasco_amd_420.h): where a 4:2:0 frame goes in device memory."""
    _fields_ = [("y", ctypes.c_void_p), ("y_pitch", ctypes.c_size_t), ("cb", ctypes.c_void_p), ("cr", ctypes.c_void_p),
                ("c_pitch", ctypes.c_size_t), ("c_step", ctypes.c_uint), ("width", ctypes.c_uint), ("height", ctypes.c_uint)]


class YCbCrFrame(ctypes.Structure):
    """struct fiasco_amd_ycbcr_frame (include/libfiasco_amd_ycbcr.h): a frame that is YCbCr already, in host or device memory."""
    _fields_ = [("y", ctypes.c_void_p), ("y_pitch", ctypes.c_size_t), ("cb", ctypes.c_void_p), ("cr", ctypes.c_void_p),
                ("c_pitch", ctypes.c_size_t), ("c_step", ctypes.c_uint), ("subsampling", ctypes.c_uint),
                ("width", ctypes.c_uint), ("height", ctypes.c_uint)]


class SeqOutputs(ctypes.Structure):
    """struct fiasco_amd_seq_outputs (include/libfiasco_amd_video.h)."""
    _fields_ = [("targets", ctypes.POINTER(DeviceTarget)), ("sse", ctypes.POINTER(ctypes.c_ulonglong)),
                ("maxdiff", ctypes.POINTER(ctypes.c_uint)), ("written", ctypes.POINTER(ctypes.c_ubyte)),
                ("stream", ctypes.c_void_p)]


class StreamInfo(ctypes.Structure):
    """struct fiasco_amd_stream_info (include/libfiasco_amd_stream.h): what the header of a stream says."""
    _fields_ = [("width", ctypes.c_uint), ("height", ctypes.c_uint), ("color", ctypes.c_int), ("frames", ctypes.c_uint),
                ("fps", ctypes.c_uint), ("smoothing", ctypes.c_uint), ("title", ctypes.c_char_p), ("comment", ctypes.c_char_p),
                ("basis_name", ctypes.c_char_p), ("rpf_mantissa", ctypes.c_uint), ("dc_rpf_mantissa", ctypes.c_uint),
                ("d_rpf_mantissa", ctypes.c_uint), ("d_dc_rpf_mantissa", ctypes.c_uint), ("B_as_past_ref", ctypes.c_int),
                ("half_pixel", ctypes.c_int)]


class Stats(ctypes.Structure):
    """struct fiasco_amd_stats (include/libfiasco_amd_hip.h)."""
    _fields_ = [("kernel_ms", ctypes.c_double), ("launches", ctypes.c_ulonglong),
                ("frames", ctypes.c_ulonglong), ("bytes_mp", ctypes.c_ulonglong),
                ("bytes_img", ctypes.c_ulonglong), ("bytes_gram", ctypes.c_ulonglong),
                ("n_mp", ctypes.c_ulonglong), ("n_steps", ctypes.c_ulonglong),
                ("n_blocks", ctypes.c_ulonglong), ("n_appends", ctypes.c_ulonglong),
                ("n_fulleval", ctypes.c_ulonglong), ("t_init", ctypes.c_ulonglong),
                ("t_approx", ctypes.c_ulonglong), ("t_ipis", ctypes.c_ulonglong),
                ("t_append", ctypes.c_ulonglong), ("t_serial", ctypes.c_ulonglong),
                ("t_total", ctypes.c_ulonglong), ("t_mpA", ctypes.c_ulonglong),
                ("t_mpB", ctypes.c_ulonglong), ("n_blockevals", ctypes.c_ulonglong),
                ("dbg", ctypes.c_ulonglong * 8), ("states_sum", ctypes.c_ulonglong),
                ("states_max", ctypes.c_ulonglong), ("reencodes", ctypes.c_ulonglong),
                ("frames_by_build", ctypes.c_ulonglong * 5),
                ("spec_frames", ctypes.c_ulonglong), ("spec_tasks", ctypes.c_ulonglong),
                ("spec_confirmed", ctypes.c_ulonglong), ("spec_wrong", ctypes.c_ulonglong),
                ("spec_timeout", ctypes.c_ulonglong), ("spec_inline", ctypes.c_ulonglong),
                ("spec_wait", ctypes.c_ulonglong), ("spec_tab_used", ctypes.c_ulonglong),
                ("spec_tab_missed", ctypes.c_ulonglong), ("spec_adopted", ctypes.c_ulonglong),
                ("decoder_frames", ctypes.c_ulonglong), ("decoder_bytes", ctypes.c_ulonglong),
                ("decoder_us", ctypes.c_ulonglong), ("coop_frames", ctypes.c_ulonglong),
                ("coop_workgroups", ctypes.c_ulonglong),
                ("spec_app_rows", ctypes.c_ulonglong), ("spec_app_wait", ctypes.c_ulonglong)]


def _abi():
    """name -> (restype, [argtypes]) of every function include/libfiasco_amd.h and include/libfiasco_amd_hip.h declare.
    Handles (options, batches, sequences), streams and planes travel as void pointers; buffers the callers make with
    create_string_buffer, and names, as char pointers."""
    c = ctypes
    P, ptr, cstr, i, u, f32, size, ull = c.POINTER, c.c_void_p, c.c_char_p, c.c_int, c.c_uint, c.c_float, c.c_size_t, c.c_ulonglong
    pnm = [P(cstr), P(size)]                   # raw PNM buffers and their lengths
    streams = [P(ptr), P(size)]                # the .fco byte strings a call hands back, and their lengths
    frames, targets = P(DeviceFrame), P(DeviceTarget)
    return {
        # the reference's interface (fiasco.h) and the two symbols its CLI objects import
        "fiasco_get_error_message": (cstr, []),
        "fiasco_set_verbosity": (None, [i]),
        "fiasco_get_verbosity": (i, []),
        "fiasco_coder": (i, [P(cstr), cstr, f32, ptr]),
        "fiasco_c_options_new": (ptr, []),
        "fiasco_c_options_delete": (None, [ptr]),
        "fiasco_c_options_set_smoothing": (i, [ptr, i]),
        "fiasco_c_options_set_frame_pattern": (i, [ptr, cstr]),
        "fiasco_c_options_set_tiling": (i, [ptr, i, u]),
        "fiasco_c_options_set_basisfile": (i, [ptr, cstr]),
        "fiasco_c_options_set_chroma_quality": (i, [ptr, f32, u]),
        "fiasco_c_options_set_optimizations": (i, [ptr, u, u, u, u, u]),
        "fiasco_c_options_set_prediction": (i, [ptr, i, u, u]),
        "fiasco_c_options_set_video_param": (i, [ptr, u, i, i, i]),
        "fiasco_c_options_set_quantization": (i, [ptr, u, i, u, i]),
        "fiasco_c_options_set_progress_meter": (i, [ptr, i]),
        "fiasco_c_options_set_comment": (i, [ptr, cstr]),
        "fiasco_c_options_set_title": (i, [ptr, cstr]),
        "fiasco_calloc": (ptr, [size, size]),
        "open_file": (ptr, [cstr, cstr, i]),
        # limits, models, batches of stills
        "fiasco_amd_set_limits": (i, [u, u]),
        "fiasco_amd_get_limits": (None, [P(u), P(u)]),
        "fiasco_amd_c_options_set_models": (i, [ptr, cstr, cstr, cstr, cstr]),
        "fiasco_amd_encode_batch": (i, [u] + pnm + [f32, ptr] + streams),
        "fiasco_amd_free": (None, [ptr]),
        "fiasco_amd_batch_stage": (ptr, [u] + pnm + [f32, ptr]),
        "fiasco_amd_batch_encode": (i, [ptr] + streams),
        "fiasco_amd_batch_submit": (i, [ptr]),
        "fiasco_amd_batch_collect": (i, [ptr] + streams + [i]),
        "fiasco_amd_batch_upload": (i, [ptr] + pnm),
        "fiasco_amd_batch_stats": (i, [ptr, u, u, P(f32), P(f32), P(u), P(u)]),
        "fiasco_amd_batch_free": (None, [ptr]),
        # the decoder's outlets on a finished batch
        "fiasco_amd_batch_decode_psnr": (i, [ptr, u, P(c.c_double), P(c.c_double)]),
        "fiasco_amd_batch_decode_psnr_all": (i, [ptr, P(c.c_double), P(c.c_double)]),
        "fiasco_amd_batch_decode_plane": (i, [ptr, u, u, cstr]),
        "fiasco_amd_batch_decode_planes": (i, [ptr, u, ptr]),
        "fiasco_amd_batch_decode_planes_magnified": (i, [ptr, u, i, ptr]),
        "fiasco_amd_magnified_size": (i, [u, u, i, P(u), P(u)]),
        "fiasco_amd_batch_smoothing_borders": (i, [ptr, u, P(Border), u]),
        # sequences across processes
        "fiasco_amd_seq_open": (ptr, [u] + pnm + [f32, ptr, u, u]),
        "fiasco_amd_seq_free": (None, [ptr]),
        "fiasco_amd_seq_gops": (u, [ptr]),
        "fiasco_amd_seq_frames": (u, [ptr]),
        "fiasco_amd_seq_gop_of": (u, [ptr, u]),
        "fiasco_amd_seq_ycol_size": (u, [ptr]),
        "fiasco_amd_seq_initial_level": (u, [ptr]),
        "fiasco_amd_seq_probe": (i, [ptr, P(u)]),
        "fiasco_amd_seq_search": (i, [ptr, P(u), P(c.c_ubyte)]),
        "fiasco_amd_seq_gop_result": (i, [ptr, u, P(u), P(i)]),
        "fiasco_amd_seq_ycol": (ptr, [ptr, u]),
        "fiasco_amd_seq_write": (i, [ptr, u, cstr] + streams),
        # the device core: counters, launch policy, devices
        "fiasco_amd_get_stats": (None, [P(Stats)]),
        "fiasco_amd_reset_stats": (None, []),
        "fiasco_amd_release_memory": (None, []),
        "fiasco_amd_core_name": (cstr, []),
        "fiasco_amd_spec_workgroups": (i, [u, i, i, i, i]),
        "fiasco_amd_spec_append_helpers": (i, [u, i, i, i]),
        "fiasco_amd_coop_workgroups": (u, [u, i]),
        "fiasco_amd_share_of": (u, [u, u, u]),
        "fiasco_amd_set_device": (i, [i]),
        "fiasco_amd_set_devices": (i, [P(i), i]),
        "fiasco_amd_device_count": (i, []),
        "fiasco_amd_rccl_gather": (i, [ptr, ptr, i, i, i, u] + pnm + [P(P(ptr)), P(P(size)), P(u)]),
        "fiasco_amd_selftest_log2": (i, [u, u, P(ull), P(ull), P(ull), P(f32)]),
        "fiasco_amd_selftest_log2_patched": (i, [u, u, P(ull), P(ull), P(ull)]),
        "fiasco_amd_selftest_log2_max_ulp": (ull, []),
        # frames in device memory, in and out
        "fiasco_amd_batch_stage_device": (ptr, [u, frames, ptr, f32, ptr]),
        "fiasco_amd_batch_upload_device": (i, [ptr, frames, ptr]),
        "fiasco_amd_batch_input_planes": (i, [ptr, u, ptr]),
        "fiasco_amd_batch_decode_device": (i, [ptr, targets, ptr]),
        "fiasco_amd_batch_decode_device_magnified": (i, [ptr, i, targets, ptr]),
        "fiasco_amd_batch_decode_device_thumbnails": (i, [ptr, targets, u, targets, ptr]),
        "fiasco_amd_planes_to_pixels_device": (i, [ptr, i, targets, ptr]),
        "fiasco_amd_batch_decode_distortion_device": (i, [ptr, P(ull), P(u), targets, ptr]),
        "fiasco_amd_planes_distortion_device": (i, [ptr, ptr, i, u, u, P(ull), P(u), ptr]),
    }


def _video_abi():
    """the same for include/libfiasco_amd_video.h: the whole stream of a sequence in one call and its reconstructed frames
    on the host (every build of the library), videos in device memory in and out (the HIP library)"""
    c = ctypes
    P, ptr, i, u, f32, size = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.c_float, c.c_size_t
    return {
        "fiasco_amd_seq_encode": (i, [ptr, P(ptr), P(size)]),
        "fiasco_amd_seq_keep_reconstructed": (i, [ptr, i]),
        "fiasco_amd_seq_reconstructed_planes": (i, [ptr, u, ptr, P(i)]),
        "fiasco_amd_seq_open_device": (ptr, [u, P(DeviceFrame), ptr, f32, ptr, u, u]),
        "fiasco_amd_seq_set_outputs_device": (i, [ptr, P(SeqOutputs)]),
    }


def _smooth_abi():
    """the same for include/libfiasco_amd_smooth.h: decoded frames smoothed along their partition borders on the device,
    as the reference's decoder shows them (the HIP library)"""
    c = ctypes
    P, ptr, i, u, ull, targets = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.c_ulonglong, c.POINTER(DeviceTarget)
    return {
        "fiasco_amd_batch_decode_device_smoothed": (i, [ptr, i, targets, ptr]),
        "fiasco_amd_batch_decode_distortion_device_smoothed": (i, [ptr, i, P(ull), P(u), targets, ptr]),
        "fiasco_amd_smooth_planes_device": (i, [ptr, u, u, P(Border), u, i, ptr]),
    }


def _display_abi():
    """the same for include/libfiasco_amd_display.h: magnified frames and thumbnails smoothed as `dfiasco` shows them (the
    border list in every build of the library, the rest in the HIP library)"""
    c = ctypes
    P, ptr, i, u, ull, targets = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.c_ulonglong, c.POINTER(DeviceTarget)
    return {
        "fiasco_amd_batch_smoothing_borders_magnified": (i, [ptr, u, i, P(Border), u]),
        "fiasco_amd_batch_decode_device_shown": (i, [ptr, i, i, targets, ptr]),
        "fiasco_amd_batch_decode_device_thumbnails_shown": (i, [ptr, i, targets, u, targets, ptr]),
        "fiasco_amd_smooth_planes_device_fused": (i, [ptr, u, u, P(Border), u, i, ptr]),
        "fiasco_amd_smooth_fused": (i, [ull, u]),
    }


def _render_abi():
    """the same for include/libfiasco_amd_render.h: decoded frames in the pixel formats of a display, as the reference's
    renderer writes them into an XImage (the handle, the size and the host loop in host code that needs no device; the kernel
    and the batch entry in the HIP library)"""
    c = ctypes
    P, ptr, i, u, ul, size, surfaces = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.c_ulong, c.c_size_t, c.POINTER(DeviceSurface)
    return {
        "fiasco_amd_renderer_new": (ptr, [ul, ul, ul, u, i]),
        "fiasco_amd_renderer_delete": (None, [ptr]),
        "fiasco_amd_renderer_surface_size": (i, [ptr, u, u, i, P(u), P(u), P(size)]),
        "fiasco_amd_renderer_render_planes": (i, [ptr, ptr, i, u, u, ptr]),
        "fiasco_amd_planes_render_device": (i, [ptr, i, u, u, ptr, surfaces, ptr]),
        "fiasco_amd_batch_decode_device_rendered": (i, [ptr, ptr, i, i, surfaces, ptr]),
    }


def _render420_abi():
    """the same for include/libfiasco_amd_render_420.h: frames decoded in 4:2:0 in the pixel formats of a display (the size
    rule and the host loop in host code that needs no device; the kernel and the batch entry in the HIP library)"""
    c = ctypes
    P, ptr, i, u, size, surfaces = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.c_size_t, c.POINTER(DeviceSurface)
    return {
        "fiasco_amd_renderer_surface_size_420": (i, [ptr, u, u, P(u), P(u), P(size)]),
        "fiasco_amd_renderer_render_planes_420": (i, [ptr, ptr, ptr, ptr, u, u, ptr]),
        "fiasco_amd_planes_render_device_420": (i, [ptr, ptr, ptr, u, u, ptr, surfaces, ptr]),
        "fiasco_amd_batch_decode_device_rendered_420": (i, [ptr, ptr, i, i, surfaces, ptr]),
    }


def _yuv420_abi():
    """the same for include/libfiasco_amd_420.h: decoded frames in 4:2:0 as NV12 / NV21 / I420 buffers (the border list and the
    host planes' entry in host code, which every build of the library has; the kernel and the batch entry in the HIP library)"""
    c = ctypes
    P, ptr, i, u, targets = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.POINTER(DeviceTarget420)
    return {
        "fiasco_amd_batch_decode_device_420": (i, [ptr, i, i, targets, ptr]),
        "fiasco_amd_batch_decode_planes_420": (i, [ptr, u, i, ptr]),
        "fiasco_amd_batch_smoothing_borders_420": (i, [ptr, u, i, P(Border), u]),
        "fiasco_amd_planes_to_420_device": (i, [ptr, ptr, ptr, u, u, targets, ptr]),
    }


def _ycbcr_abi():
    """the same for include/libfiasco_amd_ycbcr.h: NV12 / NV21 / I420 / planar 4:4:4 frames into the coder (the host entries
    in host code, which every build of the library has; the kernel and the device entries in the HIP library)"""
    c = ctypes
    P, ptr, i, u, f32, frames = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.c_float, c.POINTER(YCbCrFrame)
    return {
        "fiasco_amd_batch_stage_ycbcr": (ptr, [u, frames, f32, ptr]),
        "fiasco_amd_seq_open_ycbcr": (ptr, [u, frames, f32, ptr, u, u]),
        "fiasco_amd_batch_stage_device_ycbcr": (ptr, [u, frames, ptr, f32, ptr]),
        "fiasco_amd_batch_upload_device_ycbcr": (i, [ptr, frames, ptr]),
        "fiasco_amd_seq_open_device_ycbcr": (ptr, [u, frames, ptr, f32, ptr, u, u]),
    }


def _stream_abi():
    """the same for include/libfiasco_amd_stream.h: .fco streams read back (the reader, the frame order, the rewrite and the
    border list in host code, which every build of the product has; the decode entries in the HIP library)"""
    c = ctypes
    P, ptr, i, u, size = c.POINTER, c.c_void_p, c.c_int, c.c_uint, c.c_size_t
    return {
        "fiasco_amd_stream_open": (ptr, [c.c_char_p, size]),
        "fiasco_amd_stream_open_file": (ptr, [c.c_char_p]),
        "fiasco_amd_stream_free": (None, [ptr]),
        "fiasco_amd_stream_get_info": (i, [ptr, P(StreamInfo)]),
        "fiasco_amd_stream_frame_type": (i, [ptr, u]),
        "fiasco_amd_stream_coding_order": (i, [ptr, P(u), u]),
        "fiasco_amd_stream_rewrite": (i, [ptr, P(ptr), P(size)]),
        "fiasco_amd_stream_smoothing_borders": (i, [ptr, u, i, i, P(Border), u]),
        "fiasco_amd_stream_decode_device": (i, [ptr, u, u, i, i, P(DeviceTarget), ptr]),
        "fiasco_amd_stream_decode_device_420": (i, [ptr, u, u, i, i, P(DeviceTarget420), ptr]),
        "fiasco_amd_stream_decode_planes": (i, [ptr, u, i, ptr]),
        "fiasco_amd_stream_decode_planes_420": (i, [ptr, u, i, ptr]),
    }


_SIGNATURES = _abi()
_STREAM_SIGNATURES = _stream_abi()
# every symbol include/libfiasco_amd_stream.h declares
STREAM_SYMBOLS = list(_STREAM_SIGNATURES)
_VIDEO_SIGNATURES = _video_abi()
_SMOOTH_SIGNATURES = _smooth_abi()
_DISPLAY_SIGNATURES = _display_abi()
_RENDER_SIGNATURES = _render_abi()
_YUV420_SIGNATURES = _yuv420_abi()
_YCBCR_SIGNATURES = _ycbcr_abi()
_RENDER420_SIGNATURES = _render420_abi()
# every symbol include/libfiasco_amd_render_420.h declares
RENDER420_SYMBOLS = list(_RENDER420_SIGNATURES)
# every symbol include/libfiasco_amd_ycbcr.h declares
YCBCR_SYMBOLS = list(_YCBCR_SIGNATURES)
# every symbol include/libfiasco_amd_420.h declares
YUV420_SYMBOLS = list(_YUV420_SIGNATURES)
# every symbol include/libfiasco_amd_render.h declares
RENDER_SYMBOLS = list(_RENDER_SIGNATURES)
# every symbol include/libfiasco_amd_display.h declares
DISPLAY_SYMBOLS = list(_DISPLAY_SIGNATURES)
# every symbol include/libfiasco_amd_smooth.h declares
SMOOTH_SYMBOLS = list(_SMOOTH_SIGNATURES)
# every symbol include/libfiasco_amd_video.h declares
VIDEO_SYMBOLS = list(_VIDEO_SIGNATURES)
# every symbol include/libfiasco_amd.h and include/libfiasco_amd_hip.h declare
EXPORTED_SYMBOLS = list(_SIGNATURES)


def build(verbose=False):
    """Compile libfiasco_amd.so (gcc for the host C, hipcc --offload-arch=gfx950 for the
    device coder).  Works without a GPU (cross compilation)."""
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC], stdout=out)
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("build did not produce %s" % LIB_PATH)


class FiascoError(RuntimeError):
    pass


class Library:
    """ctypes binding of one libfiasco-compatible shared library."""

    def __init__(self, path=LIB_PATH):
        if not os.path.exists(path):
            raise FiascoError("%s is missing: run fiasco_amd.build() (there is no fallback)" % path)
        self.path = path
        self.L = ctypes.CDLL(path)
        for name, (restype, argtypes) in list(_SIGNATURES.items()) + list(_VIDEO_SIGNATURES.items()) + list(_SMOOTH_SIGNATURES.items()) + list(_DISPLAY_SIGNATURES.items()) + list(_RENDER_SIGNATURES.items()) + list(_YUV420_SIGNATURES.items()) + list(_YCBCR_SIGNATURES.items()) + list(_RENDER420_SIGNATURES.items()) + list(_STREAM_SIGNATURES.items()):      # the one place that declares the ABI to ctypes
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
        if not self.L.fiasco_amd_set_limits(max_states, max_level):
            raise FiascoError(self.error_message())

    def get_limits(self):
        a, b = ctypes.c_uint(), ctypes.c_uint()
        self.L.fiasco_amd_get_limits(ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    def set_devices(self, ids):
        """fiasco_amd_set_devices: the devices the batch entries spread their frames over ([] = automatic)."""
        arr = (ctypes.c_int * max(len(ids), 1))(*ids)
        if not self.L.fiasco_amd_set_devices(arr, len(ids)):
            raise FiascoError(self.error_message())

    def device_count(self):
        return self.L.fiasco_amd_device_count()

    def set_device(self, device):
        if not self.L.fiasco_amd_set_device(device):
            raise FiascoError(self.error_message())

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
                                   ctypes.c_float(quality), options.handle if options else None)

    def encode_batch(self, pnm_list, quality=20.0, options=None):
        """fiasco_amd_encode_batch: independent stills (raw PNM bytes) -> list of .fco bytes
        (None for a frame that failed)."""
        n = len(pnm_list)
        bufs = (ctypes.c_char_p * n)(*pnm_list)
        lens = (ctypes.c_size_t * n)(*[len(b) for b in pnm_list])
        return _streams(self.L, n, lambda outs, olen: self.L.fiasco_amd_encode_batch(
            n, bufs, lens, ctypes.c_float(quality), options.handle if options else None, outs, olen))


def _streams(L, n, call):
    """The n streams call(outs, olen) leaves in the two arrays, as bytes (None for a frame that failed); the C side's
    copies are freed."""
    outs = (ctypes.c_void_p * n)()
    olen = (ctypes.c_size_t * n)()
    call(outs, olen)
    res = []
    for i in range(n):
        if outs[i]:
            res.append(ctypes.string_at(outs[i], olen[i]))
            L.fiasco_amd_free(outs[i])
        else:
            res.append(None)
    return res


class Batch:
    """Staged batch (fiasco_amd_batch_stage / _encode / _free): inputs stay resident in HBM
    between encode() calls."""

    def __init__(self, lib, pnm_list, quality=20.0, options=None):
        c = ctypes
        L = lib.L
        self.lib = lib
        self._keep = None
        self.n = len(pnm_list)
        bufs = (c.c_char_p * self.n)(*pnm_list)
        lens = (c.c_size_t * self.n)(*[len(b) for b in pnm_list])
        self.handle = L.fiasco_amd_batch_stage(self.n, bufs, lens, c.c_float(quality),
                                               options.handle if options else None)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._geom = [_pnm_geometry(p) for p in pnm_list]

    @classmethod
    def from_device(cls, lib, frames, quality=20.0, options=None, stream=None):
        """fiasco_amd_batch_stage_device: a batch of frames that already live in device memory.  A frame is a
        torch uint8 tensor on the GPU or any object with __cuda_array_interface__: H x W is gray, H x W x 3
        interleaved R, G, B, 3 x H x W planar; pitch and plane stride come from the strides (a slice of a larger
        tensor is read in place, a stride pattern the C struct cannot express raises FiascoError).  `stream`: the
        hipStream_t (integer) on which the pixels become ready; None = torch's current stream for torch tensors,
        else the default stream.  The objects are kept alive until the next upload or free()."""
        c = ctypes
        self = cls.__new__(cls)
        self.lib = lib
        frames = list(frames)
        self.n = len(frames)
        arr = _device_frames(frames)
        self.handle = lib.L.fiasco_amd_batch_stage_device(self.n, arr, _stream_of(frames, stream), c.c_float(quality),
                                                          options.handle if options else None)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._keep = frames
        self._geom = [(a.width, a.height, 1 if a.layout == FIASCO_AMD_GRAY8 else 3) for a in arr]
        return self

    @classmethod
    def from_ycbcr(cls, lib, frames, quality=20.0, options=None, order="nv12"):
        """fiasco_amd_batch_stage_ycbcr: a batch of frames that are YCbCr already, in host memory (every build of the
        library).  A frame is (y, cb, cr), three 2-D numpy uint8 arrays -- chroma of H/2 x W/2 is 4:2:0 (I420; YV12 with cb
        and cr exchanged), of H x W 4:4:4 --, or (y, cbcr) with cbcr of shape H/2 x W/2 x 2: interleaved pairs, Cb first for
        order="nv12", Cr first for order="nv21".  Pitches come from the strides.  The planes the coder sees are
        (byte - 128) * 16, a 4:2:0 chroma sample replicated over its 2 x 2 pixels; the frames are converted during the call."""
        self = cls.__new__(cls)
        self.lib = lib
        frames = [tuple(f) for f in frames]
        self.n = len(frames)
        self._keep = None
        arr = _ycbcr_frames(frames, order, "__array_interface__")
        if not hasattr(lib.L, "fiasco_amd_batch_stage_ycbcr"):
            raise FiascoError("%s has no fiasco_amd_batch_stage_ycbcr" % lib.path)
        self.handle = lib.L.fiasco_amd_batch_stage_ycbcr(self.n, arr, ctypes.c_float(quality), options.handle if options else None)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._geom = [(a.width, a.height, 3) for a in arr[:self.n]]
        return self

    @classmethod
    def from_device_ycbcr(cls, lib, frames, quality=20.0, options=None, stream=None, order="nv12"):
        """fiasco_amd_batch_stage_device_ycbcr: from_ycbcr with frames that live in device memory -- torch uint8 tensors on
        the GPU or anything with __cuda_array_interface__, for instance what decode_420 filled -- read in place by one
        kernel launch per device share.  `stream` as from_device.  The objects are kept alive until the next upload or
        free()."""
        if not hasattr(lib.L, "fiasco_amd_batch_stage_device_ycbcr"):
            raise FiascoError("%s has no fiasco_amd_batch_stage_device_ycbcr: frames in device memory need the HIP library" % lib.path)
        self = cls.__new__(cls)
        self.lib = lib
        frames = [tuple(f) for f in frames]
        self.n = len(frames)
        arr = _ycbcr_frames(frames, order, "__cuda_array_interface__")
        flat = [a for f in frames for a in f]
        self.handle = lib.L.fiasco_amd_batch_stage_device_ycbcr(self.n, arr, _stream_of(flat, stream), ctypes.c_float(quality),
                                                                options.handle if options else None)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._keep = frames
        self._geom = [(a.width, a.height, 3) for a in arr[:self.n]]
        return self

    def upload_device_ycbcr(self, frames, stream=None, order="nv12"):
        """fiasco_amd_batch_upload_device_ycbcr: upload_device with YCbCr frames (see from_device_ycbcr); may follow and be
        followed by upload() and upload_device()."""
        frames = [tuple(f) for f in frames]
        if len(frames) != self.n:
            raise FiascoError("upload_device_ycbcr: %d frames for a batch of %d" % (len(frames), self.n))
        arr = _ycbcr_frames(frames, order, "__cuda_array_interface__")
        flat = [a for f in frames for a in f]
        if not self.lib.L.fiasco_amd_batch_upload_device_ycbcr(self.handle, arr, _stream_of(flat, stream)):
            raise FiascoError(self.lib.error_message())
        self._keep = frames

    def upload_device(self, frames, stream=None):
        """fiasco_amd_batch_upload_device: new frames for every slot, converted on the device from where they lie
        (see from_device); not waited for, the next submit / collect(resubmit=True) encodes them."""
        frames = list(frames)
        if len(frames) != self.n:
            raise FiascoError("upload_device: %d frames for a batch of %d" % (len(frames), self.n))
        arr = _device_frames(frames)
        if not self.lib.L.fiasco_amd_batch_upload_device(self.handle, arr, _stream_of(frames, stream)):
            raise FiascoError(self.lib.error_message())
        self._keep = frames

    def input_planes(self, i):
        """fiasco_amd_batch_input_planes: the planes the coder sees for frame i, int16 [bands, h, w] (12.4 fixed point)."""
        import numpy
        w, h, bands = self._geom[i]          # replacement frames keep the size and colour model of the batch
        out = numpy.empty((bands, h, w), dtype=numpy.int16)
        if not self.lib.L.fiasco_amd_batch_input_planes(self.handle, i, out.ctypes.data):
            raise FiascoError(self.lib.error_message())
        return out

    def upload(self, pnm_list):
        """fiasco_amd_batch_upload: new frames for every slot (host PNM buffers -> pinned ->
        HBM, not waited for); the next submit / collect(resubmit=True) encodes them."""
        c = ctypes
        assert len(pnm_list) == self.n
        bufs = (c.c_char_p * self.n)(*pnm_list)
        lens = (c.c_size_t * self.n)(*[len(b) for b in pnm_list])
        if not self.lib.L.fiasco_amd_batch_upload(self.handle, bufs, lens):
            raise FiascoError(self.lib.error_message())

    def submit(self):
        """fiasco_amd_batch_submit: start a pass over the resident inputs, do not wait."""
        return self.lib.L.fiasco_amd_batch_submit(self.handle)

    def collect(self, resubmit=False):
        """fiasco_amd_batch_collect: streams of the submitted pass; with resubmit the next pass
        is started before the host writes them (writer of pass i overlaps search of pass i+1)."""
        L = self.lib.L
        return _streams(L, self.n, lambda outs, olen: L.fiasco_amd_batch_collect(self.handle, outs, olen, 1 if resubmit else 0))

    def encode(self):
        L = self.lib.L
        return _streams(L, self.n, lambda outs, olen: L.fiasco_amd_batch_encode(self.handle, outs, olen))

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
        if not self.lib.L.fiasco_amd_batch_decode_plane(self.handle, i, band, buf):
            raise FiascoError(self.lib.error_message())
        return buf.raw

    def decode_planes(self, i, magnify=0):
        """fiasco_amd_batch_decode_planes: the decoded planes of frame i before any smoothing, int16 [bands, h, w]
        (12.4 fixed point).  magnify != 0: fiasco_amd_batch_decode_planes_magnified, the frame at 2^magnify times its
        side length as `dfiasco -m` shows it; h, w are those of magnified_size()."""
        import numpy
        L = self.lib.L
        w, h, bands = self._geom[i]
        if magnify:
            w, h = magnified_size(self.lib, w, h, magnify)
        out = numpy.empty((bands, h, w), dtype=numpy.int16)
        if not (L.fiasco_amd_batch_decode_planes_magnified(self.handle, i, magnify, out.ctypes.data) if magnify
                else L.fiasco_amd_batch_decode_planes(self.handle, i, out.ctypes.data)):
            raise FiascoError(self.lib.error_message())
        return out

    def smoothing_borders(self, i, magnify=0):
        """fiasco_amd_batch_smoothing_borders: the borders the reference's decoder smooths frame i along, as a list of
        (x, y, len, level, pass) sorted by pass -- odd level: rows y - 1 and y, columns x .. x + len - 1; even level:
        columns x - 1 and x, rows y .. y + len - 1.  The borders of one pass share no pixel.
        magnify != 0: fiasco_amd_batch_smoothing_borders_magnified, the borders of the frame as `dfiasco -m magnify`
        shows it, against the size magnified_size() gives.  FiascoError where the size rule refuses the magnification and
        where a state the reference smooths along falls below level 1 (the reference's own result is undefined there)."""
        L = self.lib.L
        if magnify:
            def f(handle, k, out, cap):
                return L.fiasco_amd_batch_smoothing_borders_magnified(handle, k, magnify, out, cap)
        else:
            f = L.fiasco_amd_batch_smoothing_borders
        n = f(self.handle, i, None, 0)
        if not n:
            raise FiascoError(self.lib.error_message())
        arr = (Border * n)()
        if f(self.handle, i, arr, n) != n:
            raise FiascoError(self.lib.error_message())
        return [(b.x, b.y, b.len, b.level, b.pass_) for b in arr]

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
        targets = list(targets)
        if len(targets) != self.n:
            raise FiascoError("decode_device: %d targets for a batch of %d" % (len(targets), self.n))
        arr = _device_targets(targets)
        on = _stream_of([t for t in targets if t is not None], stream)
        if smoothing:
            good = self.lib.L.fiasco_amd_batch_decode_device_smoothed(self.handle, smoothing, arr, on)
        elif magnify:
            good = self.lib.L.fiasco_amd_batch_decode_device_magnified(self.handle, magnify, arr, on)
        else:
            good = self.lib.L.fiasco_amd_batch_decode_device(self.handle, arr, on)
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

    def decode_shown(self, targets, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_batch_decode_device_shown: the frames of the last finished pass as `dfiasco -m magnify -s smoothing
        -o` writes them, into `targets` (as decode_device takes them; every target has the size magnified_size() gives
        for its frame).  The defaults give what plain `dfiasco -m magnify -o` writes: smoothed at the value of each frame's
        own stream header.  smoothing: -1, 0 (none) or 1 .. 100 per cent.  A frame that cannot be smoothed at `magnify`
        (a state of its partition falls below level 1) fails alone: the others are written, the return value counts them
        and lib.error_message() names the frame.  Returns the number of frames written."""
        targets = list(targets)
        if len(targets) != self.n:
            raise FiascoError("decode_shown: %d targets for a batch of %d" % (len(targets), self.n))
        arr = _device_targets(targets)
        good = self.lib.L.fiasco_amd_batch_decode_device_shown(self.handle, magnify, smoothing, arr,
                                                               _stream_of([t for t in targets if t is not None], stream))
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

    def decode_420(self, targets, magnify=0, smoothing=-1, stream=None, order="nv12"):
        """fiasco_amd_batch_decode_device_420: the frames of the last finished pass decoded in 4:2:0, as the reference's
        decoder does with fiasco_d_options_set_4_2_0_format -- the chroma bands come from the automaton at half the side
        length, they are not subsampled -- at `-m magnify -s smoothing`, as 8-bit Y, Cb, Cr into `targets`.  A target is
        (y, cb, cr), three writable 2-D uint8 GPU arrays of H x W, H/2 x W/2 and H/2 x W/2 (I420; the chroma planes share one
        pitch), or (y, cbcr) with cbcr of shape H/2 x W/2 x 2: interleaved pairs, Cb first for order="nv12", Cr first for
        order="nv21"; W x H is magnified_size() of the frame; None skips the frame.  Flights, smoothing, per-frame refusals
        and `stream` as decode_shown; a gray frame and a frame whose chroma the reference leaves zero fail alone.  Returns
        the number of frames written."""
        targets = list(targets)
        if len(targets) != self.n:
            raise FiascoError("decode_420: %d targets for a batch of %d" % (len(targets), self.n))
        arr = _device_targets_420(targets, order)
        flat = [a for t in targets if t is not None for a in t]
        good = self.lib.L.fiasco_amd_batch_decode_device_420(self.handle, magnify, smoothing, arr, _stream_of(flat, stream))
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

    def decode_planes_420(self, i, magnify=0):
        """fiasco_amd_batch_decode_planes_420: the unsmoothed planes of frame i decoded in 4:2:0 at `magnify`, three int16
        arrays (12.4 fixed point): Y [h, w], Cb and Cr [h / 2, w / 2]; h, w are those of magnified_size()."""
        import numpy
        w, h, _ = self._geom[i]
        if magnify:
            w, h = magnified_size(self.lib, w, h, magnify)
        out = numpy.empty(w * h + 2 * (w // 2) * (h // 2), dtype=numpy.int16)
        if not self.lib.L.fiasco_amd_batch_decode_planes_420(self.handle, i, magnify, out.ctypes.data):
            raise FiascoError(self.lib.error_message())
        c = (w // 2) * (h // 2)
        return (out[:w * h].reshape(h, w), out[w * h:w * h + c].reshape(h // 2, w // 2), out[w * h + c:].reshape(h // 2, w // 2))

    def smoothing_borders_420(self, i, magnify=0):
        """fiasco_amd_batch_smoothing_borders_420: the borders the reference smooths the Y plane of frame i along when it
        decodes in 4:2:0, (x, y, len, level, pass) as smoothing_borders() lists them: the Y passes at shift `magnify`, then
        the Cb passes at shift `magnify` - 1, against the size magnified_size() gives."""
        L = self.lib.L
        n = L.fiasco_amd_batch_smoothing_borders_420(self.handle, i, magnify, None, 0)
        if not n:
            raise FiascoError(self.lib.error_message())
        arr = (Border * n)()
        if L.fiasco_amd_batch_smoothing_borders_420(self.handle, i, magnify, arr, n) != n:
            raise FiascoError(self.lib.error_message())
        return [(b.x, b.y, b.len, b.level, b.pass_) for b in arr]

    def decode_rendered(self, renderer, surfaces, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_batch_decode_device_rendered: the frames of the last finished pass as the reference's viewer puts them
        on the screen at `-m magnify -s smoothing`, through `renderer` into `surfaces` -- one per frame, a writable uint8 GPU
        array of shape (H, W, bpp // 8) with H, W from renderer.surface_size() for the frame at magnified_size(); the pitch is
        the first stride; None skips the frame.  Flights, smoothing, per-frame refusals and `stream` as decode_shown.
        Returns the number of frames written."""
        surfaces = list(surfaces)
        if len(surfaces) != self.n:
            raise FiascoError("decode_rendered: %d surfaces for a batch of %d" % (len(surfaces), self.n))
        arr = _device_surfaces(surfaces, renderer.bpp)
        good = self.lib.L.fiasco_amd_batch_decode_device_rendered(self.handle, renderer.handle, magnify, smoothing, arr,
                                                                  _stream_of([t for t in surfaces if t is not None], stream))
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

    def decode_rendered_420(self, renderer, surfaces, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_batch_decode_device_rendered_420: the frames of the last finished pass as the reference's viewer shows
        them on a screen -- decoded in 4:2:0 as decode_420 decodes them, at `-m magnify -s smoothing`, and rendered through
        `renderer` with every chroma sample standing for its 2 x 2 pixels -- into `surfaces`, one per frame as
        decode_rendered takes them, of the size renderer.surface_size_420() gives for the frame at magnified_size(); None
        skips the frame.  A gray frame and a frame whose chroma the reference leaves zero fail alone.  Returns the number
        of frames written."""
        surfaces = list(surfaces)
        if len(surfaces) != self.n:
            raise FiascoError("decode_rendered_420: %d surfaces for a batch of %d" % (len(surfaces), self.n))
        arr = _device_surfaces(surfaces, renderer.bpp)
        good = self.lib.L.fiasco_amd_batch_decode_device_rendered_420(self.handle, renderer.handle, magnify, smoothing, arr,
                                                                      _stream_of([t for t in surfaces if t is not None], stream))
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

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
        if len(thumbs) != self.n:
            raise FiascoError("decode_thumbnails: %d thumbs for a batch of %d" % (len(thumbs), self.n))
        arr = None
        if targets is not None:
            targets = list(targets)
            if len(targets) != self.n:
                raise FiascoError("decode_thumbnails: %d targets for a batch of %d" % (len(targets), self.n))
            arr = _device_targets(targets)
        tarr = _device_targets(thumbs)
        on = _stream_of([t for t in (targets or []) + thumbs if t is not None], stream)
        if smoothing:
            good = self.lib.L.fiasco_amd_batch_decode_device_thumbnails_shown(self.handle, smoothing, arr, reduce, tarr, on)
        else:
            good = self.lib.L.fiasco_amd_batch_decode_device_thumbnails(self.handle, arr, reduce, tarr, on)
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

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
        n = self.n
        arr = None
        if targets is not None:
            targets = list(targets)
            if len(targets) != n:
                raise FiascoError("decode_distortion_device: %d targets for a batch of %d" % (len(targets), n))
            arr = _device_targets(targets)
        s, m = (c.c_ulonglong * (3 * n))(), (c.c_uint * (3 * n))()
        on = _stream_of([t for t in targets or [] if t is not None], stream)
        if smoothing:
            good = self.lib.L.fiasco_amd_batch_decode_distortion_device_smoothed(self.handle, smoothing, s, m, arr, on)
        else:
            good = self.lib.L.fiasco_amd_batch_decode_distortion_device(self.handle, s, m, arr, on)
        if not good:
            raise FiascoError(self.lib.error_message())
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
        if not self.lib.L.fiasco_amd_batch_decode_psnr(self.handle, i, ps, ms):
            raise FiascoError(self.lib.error_message())
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


def _describe(what, i, fr, d):
    """One GPU array (a torch tensor, anything with __cuda_array_interface__) into the DeviceFrame / DeviceTarget d:
    layout from the shape, pitch and plane stride from the strides.  Returns the interface's read-only flag."""
    cai = getattr(fr, "__cuda_array_interface__", None)
    if cai is None:
        raise FiascoError("%s %d is not in device memory (no __cuda_array_interface__)" % (what, i))
    if cai["typestr"] not in ("|u1", "<u1", ">u1", "=u1"):
        raise FiascoError("%s %d: 8-bit unsigned pixels expected, not %s" % (what, i, cai["typestr"]))
    shape = tuple(int(v) for v in cai["shape"])
    strides = cai.get("strides")
    if strides is None:
        strides = tuple(_packed_strides(shape))
    strides = tuple(int(v) for v in strides)
    d.data = int(cai["data"][0])
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
    return bool(cai["data"][1])


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


def _plane_of(what, i, a, ndim):
    """(address, shape, strides) of one writable uint8 GPU array of `ndim` dimensions whose innermost elements are adjacent"""
    cai = getattr(a, "__cuda_array_interface__", None)
    if cai is None:
        raise FiascoError("target %d: the %s is not in device memory (no __cuda_array_interface__)" % (i, what))
    if cai["typestr"] not in ("|u1", "<u1", ">u1", "=u1"):
        raise FiascoError("target %d: the %s holds %s, not bytes (uint8)" % (i, what, cai["typestr"]))
    shape = tuple(int(v) for v in cai["shape"])
    if len(shape) != ndim:
        raise FiascoError("target %d: the %s has shape %s, %d dimensions expected" % (i, what, shape, ndim))
    strides = cai.get("strides")
    strides = tuple(int(v) for v in (strides if strides is not None else _packed_strides(shape)))
    if strides[-1] != 1 or (ndim == 3 and strides[1] != 2) or strides[0] <= 0:
        raise FiascoError("target %d: the strides %s of the %s cannot be described by a pitch" % (i, strides, what))
    if cai["data"][1]:
        raise FiascoError("target %d: the %s is read-only" % (i, what))
    return int(cai["data"][0]), shape, strides


def _device_targets_420(targets, order="nv12"):
    """The fiasco_amd_device_target_420 array of a list of 4:2:0 targets: (y, cb, cr), three 2-D arrays, or (y, cbcr) with
    cbcr of shape H/2 x W/2 x 2 and `order` "nv12" (Cb first) or "nv21"; None: y = NULL, skipped."""
    if order not in ("nv12", "nv21"):
        raise FiascoError("order %r is neither \"nv12\" nor \"nv21\"" % (order,))
    arr = (DeviceTarget420 * max(len(targets), 1))()
    for i, t in enumerate(targets):
        if t is None:
            continue
        t = tuple(t)
        if len(t) not in (2, 3):
            raise FiascoError("target %d: (y, cb, cr) or (y, cbcr) expected, not %d arrays" % (i, len(t)))
        d = arr[i]
        y, (h, w), ys = _plane_of("Y plane", i, t[0], 2)
        d.y, d.y_pitch, d.width, d.height = y, ys[0], w, h
        if len(t) == 3:
            (cb, sb, stb), (cr, sr, str_) = _plane_of("Cb plane", i, t[1], 2), _plane_of("Cr plane", i, t[2], 2)
            if sb != (h // 2, w // 2) or sr != sb:
                raise FiascoError("target %d: chroma planes of %s and %s for a Y plane of %d x %d (%d x %d expected)"
                                  % (i, sb[::-1], sr[::-1], w, h, w // 2, h // 2))
            if stb[0] != str_[0]:
                raise FiascoError("target %d: the chroma planes have pitches %d and %d (one pitch expected)" % (i, stb[0], str_[0]))
            d.cb, d.cr, d.c_pitch, d.c_step = cb, cr, stb[0], 1
        else:
            c, sc, stc = _plane_of("chroma plane", i, t[1], 3)
            if sc != (h // 2, w // 2, 2):
                raise FiascoError("target %d: an interleaved chroma plane of shape %s for a Y plane of %d x %d (%d x %d x 2 expected)"
                                  % (i, sc, w, h, h // 2, w // 2))
            d.cb, d.cr = (c, c + 1) if order == "nv12" else (c + 1, c)
            d.c_pitch, d.c_step = stc[0], 2
    return arr


def _byte_plane(i, what, a, ndim, iface):
    """(address, shape, strides) of one uint8 array of `ndim` dimensions whose innermost elements are adjacent, read through
    `iface` (__array_interface__: host memory, __cuda_array_interface__: device memory)"""
    d = getattr(a, iface, None)
    if d is None:
        raise FiascoError("frame %d: the %s is not in %s memory (no %s)"
                          % (i, what, "device" if "cuda" in iface else "host", iface))
    if d["typestr"] not in ("|u1", "<u1", ">u1", "=u1"):
        raise FiascoError("frame %d: the %s holds %s, not bytes (uint8)" % (i, what, d["typestr"]))
    shape = tuple(int(v) for v in d["shape"])
    if len(shape) != ndim:
        raise FiascoError("frame %d: the %s has shape %s, %d dimensions expected" % (i, what, shape, ndim))
    strides = d.get("strides")
    strides = tuple(int(v) for v in (strides if strides is not None else _packed_strides(shape)))
    if strides[-1] != 1 or (ndim == 3 and strides[1] != 2) or strides[0] <= 0:
        raise FiascoError("frame %d: the strides %s of the %s cannot be described by a pitch" % (i, strides, what))
    return int(d["data"][0]), shape, strides


def _ycbcr_frames(frames, order, iface):
    """The fiasco_amd_ycbcr_frame array of a list of frames: (y, cb, cr), three 2-D arrays, or (y, cbcr) with cbcr of shape
    H/2 x W/2 x 2 and `order` "nv12" (Cb first) or "nv21" -- what _device_targets_420 accepts; `order` may also be a list, one
    entry per frame.  The subsampling is inferred
    from the chroma shape: full size is 4:4:4, half size 4:2:0, anything else raises."""
    orders = [order] * len(frames) if isinstance(order, str) else list(order)
    if len(orders) != len(frames):
        raise FiascoError("%d orders for %d frames" % (len(orders), len(frames)))
    arr = (YCbCrFrame * max(len(frames), 1))()
    for i, t in enumerate(frames):
        order = orders[i]
        if order not in ("nv12", "nv21"):
            raise FiascoError("order %r is neither \"nv12\" nor \"nv21\"" % (order,))
        if len(t) not in (2, 3):
            raise FiascoError("frame %d: (y, cb, cr) or (y, cbcr) expected, not %d arrays" % (i, len(t)))
        d = arr[i]
        y, (h, w), ys = _byte_plane(i, "Y plane", t[0], 2, iface)
        d.y, d.y_pitch, d.width, d.height = y, ys[0], w, h
        if len(t) == 3:
            (cb, sb, stb), (cr, sr, str_) = _byte_plane(i, "Cb plane", t[1], 2, iface), _byte_plane(i, "Cr plane", t[2], 2, iface)
            if sr != sb or sb not in ((h, w), (h // 2, w // 2)):
                raise FiascoError("frame %d: chroma planes of %s and %s for a Y plane of %d x %d (%d x %d for 4:4:4 or %d x %d for 4:2:0 expected)"
                                  % (i, sb[::-1], sr[::-1], w, h, w, h, w // 2, h // 2))
            if stb[0] != str_[0]:
                raise FiascoError("frame %d: the chroma planes have pitches %d and %d (one pitch expected)" % (i, stb[0], str_[0]))
            d.cb, d.cr, d.c_pitch, d.c_step, d.subsampling = cb, cr, stb[0], 1, 0 if sb == (h, w) else 1
        else:
            c, sc, stc = _byte_plane(i, "chroma plane", t[1], 3, iface)
            if sc != (h // 2, w // 2, 2):
                raise FiascoError("frame %d: an interleaved chroma plane of shape %s for a Y plane of %d x %d (%d x %d x 2 expected)"
                                  % (i, sc, w, h, h // 2, w // 2))
            d.cb, d.cr = (c, c + 1) if order == "nv12" else (c + 1, c)
            d.c_pitch, d.c_step, d.subsampling = stc[0], 2, 1
    return arr


def _device_surfaces(surfaces, bpp):
    """The fiasco_amd_device_surface array of a list of writable uint8 GPU arrays of shape (H, W, bpp // 8); the pitch is the
    first stride, the other two must be bpp // 8 and 1; None: data = NULL, skipped."""
    arr = (DeviceSurface * max(len(surfaces), 1))()
    for i, t in enumerate(surfaces):
        if t is None:
            continue
        cai = getattr(t, "__cuda_array_interface__", None)
        if cai is None:
            raise FiascoError("surface %d is not in device memory (no __cuda_array_interface__)" % i)
        if cai["typestr"] not in ("|u1", "<u1", ">u1", "=u1"):
            raise FiascoError("surface %d: bytes (uint8) expected, not %s" % (i, cai["typestr"]))
        shape = tuple(int(v) for v in cai["shape"])
        if len(shape) != 3 or shape[2] != bpp // 8:
            raise FiascoError("surface %d: shape %s is not H x W x %d (the bytes of a pixel at %d bpp)" % (i, shape, bpp // 8, bpp))
        strides = cai.get("strides")
        strides = tuple(int(v) for v in (strides if strides is not None else _packed_strides(shape)))
        if strides[2] != 1 or strides[1] != bpp // 8 or strides[0] <= 0:
            raise FiascoError("surface %d: strides %s cannot be described by a pitch (the bytes of a pixel and the pixels of a row "
                              "must be adjacent)" % (i, strides))
        if cai["data"][1]:
            raise FiascoError("surface %d is read-only" % i)
        arr[i].data, arr[i].pitch, (arr[i].height, arr[i].width) = int(cai["data"][0]), strides[0], shape[:2]
    return arr


class Renderer:
    """fiasco_amd_renderer_*: the reference's renderer (fiasco_renderer_new) restated -- colour masks, 16, 24 or 32 bits per
    pixel, optionally every pixel doubled in both directions.  Immutable; delete() frees it."""

    def __init__(self, lib, red_mask, green_mask, blue_mask, bpp, double_resolution=False):
        self.lib, self.bpp, self.double_resolution = lib, bpp, bool(double_resolution)
        self.handle = lib.L.fiasco_amd_renderer_new(red_mask, green_mask, blue_mask, bpp, 1 if double_resolution else 0)
        if not self.handle:
            raise FiascoError(lib.error_message())

    def surface_size(self, width, height, color):
        """fiasco_amd_renderer_surface_size: (surface width, surface height, bytes of a packed row) for a frame of
        width x height; FiascoError where the reference's loops would not fill the surface."""
        w, h, row = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_size_t()
        if not self.lib.L.fiasco_amd_renderer_surface_size(self.handle, width, height, 1 if color else 0, w, h, row):
            raise FiascoError(self.lib.error_message())
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
        if not self.lib.L.fiasco_amd_renderer_render_planes(self.handle, planes.ctypes.data, 1 if color else 0, w, h, buf):
            raise FiascoError(self.lib.error_message())
        return buf.raw

    def surface_size_420(self, width, height):
        """fiasco_amd_renderer_surface_size_420: (surface width, surface height, bytes of a packed row) for a 4:2:0 frame of
        width x height; FiascoError for an odd side, and at 24 bpp not doubled for a width that is no multiple of 4."""
        w, h, row = ctypes.c_uint(), ctypes.c_uint(), ctypes.c_size_t()
        if not self.lib.L.fiasco_amd_renderer_surface_size_420(self.handle, width, height, w, h, row):
            raise FiascoError(self.lib.error_message())
        return w.value, h.value, row.value

    def render_planes_420(self, y, cb, cr):
        """fiasco_amd_renderer_render_planes_420, the host loop: int16 numpy planes (12.4 fixed point) Y of H x W, Cb and Cr
        of H/2 x W/2 -> the bytes of the packed surface."""
        import numpy
        y, cb, cr = (numpy.ascontiguousarray(p, dtype=numpy.int16) for p in (y, cb, cr))
        if y.ndim != 2 or cb.shape != (y.shape[0] // 2, y.shape[1] // 2) or cr.shape != cb.shape:
            raise FiascoError("render_planes_420: int16 planes of H x W, H/2 x W/2 and H/2 x W/2 expected, not %s, %s, %s" % (y.shape, cb.shape, cr.shape))
        h, w = y.shape
        _, sh, row = self.surface_size_420(w, h)
        buf = ctypes.create_string_buffer(sh * row)
        if not self.lib.L.fiasco_amd_renderer_render_planes_420(self.handle, y.ctypes.data, cb.ctypes.data, cr.ctypes.data, w, h, buf):
            raise FiascoError(self.lib.error_message())
        return buf.raw

    def delete(self):
        if self.handle:
            self.lib.L.fiasco_amd_renderer_delete(self.handle)
            self.handle = None


def render_planes_device_420(lib, renderer, y, cb, cr, surface, stream=None):
    """fiasco_amd_planes_render_device_420: the 4:2:0 rendering kernel alone.  `y`, `cb`, `cr`: packed int16 arrays on the GPU
    (12.4 fixed point) of H x W, H/2 x W/2 and H/2 x W/2; `surface`: as Batch.decode_rendered_420.  Runs on `stream`
    (default as decode_device) and waits for it."""
    planes = [_packed_planes(n, p) for n, p in (("y", y), ("cb", cb), ("cr", cr))]
    if any(len(shape) != 2 for _, shape in planes):
        raise FiascoError("render_planes_device_420: three int16 arrays of two dimensions expected")
    (h, w), sb, sr = planes[0][1], planes[1][1], planes[2][1]
    if sb != (h // 2, w // 2) or sr != sb:
        raise FiascoError("render_planes_device_420: chroma planes of %s and %s for a Y plane of %d x %d" % (sb[::-1], sr[::-1], w, h))
    arr = _device_surfaces([surface], renderer.bpp)
    if surface is None:
        raise FiascoError("render_planes_device_420: no surface")
    if not lib.L.fiasco_amd_planes_render_device_420(planes[0][0], planes[1][0], planes[2][0], w, h, renderer.handle, arr,
                                                     _stream_of([surface], stream)):
        raise FiascoError(lib.error_message())


def render_planes_device(lib, renderer, planes, surface, stream=None):
    """fiasco_amd_planes_render_device: the rendering kernel alone.  `planes`: a packed int16 array on the GPU (12.4 fixed
    point), H x W or 3 x H x W; `surface`: as Batch.decode_rendered.  Runs on `stream` (default as decode_device) and waits
    for it."""
    address, shape = _packed_planes(None, planes)
    arr = _device_surfaces([surface], renderer.bpp)
    if surface is None:
        raise FiascoError("render_planes_device: no surface")
    if not lib.L.fiasco_amd_planes_render_device(address, 1 if len(shape) == 3 else 0, shape[-1], shape[-2], renderer.handle, arr,
                                                 _stream_of([surface], stream)):
        raise FiascoError(lib.error_message())


def magnified_size(lib, width, height, magnify):
    """fiasco_amd_magnified_size: (width, height) at which `dfiasco -m magnify` shows a frame of width x height --
    << magnify, or >> -magnify rounded up to even.  FiascoError with the reference's limit ("Maximum value is N." /
    "Minimum value is -N.") where the reference refuses.  A pure function; no device needed."""
    w, h = ctypes.c_uint(), ctypes.c_uint()
    if not lib.L.fiasco_amd_magnified_size(width, height, magnify, w, h):
        raise FiascoError(lib.error_message())
    return w.value, h.value


def planes_to_pixels_device(lib, planes, target, stream=None):
    """fiasco_amd_planes_to_pixels_device: the decoder's last step alone.  `planes`: a packed int16 array on the GPU
    (12.4 fixed point), H x W for gray or 3 x H x W for Y, Cb, Cr; `target`: as Batch.decode_device.  The conversion
    runs on `stream` (default as decode_device)."""
    address, shape = _packed_planes(None, planes)
    arr = _device_targets([target])
    if (arr[0].height, arr[0].width) != shape[-2:]:
        raise FiascoError("target of %d x %d pixels for planes of %d x %d" % (arr[0].width, arr[0].height, shape[-1], shape[-2]))
    if not lib.L.fiasco_amd_planes_to_pixels_device(address, 1 if len(shape) == 3 else 0, arr, _stream_of([target], stream)):
        raise FiascoError(lib.error_message())


def planes_to_420_device(lib, y, cb, cr, target, stream=None, order="nv12"):
    """fiasco_amd_planes_to_420_device: the 4:2:0 conversion kernel alone.  `y`, `cb`, `cr`: packed int16 arrays on the GPU
    (12.4 fixed point) of H x W, H/2 x W/2 and H/2 x W/2; `target` and `order` as Batch.decode_420.  Runs on `stream`
    (default as decode_device) and waits for it."""
    planes = [_packed_planes(n, p) for n, p in (("y", y), ("cb", cb), ("cr", cr))]
    if any(len(shape) != 2 for _, shape in planes):
        raise FiascoError("planes_to_420_device: three int16 arrays of two dimensions expected")
    (h, w), sb, sr = planes[0][1], planes[1][1], planes[2][1]
    if sb != (h // 2, w // 2) or sr != sb:
        raise FiascoError("planes_to_420_device: chroma planes of %s and %s for a Y plane of %d x %d" % (sb[::-1], sr[::-1], w, h))
    if target is None:
        raise FiascoError("planes_to_420_device: no target")
    arr = _device_targets_420([target], order)
    if not lib.L.fiasco_amd_planes_to_420_device(planes[0][0], planes[1][0], planes[2][0], w, h, arr, _stream_of(list(target), stream)):
        raise FiascoError(lib.error_message())


def _packed_planes(name, p):
    """(address, shape) of packed int16 planes on the GPU, H x W or 3 x H x W; `name' tells the planes of a call apart in
    the refusals (None: it has one set)."""
    what = "planes" if name is None else "planes `%s'" % name
    cai = getattr(p, "__cuda_array_interface__", None)
    if cai is None:
        raise FiascoError("the %s are not in device memory (no __cuda_array_interface__)" % what)
    shape = tuple(int(v) for v in cai["shape"])
    if cai["typestr"] not in ("<i2", "=i2") or len(shape) not in (2, 3) or (len(shape) == 3 and shape[0] != 3):
        raise FiascoError("%s: int16 H x W or 3 x H x W expected, not %s %s" % (what, cai["typestr"], shape))
    if cai.get("strides") is not None and tuple(int(v) for v in cai["strides"]) != tuple(2 * v for v in _packed_strides(shape)):
        raise FiascoError("%s: strides %s are not those of a packed array" % (what, tuple(cai["strides"])))
    return int(cai["data"][0]), shape


def planes_distortion_device(lib, a, b, stream=None):
    """fiasco_amd_planes_distortion_device: the measuring kernel alone.  `a`, `b`: two packed int16 arrays of one shape
    on the GPU (12.4 fixed point; torch tensors or anything with __cuda_array_interface__), H x W or 3 x H x W.  Returns
    (sse, maxdiff), three integers each (0 for bands the planes do not have).  Runs on `stream` (default as
    decode_device) and waits for the result."""
    (pa, shape), (pb, shape_b) = _packed_planes("a", a), _packed_planes("b", b)
    if shape != shape_b:
        raise FiascoError("planes of %s against planes of %s" % (shape, shape_b))
    s, m = (ctypes.c_ulonglong * 3)(), (ctypes.c_uint * 3)()
    if not lib.L.fiasco_amd_planes_distortion_device(pa, pb, 3 if len(shape) == 3 else 1, shape[-1], shape[-2], s, m,
                                                     _stream_of([a], stream)):
        raise FiascoError(lib.error_message())
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
    if not f(address, shape[-1], shape[-2], arr, len(borders), smoothing, _stream_of([planes], stream)):
        raise FiascoError(lib.error_message())


def _packed_strides(shape):
    out, n = [], 1
    for v in reversed(shape):
        out.append(n)
        n *= v
    return reversed(out)


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


class Sequence:
    """fiasco_amd_seq_*: one video, this process searching and writing every world-th group of
    pictures (include/libfiasco_amd.h).  Frames: raw PNM bytes in display order."""

    def __init__(self, lib, pnm_list, quality=20.0, options=None, rank=0, world=1):
        c = ctypes
        L = self.L = lib.L
        self.lib = lib
        self._keep = (list(pnm_list), options)                      # borrowed by the C side
        n = len(pnm_list)
        self._bufs = (c.c_char_p * n)(*pnm_list)
        self._lens = (c.c_size_t * n)(*[len(b) for b in pnm_list])
        self.handle = L.fiasco_amd_seq_open(n, self._bufs, self._lens, c.c_float(quality),
                                            options.handle if options else None, rank, world)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._geom = _pnm_geometry(pnm_list[0])
        self._opened(n, rank, world)

    def _opened(self, n, rank, world):
        L = self.L
        self.n = n                                                  # frames in display order
        self.rank, self.world = rank, world
        self.gops = L.fiasco_amd_seq_gops(self.handle)
        self.frames = L.fiasco_amd_seq_frames(self.handle)
        self.ycol_size = L.fiasco_amd_seq_ycol_size(self.handle)
        self.initial_level = L.fiasco_amd_seq_initial_level(self.handle)
        self._outputs = None                                        # what set_outputs lent to the C side

    @classmethod
    def from_device(cls, lib, frames, quality=20.0, options=None, rank=0, world=1, stream=None):
        """fiasco_amd_seq_open_device: a video whose frames already live in device memory, in display order; frames
        as Batch.from_device takes them (torch uint8 tensors or anything with __cuda_array_interface__; pitch and
        plane stride come from the strides).  Open converts the frames this rank searches and waits for that: the
        sources may be overwritten right after the call.  The objects are kept alive until free()."""
        if not hasattr(lib.L, "fiasco_amd_seq_open_device"):
            raise FiascoError("%s has no fiasco_amd_seq_open_device: videos in device memory need the HIP library" % lib.path)
        self = cls.__new__(cls)
        self.L, self.lib = lib.L, lib
        frames = list(frames)
        arr = _device_frames(frames)
        self._keep = (frames, options)
        self.handle = lib.L.fiasco_amd_seq_open_device(len(frames), arr, _stream_of(frames, stream), ctypes.c_float(quality),
                                                       options.handle if options else None, rank, world)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._geom = (arr[0].width, arr[0].height, 1 if arr[0].layout == FIASCO_AMD_GRAY8 else 3)
        self._opened(len(frames), rank, world)
        return self

    @classmethod
    def from_ycbcr(cls, lib, frames, quality=20.0, options=None, rank=0, world=1, order="nv12"):
        """fiasco_amd_seq_open_ycbcr: a video of frames that are YCbCr already, in host memory and display order; frames as
        Batch.from_ycbcr takes them.  The frames are converted during the call."""
        if not hasattr(lib.L, "fiasco_amd_seq_open_ycbcr"):
            raise FiascoError("%s has no fiasco_amd_seq_open_ycbcr" % lib.path)
        self = cls.__new__(cls)
        self.L, self.lib = lib.L, lib
        frames = [tuple(f) for f in frames]
        arr = _ycbcr_frames(frames, order, "__array_interface__")
        self._keep = (None, options)
        self.handle = lib.L.fiasco_amd_seq_open_ycbcr(len(frames), arr, ctypes.c_float(quality), options.handle if options else None,
                                                      rank, world)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._geom = (arr[0].width, arr[0].height, 3)
        self._opened(len(frames), rank, world)
        return self

    @classmethod
    def from_device_ycbcr(cls, lib, frames, quality=20.0, options=None, rank=0, world=1, stream=None, order="nv12"):
        """fiasco_amd_seq_open_device_ycbcr: from_device with frames that are YCbCr already, as Batch.from_device_ycbcr takes
        them.  Open converts the frames this rank searches and waits for that."""
        if not hasattr(lib.L, "fiasco_amd_seq_open_device_ycbcr"):
            raise FiascoError("%s has no fiasco_amd_seq_open_device_ycbcr: videos in device memory need the HIP library" % lib.path)
        self = cls.__new__(cls)
        self.L, self.lib = lib.L, lib
        frames = [tuple(f) for f in frames]
        arr = _ycbcr_frames(frames, order, "__cuda_array_interface__")
        self._keep = (frames, options)
        flat = [a for f in frames for a in f]
        self.handle = lib.L.fiasco_amd_seq_open_device_ycbcr(len(frames), arr, _stream_of(flat, stream), ctypes.c_float(quality),
                                                             options.handle if options else None, rank, world)
        if not self.handle:
            raise FiascoError(lib.error_message())
        self._geom = (arr[0].width, arr[0].height, 3)
        self._opened(len(frames), rank, world)
        return self

    def set_outputs(self, targets=None, distortion=False, stream=None):
        """fiasco_amd_seq_set_outputs_device: from now on every search reconstructs every frame of the GOPs it searches
        and delivers it on the device.  targets: one writable GPU array per display frame as Batch.decode_device takes
        them (None entries: not this frame), or None; distortion: measure every frame against its original
        (distortion() hands the sums out).  Neither: no outputs again.  The arrays live in this object."""
        import numpy
        if not hasattr(self.L, "fiasco_amd_seq_set_outputs_device"):
            raise FiascoError("%s has no fiasco_amd_seq_set_outputs_device: device outputs need the HIP library" % self.lib.path)
        if targets is None and not distortion:
            if not self.L.fiasco_amd_seq_set_outputs_device(self.handle, None):
                raise FiascoError(self.lib.error_message())
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
        st = _stream_of([t for t in (targets or []) if t is not None], stream)
        o.stream = st.value if st is not None else None
        if not self.L.fiasco_amd_seq_set_outputs_device(self.handle, c.byref(o)):
            raise FiascoError(self.lib.error_message())        # nothing was set: what was lent before stays lent
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
        c = ctypes
        out, n = c.c_void_p(), c.c_size_t()
        if not self.L.fiasco_amd_seq_encode(self.handle, out, n):
            raise FiascoError(self.lib.error_message())
        data = c.string_at(out, n.value)
        self.L.fiasco_amd_free(out)
        return data

    def keep_reconstructed(self, keep=True):
        """fiasco_amd_seq_keep_reconstructed: the searches keep the coder's reconstruction of every frame on the host."""
        if not self.L.fiasco_amd_seq_keep_reconstructed(self.handle, 1 if keep else 0):
            raise FiascoError(self.lib.error_message())

    def reconstructed_planes(self, display):
        """fiasco_amd_seq_reconstructed_planes: (int16 [bands, h, w] 12.4 fixed point, frame type 0 I / 1 P / 2 B)."""
        import numpy
        w, h, bands = self._geom
        out = numpy.empty((bands, h, w), dtype=numpy.int16)
        t = ctypes.c_int(-1)
        if not self.L.fiasco_amd_seq_reconstructed_planes(self.handle, display, out.ctypes.data, t):
            raise FiascoError(self.lib.error_message())
        return out, t.value

    def gop_of(self, frame):
        return self.L.fiasco_amd_seq_gop_of(self.handle, frame)

    def probe(self):
        """Level to speculate for the GOPs behind the first: what frame 0 alone leaves."""
        lv = ctypes.c_uint()
        if not self.L.fiasco_amd_seq_probe(self.handle, lv):
            raise FiascoError(self.lib.error_message())
        return lv.value

    def search(self, carry_in, todo):
        c = ctypes
        ci = (c.c_uint * self.gops)(*carry_in)
        td = (c.c_ubyte * self.gops)(*[1 if t else 0 for t in todo])
        if not self.L.fiasco_amd_seq_search(self.handle, ci, td):
            raise FiascoError(self.lib.error_message())

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
        c = ctypes
        out, n = c.c_void_p(), c.c_size_t()
        if not self.L.fiasco_amd_seq_write(self.handle, frame, ycol, out, n):
            raise FiascoError(self.lib.error_message())
        data = c.string_at(out, n.value)
        self.L.fiasco_amd_free(out)
        return data

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
        if not self.handle:
            raise FiascoError(lib.error_message())
        raw = StreamInfo()
        if not lib.L.fiasco_amd_stream_get_info(self.handle, ctypes.byref(raw)):
            raise FiascoError(lib.error_message())
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
        out, n = ctypes.c_void_p(), ctypes.c_size_t()
        if not self.lib.L.fiasco_amd_stream_rewrite(self.handle, ctypes.byref(out), ctypes.byref(n)):
            raise FiascoError(self.lib.error_message())
        try:
            return ctypes.string_at(out.value, n.value)
        finally:
            self.lib.L.fiasco_amd_free(out)

    def smoothing_borders(self, display, magnify=0, format_420=False):
        """fiasco_amd_stream_smoothing_borders: the borders `dfiasco -m magnify` smooths display frame `display` along,
        (x, y, len, level, pass) as Batch.smoothing_borders() lists them; format_420: as Batch.smoothing_borders_420()."""
        L = self.lib.L
        n = L.fiasco_amd_stream_smoothing_borders(self.handle, display, magnify, int(bool(format_420)), None, 0)
        if not n:
            raise FiascoError(self.lib.error_message())
        arr = (Border * n)()
        if L.fiasco_amd_stream_smoothing_borders(self.handle, display, magnify, int(bool(format_420)), arr, n) != n:
            raise FiascoError(self.lib.error_message())
        return [(b.x, b.y, b.len, b.level, b.pass_) for b in arr]

    def decode_device(self, targets, first=0, magnify=0, smoothing=-1, stream=None):
        """fiasco_amd_stream_decode_device: display frames first .. first + len(targets) - 1 as `dfiasco -m magnify -s
        smoothing -o` writes them, P and B frames included, into `targets` (as Batch.decode_shown takes them; None: not
        this frame).  Returns the number of frames written; a frame that fails takes the frames predicted from it along
        and lib.error_message() names the first and the cause."""
        targets = list(targets)
        arr = _device_targets(targets)
        good = self.lib.L.fiasco_amd_stream_decode_device(self.handle, first, len(targets), magnify, smoothing, arr,
                                                          _stream_of([t for t in targets if t is not None], stream))
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

    def decode_420(self, targets, first=0, magnify=0, smoothing=-1, stream=None, order="nv12"):
        """fiasco_amd_stream_decode_device_420: the same in 4:2:0, into targets as Batch.decode_420 takes them."""
        targets = list(targets)
        arr = _device_targets_420(targets, order)
        flat = [a for t in targets if t is not None for a in t]
        good = self.lib.L.fiasco_amd_stream_decode_device_420(self.handle, first, len(targets), magnify, smoothing, arr,
                                                              _stream_of(flat, stream))
        if not good:
            raise FiascoError(self.lib.error_message())
        return good

    def decode_planes(self, display, magnify=0):
        """fiasco_amd_stream_decode_planes: the unsmoothed planes of display frame `display` at `magnify`, int16
        [bands, h, w] (12.4 fixed point); the frames it is predicted from are decoded on the way."""
        import numpy
        w, h = self._size(magnify)
        out = numpy.empty((3 if self.info["color"] else 1, h, w), dtype=numpy.int16)
        if not self.lib.L.fiasco_amd_stream_decode_planes(self.handle, display, magnify, out.ctypes.data):
            raise FiascoError(self.lib.error_message())
        return out

    def decode_planes_420(self, display, magnify=0):
        """fiasco_amd_stream_decode_planes_420: the same decoded in 4:2:0: Y [h, w], Cb and Cr [h / 2, w / 2]."""
        import numpy
        w, h = self._size(magnify)
        c = (w // 2) * (h // 2)
        out = numpy.empty(w * h + 2 * c, dtype=numpy.int16)
        if not self.lib.L.fiasco_amd_stream_decode_planes_420(self.handle, display, magnify, out.ctypes.data):
            raise FiascoError(self.lib.error_message())
        return (out[:w * h].reshape(h, w), out[w * h:w * h + c].reshape(h // 2, w // 2), out[w * h + c:].reshape(h // 2, w // 2))

    def free(self):
        if self.handle:
            self.lib.L.fiasco_amd_stream_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class COptions:
    """fiasco_c_options_t with the reference's setter names (fiasco.h:132-174)."""

    def __init__(self, lib):
        self.lib = lib
        self.handle = lib.L.fiasco_c_options_new()
        if not self.handle:
            raise FiascoError(lib.error_message())

    def _call(self, name, *args):
        conv = [a.encode() if isinstance(a, str) else a for a in args]
        ok = getattr(self.lib.L, "fiasco_c_options_" + name)(self.handle, *conv)
        if not ok:
            raise FiascoError(self.lib.error_message())
        return ok

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
