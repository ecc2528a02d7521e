"""The C ABI of libfiasco_amd.so as ctypes sees it: the enum values, the structures, and ABI, the one table of every
function the headers under include/ declare.  Library.__init__ (fiasco_amd/__init__.py) applies the table; nothing else in
the package assigns a restype or argtypes."""
import ctypes


class FiascoError(RuntimeError):
    pass


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


def _declare():
    """header -> {name: (restype, [argtypes])} of every function the header declares, in the header's order; the headers in
    the order they were added.  Handles (options, batches, sequences, renderers, streams that were read, decoders, images), hipStream_t and
    planes travel as void pointers; buffers the callers make with create_string_buffer, and names, as char pointers."""
    c = ctypes
    P, ptr, cstr, i, u, f32, f64 = c.POINTER, c.c_void_p, c.c_char_p, c.c_int, c.c_uint, c.c_float, c.c_double
    size, ul, ull = c.c_size_t, c.c_ulong, c.c_ulonglong
    pnm = [P(cstr), P(size)]                   # raw PNM buffers and their lengths
    streams = [P(ptr), P(size)]                # the .fco byte strings a call hands back, and their lengths
    frames, targets, surfaces, borders = P(DeviceFrame), P(DeviceTarget), P(DeviceSurface), P(Border)
    targets420, ycbcr = P(DeviceTarget420), P(YCbCrFrame)
    return {
        # libfiasco_amd.h and libfiasco_amd_hip.h
        "libfiasco_amd.h": {
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
            "fiasco_amd_batch_decode_psnr": (i, [ptr, u, P(f64), P(f64)]),
            "fiasco_amd_batch_decode_psnr_all": (i, [ptr, P(f64), P(f64)]),
            "fiasco_amd_batch_decode_plane": (i, [ptr, u, u, cstr]),
            "fiasco_amd_batch_decode_planes": (i, [ptr, u, ptr]),
            "fiasco_amd_batch_decode_planes_magnified": (i, [ptr, u, i, ptr]),
            "fiasco_amd_magnified_size": (i, [u, u, i, P(u), P(u)]),
            "fiasco_amd_batch_smoothing_borders": (i, [ptr, u, borders, u]),
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
        },
        # the whole stream of a sequence in one call and its reconstructed frames on the host (every build of the library),
        # videos in device memory in and out (the HIP library)
        "libfiasco_amd_video.h": {
            "fiasco_amd_seq_encode": (i, [ptr, P(ptr), P(size)]),
            "fiasco_amd_seq_keep_reconstructed": (i, [ptr, i]),
            "fiasco_amd_seq_reconstructed_planes": (i, [ptr, u, ptr, P(i)]),
            "fiasco_amd_seq_open_device": (ptr, [u, frames, ptr, f32, ptr, u, u]),
            "fiasco_amd_seq_set_outputs_device": (i, [ptr, P(SeqOutputs)]),
        },
        # decoded frames smoothed along their partition borders on the device, as the reference's decoder shows them (the
        # HIP library)
        "libfiasco_amd_smooth.h": {
            "fiasco_amd_batch_decode_device_smoothed": (i, [ptr, i, targets, ptr]),
            "fiasco_amd_batch_decode_distortion_device_smoothed": (i, [ptr, i, P(ull), P(u), targets, ptr]),
            "fiasco_amd_smooth_planes_device": (i, [ptr, u, u, borders, u, i, ptr]),
        },
        # magnified frames and thumbnails smoothed as `dfiasco` shows them (the border list in every build of the library,
        # the rest in the HIP library)
        "libfiasco_amd_display.h": {
            "fiasco_amd_batch_smoothing_borders_magnified": (i, [ptr, u, i, borders, u]),
            "fiasco_amd_batch_decode_device_shown": (i, [ptr, i, i, targets, ptr]),
            "fiasco_amd_batch_decode_device_thumbnails_shown": (i, [ptr, i, targets, u, targets, ptr]),
            "fiasco_amd_smooth_planes_device_fused": (i, [ptr, u, u, borders, u, i, ptr]),
            "fiasco_amd_smooth_fused": (i, [ull, u]),
        },
        # decoded frames in the pixel formats of a display, as the reference's renderer writes them into an XImage (the
        # handle, the size and the host loop in host code that needs no device; the kernel and the batch entry in the HIP
        # library)
        "libfiasco_amd_render.h": {
            "fiasco_amd_renderer_new": (ptr, [ul, ul, ul, u, i]),
            "fiasco_amd_renderer_delete": (None, [ptr]),
            "fiasco_amd_renderer_surface_size": (i, [ptr, u, u, i, P(u), P(u), P(size)]),
            "fiasco_amd_renderer_render_planes": (i, [ptr, ptr, i, u, u, ptr]),
            "fiasco_amd_planes_render_device": (i, [ptr, i, u, u, ptr, surfaces, ptr]),
            "fiasco_amd_batch_decode_device_rendered": (i, [ptr, ptr, i, i, surfaces, ptr]),
        },
        # decoded frames in 4:2:0 as NV12 / NV21 / I420 buffers (the border list and the host planes' entry in host code,
        # which every build of the library has; the kernel and the batch entry in the HIP library)
        "libfiasco_amd_420.h": {
            "fiasco_amd_batch_decode_device_420": (i, [ptr, i, i, targets420, ptr]),
            "fiasco_amd_batch_decode_planes_420": (i, [ptr, u, i, ptr]),
            "fiasco_amd_batch_smoothing_borders_420": (i, [ptr, u, i, borders, u]),
            "fiasco_amd_planes_to_420_device": (i, [ptr, ptr, ptr, u, u, targets420, ptr]),
        },
        # NV12 / NV21 / I420 / planar 4:4:4 frames into the coder (the host entries in host code, which every build of the
        # library has; the kernel and the device entries in the HIP library)
        "libfiasco_amd_ycbcr.h": {
            "fiasco_amd_batch_stage_ycbcr": (ptr, [u, ycbcr, f32, ptr]),
            "fiasco_amd_seq_open_ycbcr": (ptr, [u, ycbcr, f32, ptr, u, u]),
            "fiasco_amd_batch_stage_device_ycbcr": (ptr, [u, ycbcr, ptr, f32, ptr]),
            "fiasco_amd_batch_upload_device_ycbcr": (i, [ptr, ycbcr, ptr]),
            "fiasco_amd_seq_open_device_ycbcr": (ptr, [u, ycbcr, ptr, f32, ptr, u, u]),
        },
        # frames decoded in 4:2:0 in the pixel formats of a display (the size rule and the host loop in host code that needs
        # no device; the kernel and the batch entry in the HIP library)
        "libfiasco_amd_render_420.h": {
            "fiasco_amd_renderer_surface_size_420": (i, [ptr, u, u, P(u), P(u), P(size)]),
            "fiasco_amd_renderer_render_planes_420": (i, [ptr, ptr, ptr, ptr, u, u, ptr]),
            "fiasco_amd_planes_render_device_420": (i, [ptr, ptr, ptr, u, u, ptr, surfaces, ptr]),
            "fiasco_amd_batch_decode_device_rendered_420": (i, [ptr, ptr, i, i, surfaces, ptr]),
        },
        # .fco streams read back (the reader, the frame order, the rewrite and the border list in host code, which every
        # build of the product has; the decode entries in the HIP library)
        "libfiasco_amd_stream.h": {
            "fiasco_amd_stream_open": (ptr, [cstr, size]),
            "fiasco_amd_stream_open_file": (ptr, [cstr]),
            "fiasco_amd_stream_free": (None, [ptr]),
            "fiasco_amd_stream_get_info": (i, [ptr, P(StreamInfo)]),
            "fiasco_amd_stream_frame_type": (i, [ptr, u]),
            "fiasco_amd_stream_coding_order": (i, [ptr, P(u), u]),
            "fiasco_amd_stream_rewrite": (i, [ptr, P(ptr), P(size)]),
            "fiasco_amd_stream_smoothing_borders": (i, [ptr, u, i, i, borders, u]),
            "fiasco_amd_stream_decode_device": (i, [ptr, u, u, i, i, targets, ptr]),
            "fiasco_amd_stream_decode_device_420": (i, [ptr, u, u, i, i, targets420, ptr]),
            "fiasco_amd_stream_decode_planes": (i, [ptr, u, i, ptr]),
            "fiasco_amd_stream_decode_planes_420": (i, [ptr, u, i, ptr]),
        },
        # the decoder half of fiasco.h -- options, decoder, image, renderer -- and the extensions around it (the objects, the
        # stream's header and the host renderer in host code; the frames in the HIP library)
        "libfiasco_amd_decoder.h": {
            "fiasco_d_options_new": (ptr, []),
            "fiasco_d_options_delete": (None, [ptr]),
            "fiasco_d_options_set_smoothing": (i, [ptr, i]),
            "fiasco_d_options_set_magnification": (i, [ptr, i]),
            "fiasco_d_options_set_4_2_0_format": (i, [ptr, i]),
            "fiasco_decoder_new": (ptr, [cstr, ptr]),
            "fiasco_decoder_delete": (i, [ptr]),
            "fiasco_decoder_write_frame": (i, [ptr, cstr]),
            "fiasco_decoder_get_frame": (ptr, [ptr]),
            "fiasco_decoder_get_width": (u, [ptr]),
            "fiasco_decoder_get_height": (u, [ptr]),
            "fiasco_decoder_is_color": (i, [ptr]),
            "fiasco_decoder_get_rate": (u, [ptr]),
            "fiasco_decoder_get_length": (u, [ptr]),
            "fiasco_decoder_get_title": (cstr, [ptr]),
            "fiasco_decoder_get_comment": (cstr, [ptr]),
            "fiasco_image_new": (ptr, [cstr]),
            "fiasco_image_delete": (None, [ptr]),
            "fiasco_image_get_width": (u, [ptr]),
            "fiasco_image_get_height": (u, [ptr]),
            "fiasco_image_is_color": (i, [ptr]),
            "fiasco_renderer_new": (ptr, [ul, ul, ul, u, i]),
            "fiasco_renderer_delete": (None, [ptr]),
            "fiasco_renderer_render": (i, [ptr, ptr, ptr]),
            "fiasco_amd_decoder_new_memory": (ptr, [cstr, size, ptr]),
            "fiasco_amd_decoder_set_read_ahead": (i, [ptr, u]),
            "fiasco_amd_decoder_position": (i, [ptr]),
            "fiasco_amd_image_get_height": (u, [ptr]),
            "fiasco_amd_image_format": (i, [ptr]),
            "fiasco_amd_image_planes": (i, [ptr, ptr]),
            "fiasco_amd_image_planes_device": (i, [ptr, P(ptr), P(i)]),
            "fiasco_amd_renderer_render_device": (i, [ptr, surfaces, ptr, ptr]),
        },
    }


ABI = _declare()

# the table of each header, and the names it declares in its order: entries of ABI, not copies
_SIGNATURES = ABI["libfiasco_amd.h"]                     # with what libfiasco_amd_hip.h declares
_VIDEO_SIGNATURES = ABI["libfiasco_amd_video.h"]
_SMOOTH_SIGNATURES = ABI["libfiasco_amd_smooth.h"]
_DISPLAY_SIGNATURES = ABI["libfiasco_amd_display.h"]
_RENDER_SIGNATURES = ABI["libfiasco_amd_render.h"]
_YUV420_SIGNATURES = ABI["libfiasco_amd_420.h"]
_YCBCR_SIGNATURES = ABI["libfiasco_amd_ycbcr.h"]
_RENDER420_SIGNATURES = ABI["libfiasco_amd_render_420.h"]
_STREAM_SIGNATURES = ABI["libfiasco_amd_stream.h"]
_DECODER_SIGNATURES = ABI["libfiasco_amd_decoder.h"]
EXPORTED_SYMBOLS = list(_SIGNATURES)
VIDEO_SYMBOLS = list(_VIDEO_SIGNATURES)
SMOOTH_SYMBOLS = list(_SMOOTH_SIGNATURES)
DISPLAY_SYMBOLS = list(_DISPLAY_SIGNATURES)
RENDER_SYMBOLS = list(_RENDER_SIGNATURES)
YUV420_SYMBOLS = list(_YUV420_SIGNATURES)
YCBCR_SYMBOLS = list(_YCBCR_SIGNATURES)
RENDER420_SYMBOLS = list(_RENDER420_SIGNATURES)
STREAM_SYMBOLS = list(_STREAM_SIGNATURES)
DECODER_SYMBOLS = list(_DECODER_SIGNATURES)
