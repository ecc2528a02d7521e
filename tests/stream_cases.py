"""What tests/golden/make_decoded_streams.py, tests/test_stream_reader.py, tests/test_stream_check.py (CPU) and
tests/test_gpu_stream.py (device) share: the streams of tests/golden/DECODED_STREAMS.json, the option tuples, file handling.
No codec logic here.

The fixture holds, per stream and option tuple "<magnify>:<444|420>:<smoothing>", either {"refused": the reference's
message} or the size shown and, per display frame, its type and two md5s of what the REFERENCE's decoder library hands out
(fiasco_decoder_get_frame of oracle/_ref/libfiasco_ref.so): "planes_md5" of the int16 12.4 planes (4:4:4: all bands back to
back; 4:2:0: Y, then Cb and Cr of (W >> 1) x (H >> 1) values) and "pixels_md5" of the bytes (4:4:4: pixels_ref.
pixels_of_planes, the payload of the PGM / PPM `dfiasco -o' writes; 4:2:0: yuv420_ref.i420, Y | Cb | Cr).  "left_out" names
the tuples the reference dies on, with the reason.  The md5s and the sizes are the reference's.  Two fields come through the
product's own reader, because the reference's decoder interface does not hand them out: "frame_types" (tests/stream_check.c
offsets; the yardstick for the types is the pattern of MANIFEST.json, tests/test_stream_reader.py) and the header's
"smoothing" (the value that smoothing -1 stands for; a wrong one shows in the smoothed md5s)."""
import json
import os

from conftest import GOLDEN

FIXTURE = os.path.join(GOLDEN, "DECODED_STREAMS.json")

STILLS = ["g32x32_q20", "g100x70_q20", "pred_g256", "g256_z1", "g256_rpf", "st_longa_g256"]
VIDEOS = ["seq2_gray_ip", "seq4_gray_ippp", "seq4_gray_ipbb", "seq4_gray_ibbp", "seq4_gray_ibbp_pred_q60", "seq3_color_carry48",
          "seq3_color_carry74"]
IPBBP = "st_color_ipbbp_64"                 # reference-coded, 64 x 64, five frames
IBBP_B0 = "st_color_ibbp_70x66_b0"          # reference-coded through its library with B_as_past_ref off, ragged 70 x 66
SATURATED = "st_color_sat_ibp_100x70"      # reference-coded, saturated colours that move: chroma at both clip bounds in P and B frames
WRAPPED = "st_color_wrap_ibbp_70x66"        # IBBP_B0 with a forward block of its P frame and a backward block of each B frame moved
                                            # 3 pixels over the right edge of the frame (tests/stream_check.c wrap): no coder writes it
NEW = [IPBBP, IBBP_B0, SATURATED, WRAPPED]
NAMES = STILLS + VIDEOS + NEW
ORPHAN = "st_orphan_ibbi"                   # I0 I3 B1 B2: frames of two reference-coded streams spliced (make_decoded_streams.py)

MAGNIFY = [-1, 0, 1]
SMOOTHING = [0, -1, 35]
# the pinned videos of RECONST.json that are coded at the default mantissas: the reference coder's reconstruction IS what
# `dfiasco -s 0' shows
RECONST_NAMES = ["shift100x70_ibbp", "shift100x70_ibp", "shift100x70_ibbp_pred", "noise100x70_ibbp", "sat_q60_ibp", "blend_q60_ibp", "gops_ibpi"]


def fixture():
    return json.load(open(FIXTURE))


def stream_path(name):
    return os.path.join(GOLDEN, name + ".fco")


def stream_bytes(name):
    return open(stream_path(name), "rb").read()


def orphaned_b_stream():
    return stream_bytes(ORPHAN)


def key_of(magnify, fmt, smoothing):
    return "%d:%s:%d" % (magnify, fmt, smoothing)


def parse_key(key):
    m, fmt, s = key.split(":")
    return int(m), fmt, int(s)


def half_pixel_stream(lib):
    """seq2_gray_ip with the half-pixel bit of its header set: the one single-bit flip of the header that changes that flag
    and nothing else the reader reports (host code: any build of the product)"""
    import fiasco_amd
    data = stream_bytes("seq2_gray_ip")
    plain = fiasco_amd.Stream(lib, data)
    want = dict(plain.info, half_pixel=1)
    types = plain.frame_types
    plain.free()
    found = []
    for bit in range(8 * 48):
        flipped = bytearray(data)
        flipped[bit // 8] ^= 0x80 >> (bit % 8)
        try:
            s = fiasco_amd.Stream(lib, bytes(flipped))
        except fiasco_amd.FiascoError:
            continue
        if s.info == want and s.frame_types == types:
            found.append(bytes(flipped))
        s.free()
    assert len(found) == 1, len(found)
    return found[0]
