"""The decoder half of fiasco.h on the host (include/libfiasco_amd_decoder.h; csrc/host/fa_decoder.c): the header, the
symbols and the structures, the options' and the decoder's sentences, the getters, images read from PNM files and the
renderer on host images.  No device: what needs one fails with the library's no-device message.

Yardsticks: tests/golden/DECODER_API.json (tests/golden/make_decoder_api.py: what the reference's library says through the
same names), tests/golden/DECODED_STREAMS.json for the refusals of the option tuples, and the reference's own fiasco.h for
the layout of the four structures where its tree is present."""
import ctypes
import glob
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import fiasco_amd
import render_ref
import stream_cases as sc
from conftest import GOLDEN, ROOT

API = json.load(open(os.path.join(GOLDEN, "DECODER_API.json")))
INCLUDE = os.path.join(ROOT, "include")
HEADER = os.path.join(INCLUDE, "libfiasco_amd_decoder.h")
FIASCO_H = ["fiasco_d_options_new", "fiasco_d_options_delete", "fiasco_d_options_set_smoothing", "fiasco_d_options_set_magnification",
            "fiasco_d_options_set_4_2_0_format", "fiasco_decoder_new", "fiasco_decoder_delete", "fiasco_decoder_write_frame",
            "fiasco_decoder_get_frame", "fiasco_decoder_get_width", "fiasco_decoder_get_height", "fiasco_decoder_is_color",
            "fiasco_decoder_get_rate", "fiasco_decoder_get_length", "fiasco_decoder_get_title", "fiasco_decoder_get_comment",
            "fiasco_image_new", "fiasco_image_delete", "fiasco_image_get_width", "fiasco_image_get_height", "fiasco_image_is_color",
            "fiasco_renderer_new", "fiasco_renderer_delete", "fiasco_renderer_render"]
NAMES = FIASCO_H + ["fiasco_amd_decoder_new_memory", "fiasco_amd_decoder_set_read_ahead", "fiasco_amd_decoder_position",
                    "fiasco_amd_image_get_height", "fiasco_amd_image_format", "fiasco_amd_image_planes",
                    "fiasco_amd_image_planes_device", "fiasco_amd_renderer_render_device"]
NO_DEVICE = "no HIP device available"
STREAMS = [f for f in sorted(glob.glob(os.path.join(GOLDEN, "*.fco"))) if open(f, "rb").read(7) == b"FIASCO\n"]


def test_header_symbol_list_and_library_agree(product, oracle):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = re.findall(r"^(?!typedef)[\w \*]*?\b(fiasco_\w+)\s*\(", src, flags=re.M)
    assert declared == NAMES == fiasco_amd.DECODER_SYMBOLS == list(fiasco_amd._DECODER_SIGNATURES)
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    older = (fiasco_amd.EXPORTED_SYMBOLS + fiasco_amd.VIDEO_SYMBOLS + fiasco_amd.SMOOTH_SYMBOLS + fiasco_amd.DISPLAY_SYMBOLS + fiasco_amd.RENDER_SYMBOLS
             + fiasco_amd.YUV420_SYMBOLS + fiasco_amd.YCBCR_SYMBOLS + fiasco_amd.RENDER420_SYMBOLS + fiasco_amd.STREAM_SYMBOLS)
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        want = 0 if params.strip() == "void" else params.count(",") + 1
        assert want == len(fiasco_amd._DECODER_SIGNATURES[name][1]), name
        assert name not in older, name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert getattr(product.L, name).argtypes == fiasco_amd._DECODER_SIGNATURES[name][1], name      # bound by Library.__init__
        assert not hasattr(oracle.L, name), name               # the oracle library names its sources: no decoder objects


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_header_compiles_alone(lang):
    subprocess.check_call(["gcc", "-Wall", "-Werror", "-fsyntax-only", "-I" + INCLUDE, "-x", lang, HEADER])


STRUCTS = {"fiasco_image_t": ["delete", "get_width", "get_height", "is_color", "private"],
           "fiasco_decoder_t": ["delete", "write_frame", "get_frame", "get_length", "get_rate", "get_width", "get_height", "get_title", "get_comment",
                                "is_color", "private"],
           "fiasco_d_options_t": ["delete", "set_smoothing", "set_magnification", "set_4_2_0_format", "private"],
           "fiasco_renderer_t": ["render", "delete", "private"]}


def _layout(tmp_path, label, include_dir, header, rename):
    body = "".join('    printf("%s %%zu\\n", sizeof(%s));\n' % (t, t) + "".join(
        '    printf("%s.%s %%zu\\n", offsetof(%s, %s));\n' % (t, m, t, m + "_" if rename and m in ("delete", "private") else m) for m in members)
        for t, members in STRUCTS.items())
    src = tmp_path / (label + ".c")
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void)\n{\n%s    return 0;\n}\n' % (header, body))
    exe = str(tmp_path / label)
    subprocess.check_call(["gcc", "-std=gnu99", "-I" + include_dir, "-o", exe, str(src)])
    return subprocess.check_output([exe]).decode()


def test_structures_have_the_layout_of_the_references_fiasco_h(tmp_path):
    ours = _layout(tmp_path, "ours", INCLUDE, "libfiasco_amd_decoder.h", True)
    assert len(ours.strip().split("\n")) == sum(len(m) + 1 for m in STRUCTS.values())
    # every member is a pointer: the offsets are multiples of its size, in the order of fiasco.h
    for t, members in STRUCTS.items():
        assert [int(v) for v in re.findall(r"^%s\.\w+ (\d+)$" % t, ours, flags=re.M)] == [k * ctypes.sizeof(ctypes.c_void_p) for k in range(len(members))]
    # the tree oracle/ref_build.sh builds from: FIASCO_REFERENCE, or the default the script names
    recipe = open(os.path.join(ROOT, "oracle", "ref_build.sh")).read()
    ref = os.environ.get("FIASCO_REFERENCE") or re.search(r"^REF=\$\{FIASCO_REFERENCE:-([^}]+)\}", recipe, flags=re.M).group(1)
    if not os.path.exists(os.path.join(ref, "fiasco.h")):
        pytest.skip("the reference tree is not here: compared with the member lists of fiasco.h above only")
    assert _layout(tmp_path, "theirs", ref, "fiasco.h", False) == ours


def test_a_caller_of_every_fiasco_h_decoder_name_links_and_runs(tmp_path):
    exe = str(tmp_path / "decoder_api_user")
    libdir = os.path.dirname(fiasco_amd.LIB_PATH)
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-I" + INCLUDE, "-o", exe, os.path.join(ROOT, "tests", "decoder_api_user.c"),
                           "-L" + libdir, "-lfiasco_amd", "-Wl,-rpath," + libdir])
    out = subprocess.check_output([exe, sc.stream_path(sc.IBBP_B0)]).decode().split()
    want = API["info"][sc.IBBP_B0]["0"]
    assert [int(v) for v in out] == [want[k] for k in ("width", "height", "length", "rate", "color")]
    src = open(os.path.join(ROOT, "tests", "decoder_api_user.c")).read()
    assert all(re.search(r"\(const void \*\) %s\b" % n, src) for n in FIASCO_H)


def _message(lib):
    return lib.error_message()


def test_option_sentences_and_defaults(product):
    L, msg = product.L, API["messages"]
    o = L.fiasco_d_options_new()
    for v in (-2, 101):
        assert L.fiasco_d_options_set_smoothing(o, v) == 0 and _message(product) == msg["smoothing_%d" % v]
    for v in (-1, 0, 100):
        assert L.fiasco_d_options_set_smoothing(o, v) == 1
    assert L.fiasco_d_options_set_magnification(o, -7) == 1 and L.fiasco_d_options_set_4_2_0_format(o, 5) == 1
    methods = (ctypes.c_void_p * 5).from_address(o)
    assert all(methods[k] for k in range(5))                     # delete, the three setters, private
    null = (ctypes.c_void_p * 5)()
    assert L.fiasco_d_options_set_smoothing(ctypes.addressof(null), 10) == 0 and _message(product) == msg["options_null"]
    other = ctypes.create_string_buffer(b"XXXXXXXX", 64)
    wrong = (ctypes.c_void_p * 5)(None, None, None, None, ctypes.addressof(other))
    assert L.fiasco_d_options_set_magnification(ctypes.addressof(wrong), 0) == 0 and _message(product) == msg["options_wrong_type"]
    assert not L.fiasco_decoder_new(sc.stream_path("g256").encode(), ctypes.addressof(wrong)) and _message(product) == msg["options_wrong_type"]
    L.fiasco_d_options_delete(o)


def test_magnification_limits_with_the_references_sentences(product):
    for key in ("too_small", "too_small_2", "too_large", "too_large_2"):
        case = API["messages"][key]
        assert "Magnifaction" in case["message"]
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.Decoder(product, sc.stream_path(case["stream"]), magnify=case["magnify"])
        assert str(e.value) == case["message"], key


@pytest.mark.parametrize("name", sc.NAMES)
def test_getters_equal_the_references(product, name):
    fx = sc.fixture()["streams"][name]["decoded"]
    for m in sc.MAGNIFY:
        want = API["info"][name][str(m)]
        if "refused" in want:
            with pytest.raises(fiasco_amd.FiascoError) as e:
                fiasco_amd.Decoder(product, sc.stream_bytes(name), magnify=m)
            assert str(e.value) == want["refused"] == fx[sc.key_of(m, "444", 0)]["refused"]
            continue
        d = fiasco_amd.Decoder(product, sc.stream_path(name), magnify=m, format_420=bool(m & 1))
        assert (d.width, d.height, d.length, d.rate, int(d.color), d.title, d.comment) == tuple(
            want[k] for k in ("width", "height", "length", "rate", "color", "title", "comment"))
        d.delete()


@pytest.mark.parametrize("path", STREAMS, ids=[os.path.basename(p) for p in STREAMS])
def test_every_golden_stream_opens_without_a_device_and_decodes_only_with_one(product, path, tmp_path):
    d = fiasco_amd.Decoder(product, path)
    s = fiasco_amd.Stream(product, path, filename=True)
    assert (d.length, d.rate, d.color) == (s.n, s.info["fps"], bool(s.info["color"]))
    assert (d.width, d.height) == (s.info["width"] + (s.info["width"] & 1), s.info["height"] + (s.info["height"] & 1))
    s.free()
    if not os.path.exists("/dev/kfd"):
        with pytest.raises(fiasco_amd.FiascoError, match=NO_DEVICE):
            d.get_frame()
        with pytest.raises(fiasco_amd.FiascoError, match=NO_DEVICE):
            d.write_frame(tmp_path / "never.pnm")
        assert not (tmp_path / "never.pnm").exists()
    d.delete()
    d.delete()


def test_streams_the_reader_refuses_are_refused_with_its_sentence(product, tmp_path):
    data = sc.stream_bytes("seq2_gray_ip")
    for bad, what in ((b"FIASCX\n" + data[7:], "magic"), (data[:len(data) // 2], "truncated"), (data[:20], "truncated header")):
        with pytest.raises(fiasco_amd.FiascoError) as by_stream:
            fiasco_amd.Stream(product, bad)
        with pytest.raises(fiasco_amd.FiascoError) as by_decoder:
            fiasco_amd.Decoder(product, bad)
        assert str(by_decoder.value) == str(by_stream.value) and str(by_stream.value), what
    # a tiling stream: the flag of the first frame's header set (no coder of this project writes it; the reader names it)
    found = 0
    for bit in range(8 * 40, 8 * 120):
        flipped = bytearray(data)
        flipped[bit // 8] ^= 0x80 >> (bit % 8)
        try:
            fiasco_amd.Stream(product, bytes(flipped)).free()
        except fiasco_amd.FiascoError as e:
            if "iling" in str(e):
                with pytest.raises(fiasco_amd.FiascoError) as by_decoder:
                    fiasco_amd.Decoder(product, bytes(flipped))
                assert str(by_decoder.value) == str(e)
                found += 1
                break
    assert found == 1
    with pytest.raises(fiasco_amd.FiascoError, match="I/O Error"):
        fiasco_amd.Decoder(product, tmp_path / "there_is_no_such.fco")
    with pytest.raises(fiasco_amd.FiascoError, match="n >= 1"):
        fiasco_amd.Decoder(product, data, read_ahead=0)


def test_get_frame_in_420_on_a_gray_stream_is_refused(product):
    """what the reference hands out there is recorded (tests/golden/DECODER_API.json gray_420) and not reproduced"""
    d = fiasco_amd.Decoder(product, sc.stream_bytes("seq4_gray_ibbp"), format_420=True)
    with pytest.raises(fiasco_amd.FiascoError, match="4:2:0: a gray frame has no chroma bands"):
        d.get_frame()
    assert d.position == 0                      # a call that is refused as a whole consumes nothing
    d.delete()


@pytest.mark.parametrize("name", sorted(API["images"]))
def test_images_from_pnm_files_and_the_renderer_on_them(product, name):
    want = API["images"][name]
    im = fiasco_amd.Image.open(product, os.path.join(GOLDEN, name))
    # the reference's fiasco_image_get_height returns the width (lib/image.c:127-135), and so does this library's; the height
    # comes from fiasco_amd_image_get_height
    assert product.L.fiasco_image_get_height(im.handle) == want["get_height"] == want["get_width"] == im.width
    assert (im.height, int(im.color), im.format_420) == (want["height"], want["color"], False)
    planes = im.planes()
    assert hashlib.md5(np.ascontiguousarray(planes, "<i2").tobytes()).hexdigest() == want["planes_md5"]
    for rname, md5 in want["ximage_md5"].items():
        bpp, red, green, blue, doubled = render_ref.RENDERERS[rname]
        r = fiasco_amd.Renderer(product, red, green, blue, bpp, doubled)
        got = im.render(r)                                          # a host image: the host loops
        assert got == r.render_planes(planes if im.color else planes[0]) and hashlib.md5(got).hexdigest() == md5, (name, rname)
        r.delete()
    im.delete()
    im.delete()


def test_image_and_renderer_refusals(product, tmp_path):
    with pytest.raises(fiasco_amd.FiascoError, match="I/O Error"):
        fiasco_amd.Image.open(product, tmp_path / "none.pgm")
    odd = tmp_path / "odd.pgm"
    odd.write_bytes(b"P5\n33 32\n255\n" + bytes(33 * 32))
    with pytest.raises(fiasco_amd.FiascoError, match="must be even numbers"):
        fiasco_amd.Image.open(product, odd)
    assert not product.L.fiasco_renderer_new(0xf800, 0x7e0, 0x1f, 15, 0)
    assert product.error_message() == "Rendering depth of XImage must be 16, 24, or 32 bpp."
    im = fiasco_amd.Image.open(product, os.path.join(GOLDEN, "g100x70.pgm"))
    r = fiasco_amd.Renderer(product, 0xf800, 0x7e0, 0x1f, 16)
    buf = ctypes.create_string_buffer(16)
    for args, who in (((None, buf, im.handle), "this"), ((r.fiasco_renderer(), None, im.handle), "ximage"), ((r.fiasco_renderer(), buf, None), "fiasco_image")):
        assert product.L.fiasco_renderer_render(*args) == 0 and product.error_message() == "Parameter `%s' not defined (NULL)." % who
    r.delete(); im.delete()
