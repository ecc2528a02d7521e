"""The .fco reader against the writer and against the headers the goldens were coded with: host code of the product
library, no device (include/libfiasco_amd_stream.h; csrc/host/fa_reader.c, fa_stream.c, the read side of fa_bitio.c).

Stream.rewrite() sends every frame that was read through fa_write_header / fa_write_frame again; for a stream a coder
wrote the bytes that come out are the bytes that went in.  That pins the reader against the writer field by field --
tree, domain types, nd tree and coefficients, motion tree and vectors, column 0, the delta and chroma matrices, every
weight format, the three flags -- and needs no reference.  The decoded pixels are pinned by tests/test_stream_check.py
(CPU) and tests/test_gpu_stream.py (device)."""
import glob
import hashlib
import json
import os
import re
import subprocess

import pytest

import fiasco_amd
import reconst_cases as rc
import stream_cases as sc
import synth
import video_param_cases as vc
from conftest import GOLDEN, ROOT, options_from_args

FILES = sorted(glob.glob(os.path.join(GOLDEN, "*.fco")))
STREAMS = [f for f in FILES if open(f, "rb").read(7) == b"FIASCO\n"]
BASES = [f for f in FILES if f not in STREAMS]            # long_a / _b / _c.fco are ASCII initial bases ("Fiasco")
NAMES = ["fiasco_amd_stream_open", "fiasco_amd_stream_open_file", "fiasco_amd_stream_free", "fiasco_amd_stream_get_info",
         "fiasco_amd_stream_frame_type", "fiasco_amd_stream_coding_order", "fiasco_amd_stream_rewrite", "fiasco_amd_stream_smoothing_borders",
         "fiasco_amd_stream_decode_device", "fiasco_amd_stream_decode_device_420", "fiasco_amd_stream_decode_planes",
         "fiasco_amd_stream_decode_planes_420"]


def test_header_symbol_list_and_library_hold_the_twelve_names(product, oracle):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "libfiasco_amd_stream.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(fiasco_\w*)\s*\(", src)) == set(NAMES) and fiasco_amd.STREAM_SYMBOLS == NAMES
    assert NAMES == list(fiasco_amd._STREAM_SIGNATURES)
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "fiasco_amd", "csrc", "exports.map")).read(), flags=re.S)
    patterns = re.findall(r"^\s*([\w*]+);", exports.split("local:")[0], flags=re.M)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", fiasco_amd.LIB_PATH]).decode()
    older = (fiasco_amd.EXPORTED_SYMBOLS + fiasco_amd.VIDEO_SYMBOLS + fiasco_amd.SMOOTH_SYMBOLS + fiasco_amd.DISPLAY_SYMBOLS + fiasco_amd.RENDER_SYMBOLS
             + fiasco_amd.YUV420_SYMBOLS + fiasco_amd.YCBCR_SYMBOLS + fiasco_amd.RENDER420_SYMBOLS)
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, src).group(1)
        assert params.count(",") + 1 == len(fiasco_amd._STREAM_SIGNATURES[name][1]), name
        assert name not in older, name
        assert any(re.fullmatch(p.replace("*", r"\w*"), name) for p in patterns), name
        assert re.search(r" T %s$" % name, syms, flags=re.M), name
        assert getattr(product.L, name).argtypes == fiasco_amd._STREAM_SIGNATURES[name][1], name      # bound by Library.__init__
        assert not hasattr(oracle.L, name), name               # the oracle library names its sources: no reader
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-Werror", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
                           "-x", "c", os.path.join(ROOT, "include", "libfiasco_amd_stream.h")])
    with pytest.raises(fiasco_amd.FiascoError, match="has no stream reader"):
        fiasco_amd.Stream(oracle, b"FIASCO\n")


@pytest.mark.parametrize("path", STREAMS, ids=[os.path.basename(p) for p in STREAMS])
def test_rewrite_gives_the_bytes_of_every_golden_stream(product, path):
    data = open(path, "rb").read()
    s = fiasco_amd.Stream(product, data)
    assert s.rewrite() == data
    assert sorted(s.coding_order) == list(range(s.n)) and s.coding_order[0] == 0 and s.frame_types[0] == 0
    f = fiasco_amd.Stream(product, path, filename=True)           # ... and from its file
    assert f.info == s.info and f.frame_types == s.frame_types and f.rewrite() == data
    s.free(); f.free()


def test_there_are_streams_of_every_kind():
    assert len(STREAMS) >= 45 and len(BASES) == 3


@pytest.mark.parametrize("what", ["prediction_still", "colour_ipbbp", "mantissas_2_7", "b_as_past_ref_0"])
def test_rewrite_gives_the_bytes_of_streams_the_oracle_codes(product, oracle, what, tmp_path):
    if what == "prediction_still":
        frames, args = [synth.pgm_bytes(synth.synth(96, 64, 3))], ["--prediction", "-q", "60"]
    elif what == "colour_ipbbp":
        frames, args = [synth.ppm_bytes(synth.synth_color_k(70, 50, 6, f)) for f in range(5)], ["--pattern", "ipbbp", "-q", "10"]
    elif what == "mantissas_2_7":
        frames, args = rc._shift(3), ["--pattern", "ibp", "--rpf-mantissa", "2", "--dc-rpf-mantissa", "7"]
    else:
        frames, args = rc._shift(4), ["--pattern", "ibbp"]
    if what == "b_as_past_ref_0":
        stream, _, _, msg = vc.run_library(oracle, frames, args, (30, 1, 0), tmp_path)
    else:
        stream, _, _, msg = rc.run_library(oracle, frames, args, tmp_path)
    assert stream is not None, msg
    s = fiasco_amd.Stream(product, stream)
    assert s.rewrite() == stream
    w, h, nb = rc.geometry(frames)
    assert (s.info["width"], s.info["height"], s.info["color"], s.n) == (w, h, int(nb == 3), len(frames))
    if what == "colour_ipbbp":
        assert s.frame_types == [0, 1, 2, 2, 1] and s.coding_order == [0, 1, 4, 2, 3]
    if what == "mantissas_2_7":
        assert [s.info[k] for k in ("rpf_mantissa", "dc_rpf_mantissa", "d_rpf_mantissa", "d_dc_rpf_mantissa")] == [2, 7, 3, 5]      # the delta formats keep their defaults
    if what == "b_as_past_ref_0":
        assert (s.info["B_as_past_ref"], s.info["fps"]) == (0, 30)
    s.free()


def test_info_against_the_manifests(product, manifest):
    """size, colour, frames and the options a case was coded with, for every golden stream the manifest knows"""
    seen = 0
    for case in manifest["cases"] + manifest["video_cases"]:
        if not case.get("file"):
            continue
        s = fiasco_amd.Stream(product, open(os.path.join(GOLDEN, case["file"]), "rb").read())
        ent = manifest["inputs"][case["inputs"][0]]
        a = case["args"]
        assert hashlib.md5(open(os.path.join(GOLDEN, case["file"]), "rb").read()).hexdigest() == case["md5"]
        if "args" in ent and "w" in ent.get("args", {}):
            assert (s.info["width"], s.info["height"]) == (ent["args"]["w"], ent["args"]["h"]), case["name"]
        assert s.info["color"] == int(ent["ext"] == "ppm") and s.n == len(case["inputs"]) == s.info["frames"], case["name"]
        assert s.info["basis_name"] == "small.fco" and s.info["smoothing"] == 70, case["name"]
        assert s.info["rpf_mantissa"] == (int(a[a.index("--rpf-mantissa") + 1]) if "--rpf-mantissa" in a else 3), case["name"]
        assert s.info["dc_rpf_mantissa"] == (int(a[a.index("--dc-rpf-mantissa") + 1]) if "--dc-rpf-mantissa" in a else 5), case["name"]
        assert s.info["title"] == (a[a.index("-t") + 1] if "-t" in a else ""), case["name"]
        assert s.info["comment"] == (a[a.index("-c") + 1] if "-c" in a else ""), case["name"]
        if s.n > 1:
            assert (s.info["fps"], s.info["B_as_past_ref"], s.info["half_pixel"]) == (25, 1, 0), case["name"]
            if "--pattern" in a:
                pattern = a[a.index("--pattern") + 1]
                want = ["ipb".index(pattern[d % len(pattern)]) if d else 0 for d in range(s.n)]
                if want[-1] == 2:
                    want[-1] = 1                    # a trailing B frame is coded as a P frame
                assert s.frame_types == want, case["name"]
        seen += 1
        s.free()
    assert seen >= 35
    vp = json.load(open(os.path.join(GOLDEN, "VIDEO_PARAM.json")))["cases"]
    fx = sc.fixture()["streams"]
    s = fiasco_amd.Stream(product, sc.stream_bytes(sc.IBBP_B0))
    assert (s.info["B_as_past_ref"], s.info["fps"], s.frame_types, s.coding_order) == (0, 25, [0, 2, 2, 1], [0, 3, 1, 2])
    assert s.frame_types == [f["type"] for f in vp["colour_ibbp_x4_fps25_cross1_b0"]["frames"]] == fx[sc.IBBP_B0]["frame_types"]
    s.free()
    s = fiasco_amd.Stream(product, sc.stream_bytes("st_longa_g256"))
    assert s.info["basis_name"] == "long_a.fco"
    s.free()


def _flip(data, predicate, first=0, last=None):
    """the single-bit flips of bytes first .. last of `data` whose refusal `predicate` accepts"""
    out = []
    for bit in range(8 * first, 8 * (len(data) if last is None else last)):
        d = bytearray(data)
        d[bit // 8] ^= 0x80 >> (bit % 8)
        out.append(bytes(d))
    return out


def test_refusals_each_with_its_sentence(product, tmp_path):
    data = sc.stream_bytes("g32x32_q20")

    def refused(d):
        with pytest.raises(fiasco_amd.FiascoError) as e:
            fiasco_amd.Stream(product, d)
        return str(e.value)

    assert refused(b"") == "Input file <memory> is not a valid FIASCO file!"
    assert refused(b"Fiasco\n" + data[7:]) == "Input file <memory> is not a valid FIASCO file!"
    for path in BASES:                                      # an ASCII basis is no stream
        assert "is not a valid FIASCO file!" in refused(open(path, "rb").read())
    with pytest.raises(fiasco_amd.FiascoError, match="No such file|not a valid|I/O Error"):
        fiasco_amd.Stream(product, str(tmp_path / "none.fco"), filename=True)
    # the release: Rice code of 2 with k = 8 right behind the basis name (9 bits: 0, then 00000010)
    at = 7 + len(b"small.fco\0")
    assert data[at:at + 2] == bytes([0x01, 0x00])
    assert refused(data[:at] + bytes([0x01, 0x80]) + data[at + 2:]) == ("Can't decode FIASCO files of file format release `3'.\n"
                                                                         "Current file format release is `2'.")
    assert "release `1'" in refused(data[:at] + bytes([0x00, 0x80]) + data[at + 2:])
    # truncation anywhere: every proper prefix of the 59 bytes
    assert len(data) == 59
    for n in range(1, len(data)):
        msg = refused(data[:n])
        assert "truncated" in msg or "not a valid FIASCO file" in msg, (n, msg)
    # the tiling flag: the first bit behind the frame header (three Rice codes, aligned)
    s = fiasco_amd.Stream(product, data)
    assert s.rewrite() == data
    s.free()
    tiled = [d for d in _flip(data, None) if "tiling" in (refused(d) if _refuses(product, d) else "")]
    assert tiled and refused(tiled[0]) == "Image tiling is not supported: no coder writes it (the tiling flag of frame 0 is set)."
    # a basis that cannot be loaded
    named = data[:7] + b"nosuch.fco\0" + data[at:]
    assert "nosuch.fco" in refused(named)
    # symbols outside their alphabet, trees and edges no coder writes: among all single-bit flips some are refused with
    # each of these sentences, and every refusal has one
    every = [refused(d) for d in _flip(data, None) if _refuses(product, d)]
    assert all(every) and len(every) > 300
    # (a symbol outside its alphabet: a header item of no known type, a mantissa outside [2,8], a frame type above 2, more
    # edges per range than five; the arithmetic decoders cannot leave theirs on any input, and are checked all the same)
    for part in ("header item of unknown type", "a mantissa of 9 bits is outside the interval [2,8]", "Stream error: frame type", "edges per range",
                 "the bintree has", "Stream error: a frame of"):
        assert any(part in m for m in every), part
    # a motion vector outside the search range, a vector that leaves the frame: flips of a video's motion section
    video = sc.stream_bytes("seq2_gray_ip")
    msgs = [refused(d) for d in _flip(video, None) if _refuses(product, d)]
    assert any("motion vector" in m for m in msgs) and "wrong huffman code !" in msgs
    assert any("frames are not in an order a coder writes" in m or "frame number" in m for m in msgs)


def _refuses(lib, data):
    try:
        fiasco_amd.Stream(lib, data).free()
        return False
    except fiasco_amd.FiascoError:
        return True


def test_half_pixel_stream_is_read(product):
    data = sc.half_pixel_stream(product)
    s = fiasco_amd.Stream(product, data)
    assert s.info["half_pixel"] == 1 and s.rewrite() == data
    s.free()


def test_orphaned_b_frames_are_read_and_the_coders_refuse_the_pattern(product, oracle, tmp_path):
    """I0 I3 B1 B2: the order get_next_frame walks without complaint and no coder writes"""
    data = sc.orphaned_b_stream()
    s = fiasco_amd.Stream(product, data)
    assert s.frame_types == [0, 2, 2, 0] and s.coding_order == [0, 3, 1, 2] and s.rewrite() == data
    s.free()
    stream, _, _, msg = rc.run_library(oracle, rc._shift(4), ["--pattern", "ibbi"], tmp_path)
    assert stream is None and msg == vc.REFUSAL


def test_borders_of_a_stream_are_those_of_the_batch_that_wrote_it(product, oracle):
    """intra frames: Stream.smoothing_borders() against Batch.smoothing_borders() of the oracle on the same automaton, at
    every magnification and in 4:2:0; P and B frames have lists of their own automaton"""
    pnm = synth.ppm_bytes(synth.synth_color_k(102, 66, 5, 0))
    q, o = options_from_args(oracle, [])
    b = fiasco_amd.Batch(oracle, [pnm], q, o)
    stream = b.encode()[0]
    s = fiasco_amd.Stream(product, stream)
    for m in (-1, 0, 1):
        assert s.smoothing_borders(0, magnify=m) == b.smoothing_borders(0, magnify=m)
        assert s.smoothing_borders(0, magnify=m, format_420=True) == b.smoothing_borders_420(0, magnify=m)
    b.free(); o.delete(); s.free()
    v = fiasco_amd.Stream(product, sc.stream_bytes(sc.IPBBP))
    lists = [v.smoothing_borders(d) for d in range(v.n)]
    assert all(lists) and len({tuple(x) for x in lists}) > 1
    assert all(v.smoothing_borders(d, magnify=-1, format_420=True) for d in range(v.n))
    with pytest.raises(fiasco_amd.FiascoError, match="no frame 5"):
        v.smoothing_borders(5)
    v.free()
