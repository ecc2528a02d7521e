#!/usr/bin/env python3
"""Frames of .fco streams as the REAL reference's decoder hands them out, video frames included:
tests/golden/DECODED_STREAMS.json.  Build container only (oracle/_ref from oracle/ref_build.sh).

The reference library oracle/_ref/libfiasco_ref.so is driven through ctypes as tests/golden/make_decoded_420.py drives
it -- fiasco_d_options_set_magnification / _set_smoothing / _set_4_2_0_format, fiasco_decoder_new, one
fiasco_decoder_get_frame per display frame -- and the planes are read out of image_t.  One child process per (stream,
option tuple): the reference ends the process on some inputs, and such a tuple is left out BY NAME with how it ended.
A tuple the reference refuses with a message is recorded as refused.

Streams (tests/stream_cases.py): golden stills and videos that are committed already, and six that this script makes
and commits as fixtures:
  st_longa_g256             `cfiasco_ref --basis-name long_a.fco' on g256
  st_color_ipbbp_64         `cfiasco_ref --pattern ipbbp -q 40' on five tinted 64 x 64 windows of one moving frame
  st_color_ibbp_70x66_b0    the reference LIBRARY with set_video_param(25, 0, 1, B_as_past_ref = 0), `ibbp', ragged 70 x 66
  st_color_sat_ibp_100x70   `cfiasco_ref -q 60 --pattern ibp' on reconst_cases._saturated: chroma at both clip bounds
  st_color_wrap_ibbp_70x66  st_color_ibbp_70x66_b0 with a forward block of the P frame and a backward block of each B frame given
                            a vector that carries it 3 pixels over the right edge (tests/stream_check.c wrap; written by
                            fa_write_frame).  The reference's search never yields such a vector; its decoder, which addresses
                            linearly, takes it at every magnification and in 4:2:0
  st_orphan_ibbi            not decoded here: I0 and the B frames of an `ibbp' stream with I3 of the `iiii' stream of the
                            same frames in place of P3 (the frames of a stream are byte-aligned units behind equal headers;
                            tests/stream_check.c gives the offsets).  No coder writes that order (the reference dies on
                            it); the reader accepts it and the decoder fails its B frames: tests/test_gpu_stream.py
Asserted here, or the script fails: a video is accepted at magnification -1 and one at +1; in 4:2:0 a forward, a backward
and an interpolated block carry a vector with a negative odd component; a chroma sample of a P or B frame sits at a clip
bound; a motion block leaves the frame on the right (those of st_color_wrap_ibbp_70x66: no coder writes one)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), HERE]
import conftest  # noqa: E402
import pixels_ref  # noqa: E402
import reconst_cases as rc  # noqa: E402
import stream_cases as sc  # noqa: E402
import synth  # noqa: E402
import video_param_cases as vc  # noqa: E402
import yuv420_ref  # noqa: E402
from make_decoded_420 import FiascoImage, Image, load  # noqa: E402

c = ctypes
ENV = dict(os.environ, FIASCO_DATA=conftest.GOLDEN + ":" + conftest.REF_SHARE)


def tinted(n, w, h, seed):
    """windows of one frame that move by (3, 2) pixels per frame, R, G, B = gray + 30, - 20, + 10.  The seeds used below are
    ones whose video the reference codes: it ends most small colour videos with `Can't write more than n weights'"""
    a = synth.synth(200, 160, seed).astype(np.int32)
    return [synth.ppm_bytes(np.clip(np.stack([a[10 + 2 * i:10 + h + 2 * i, 20 + 3 * i:20 + w + 3 * i] + d for d in (30, -20, 10)], -1),
                                    0, 255).astype(np.uint8)) for i in range(n)]


def child(fco, magnify, smoothing, subsampled):
    """one decode of every frame by the reference library; prints one JSON line"""
    L = load()
    L.fiasco_decoder_get_length.argtypes = [c.c_void_p]
    L.fiasco_decoder_get_length.restype = c.c_uint
    o = L.fiasco_d_options_new()
    assert L.fiasco_d_options_set_magnification(o, magnify) == 1
    if smoothing >= 0:                      # -1: not set, the header's value
        assert L.fiasco_d_options_set_smoothing(o, smoothing) == 1
    assert L.fiasco_d_options_set_4_2_0_format(o, 1 if subsampled else 0) == 1
    d = L.fiasco_decoder_new(fco.encode(), o)
    if not d:
        print(json.dumps({"refused": L.fiasco_get_error_message().decode("latin-1")}))
        return
    frames, clipped = [], 0
    for k in range(L.fiasco_decoder_get_length(d)):
        image = L.fiasco_decoder_get_frame(d)
        if not image:
            print(json.dumps({"refused": L.fiasco_get_error_message().decode("latin-1"), "at_frame": k}))
            return
        im = c.cast(image.contents.private, c.POINTER(Image)).contents
        w, h, colour = im.width, im.height, bool(im.color)
        cw, ch = (w >> 1, h >> 1) if subsampled else (w, h)
        planes = [np.ctypeslib.as_array(im.pixels[0], (h, w)).copy()]
        if colour:
            planes += [np.ctypeslib.as_array(im.pixels[b], (ch, cw)).copy() for b in (1, 2)]
        if subsampled:
            px = yuv420_ref.i420(*planes)
        else:
            px = np.ascontiguousarray(pixels_ref.pixels_of_planes(np.stack(planes) if colour else planes[0]), np.uint8).tobytes()
        frames.append({"planes_md5": hashlib.md5(b"".join(np.ascontiguousarray(p, "<i2").tobytes() for p in planes)).hexdigest(),
                       "pixels_md5": hashlib.md5(px).hexdigest(),
                       "chroma_at_clip": int(sum((p == b).sum() for p in planes[1:] for b in rc.CHROMA_CLIP)) if colour else 0})
    print(json.dumps({"width": w, "height": h, "color": colour, "frames": frames}))


def decode(name, magnify, fmt, smoothing):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", sc.stream_path(name), str(magnify), str(smoothing), fmt],
                       env=ENV, capture_output=True)
    if r.returncode != 0:
        how = "signal %d" % -r.returncode if r.returncode < 0 else "exit %d: %s" % (r.returncode, r.stderr.decode("latin-1").strip().split("\n")[-1][:120])
        return {"died": how}
    return json.loads(r.stdout.decode().strip().split("\n")[-1])


def make_streams(tmp, exe):
    def write(name, data):
        open(sc.stream_path(name), "wb").write(data)

    g256 = conftest.Inputs(json.load(open(os.path.join(HERE, "MANIFEST.json"))), tmp).data("g256")
    err, stream, _ = rc.run_reference(rc.CFIASCO, [g256], ["--basis-name", "long_a.fco"], os.path.join(tmp, "longa"), dump=False)
    assert err is None, err
    write("st_longa_g256", stream)
    err, stream, _ = rc.run_reference(rc.CFIASCO, tinted(5, 64, 64, 11), ["--pattern", "ipbbp", "-q", "40"], os.path.join(tmp, "ipbbp"), dump=False)
    assert err is None, err
    write(sc.IPBBP, stream)
    err, stream, _ = vc.run_reference_library(tinted(4, 70, 66, 7), ["--pattern", "ibbp"], (25, 1, 0), os.path.join(tmp, "ibbp_b0"), dump=False)
    assert err is None, err
    write(sc.IBBP_B0, stream)
    err, stream, _ = rc.run_reference(rc.CFIASCO, rc._saturated(), ["-q", "60", "--pattern", "ibp"], os.path.join(tmp, "sat"), dump=False)
    assert err is None, err
    write(sc.SATURATED, stream)
    # blocks that leave the frame on the right: one per block type and P/B frame of the ragged video, moved by hand
    print(subprocess.check_output([exe, "wrap", sc.stream_path(sc.IBBP_B0), sc.stream_path(sc.WRAPPED)], env=ENV).decode().strip())
    # the orphaned B frames
    frames = rc._shift(4)
    e1, ibbp, _ = rc.run_reference(rc.CFIASCO, frames, ["--pattern", "ibbp"], os.path.join(tmp, "o_ibbp"), dump=False)
    e2, iiii, _ = rc.run_reference(rc.CFIASCO, frames, ["--pattern", "iiii"], os.path.join(tmp, "o_iiii"), dump=False)
    assert e1 is None and e2 is None, (e1, e2)

    def offsets(data, label):
        p = os.path.join(tmp, label + ".fco")
        open(p, "wb").write(data)
        lines = [ln.split() for ln in subprocess.check_output([exe, "offsets", p], env=ENV).decode().split("\n") if ln and not ln.startswith("mv")]
        return [int(f[0]) for f in lines], [(int(f[1]), int(f[2])) for f in lines[:-1]]
    oa, fa = offsets(ibbp, "a")
    ob, fb = offsets(iiii, "b")
    assert fa == [(0, 0), (3, 1), (1, 2), (2, 2)] and fb == [(k, 0) for k in range(4)], (fa, fb)
    assert ibbp[:oa[0]] == iiii[:ob[0]], "the headers differ"
    write(sc.ORPHAN, ibbp[:oa[1]] + iiii[ob[3]:ob[4]] + ibbp[oa[2]:])


def blocks_of(exe, name):
    """[(display, x, y, level, type, fx, fy, bx, by)] of a stream, from the reader (tests/stream_check.c offsets)"""
    text = subprocess.check_output([exe, "offsets", sc.stream_path(name)], env=ENV).decode()
    return [tuple(int(v) for v in ln.split()[1:]) for ln in text.split("\n") if ln.startswith("mv")]


def main():
    import fiasco_amd
    import test_stream_check
    tmp = tempfile.mkdtemp(prefix="fiasco_decoded_streams_")
    exe = test_stream_check.build(tmp)
    make_streams(tmp, exe)
    ora = fiasco_amd.Library(conftest.ORACLE_LIB)            # host code only: the size rule
    product = fiasco_amd.Library(fiasco_amd.LIB_PATH)        # host code only: the reader, for the header's smoothing
    product.set_verbosity(0)
    out, left_out = {}, {}
    accepted = {-1: [], 1: []}
    clipped = 0
    for name in sc.NAMES:
        data = sc.stream_bytes(name)
        base = decode(name, 0, "444", 0)
        assert "frames" in base, (name, base)
        colour = base["color"]
        offs = subprocess.check_output([exe, "offsets", sc.stream_path(name)], env=ENV).decode().split("\n")
        types = {int(f[1]): int(f[2]) for f in (ln.split() for ln in offs if ln and not ln.startswith("mv") and "end" not in ln)}
        rec = {"md5": hashlib.md5(data).hexdigest(), "width": base["width"], "height": base["height"], "color": bool(colour),
               "frame_types": [types[d] for d in sorted(types)], "decoded": {}}
        for m in sc.MAGNIFY:
            for fmt in (["444", "420"] if colour else ["444"]):
                for s in sc.SMOOTHING:
                    key = sc.key_of(m, fmt, s)
                    got = decode(name, m, fmt, s)
                    if "died" in got:
                        left_out["%s %s" % (name, key)] = got["died"]
                        continue
                    if "refused" in got:
                        rec["decoded"][key] = {"refused": got["refused"]}
                        continue
                    try:
                        assert (got["width"], got["height"]) == tuple(fiasco_amd.magnified_size(ora, base["width"], base["height"], m)), (name, key)
                    except fiasco_amd.FiascoError:
                        raise AssertionError((name, key, "the reference decodes what the size rule refuses"))
                    if any(t for t in rec["frame_types"]):
                        if m in accepted:
                            accepted[m].append(name)
                        clipped += sum(f["chroma_at_clip"] for d, f in enumerate(got["frames"]) if rec["frame_types"][d])
                    rec["decoded"][key] = {"width": got["width"], "height": got["height"],
                                           "frames": [{"type": rec["frame_types"][d], "planes_md5": f["planes_md5"], "pixels_md5": f["pixels_md5"]}
                                                      for d, f in enumerate(got["frames"])]}
        # the header's percentage (the product's reader, host code): what smoothing -1 stands for
        s = fiasco_amd.Stream(product, data)
        rec["smoothing"] = s.info["smoothing"]
        s.free()
        out[name] = rec
        print("%-26s %s %d tuples" % (name, "".join("IPB"[t] for t in rec["frame_types"]), len(rec["decoded"])))
    assert accepted[-1] and accepted[1], accepted
    assert clipped > 0, "no chroma sample of a P or B frame at a clip bound"
    # the vectors the 4:2:0 path halves toward zero, and a block that leaves the frame on the right
    odd = {1: 0, 2: 0, 3: 0}
    right = 0
    for name in sc.VIDEOS + sc.NEW:
        w = out[name]["width"]
        for d, x, y, level, t, fx, fy, bx, by in blocks_of(exe, name):
            comps = ([fx, fy] if t != 2 else []) + ([bx, by] if t != 1 else [])
            odd[t] += name in sc.NEW and any(v < 0 and v % 2 for v in comps)          # the colour videos: decoded in 4:2:0
            right += any(x + v + (1 << (level >> 1)) > w for v in ([fx] if t != 2 else []) + ([bx] if t != 1 else []))
    assert all(odd.values()), ("negative odd vector components by block type (forward, backward, interpolated)", odd)
    # No stream a coder wrote holds such a block (the reference's motion search skips the vectors, codec/mwfa.c:571-575):
    # they are those of sc.WRAPPED, which the reference's decoder takes like any other stream -- it addresses linearly
    assert right >= 3, right
    json.dump({"generator": "tests/golden/make_decoded_streams.py", "reference": "oracle/_ref/libfiasco_ref.so (oracle/ref_build.sh), driven through ctypes",
               "magnify": sc.MAGNIFY, "smoothing": sc.SMOOTHING, "streams": out, "left_out": left_out,
               "asserted": {"videos_at_-1": sorted(set(accepted[-1])), "videos_at_+1": sorted(set(accepted[1])), "chroma_at_clip_in_P_B": clipped,
                            "negative_odd_by_type": odd, "blocks_leaving_on_the_right": right}},
              open(sc.FIXTURE, "w"), indent=1)
    print("DECODED_STREAMS.json: %d bytes; left out: %s" % (os.path.getsize(sc.FIXTURE), left_out))


if __name__ == "__main__":
    if len(sys.argv) == 6 and sys.argv[1] == "--one":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] == "420")
    else:
        main()
