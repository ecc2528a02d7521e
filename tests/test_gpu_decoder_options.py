"""The DEVICE decoder (fiasco_amd/csrc/hip/frame_decoder.inc) pinned to the real reference's decoder over the option
space (-m gpu): for every case of tests/golden/DECODED_OPTIONS.json the device writes the reference's stream,
Batch.decode_device() gives the bytes `dfiasco_ref -s 0 -o` wrote for it, and every band of decode_plane() is the
oracle's band (tests/test_decoder_pins.py pins the oracle's decoder to the same fixture without a GPU).  The cases
reach what default-option stills do not: edge lists of more than six entries (--basis-name: the `n > 6` branch of
dec_pixel, the table dec_prepare puts behind the nodes), states with a tree child and edges in one half
(--prediction), linear combinations at other levels (--min-level / --max-level, -z), frames whose largest linear
combination sits at a band root or the frame root (flat frames, constant chroma), mantissas 6 .. 8 and the other
ranges.  Then frames of different sizes in one flight, and the differential fuzz of tests/decoder_cases.py against
the live dfiasco_ref with the seeds the CPU file runs against the oracle.  Every comparison is byte equality."""
import hashlib
import os

import numpy as np
import pytest

if os.path.exists("/dev/kfd"):
    import torch                                    # before the product library: one HIP runtime for both

import fiasco_amd
import decoder_cases as dc
from fuzz_parity import apply

NAMES, RECORDS = dc.names(), dc.fixture()
# frames the CPU oracle needs 10 to 16 s to code (1280 x 720 colour, 512 x 384 at -z 3): the device's pixels meet the
# reference's recorded bytes here, the band-by-band comparison with the oracle is left to the smaller cases
NO_ORACLE = ["cd200_k720", "cd1000_k720", "z3_n512"]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(product):
    assert os.path.exists("/dev/kfd"), "no GPU on this box"
    return product


def packed(geom):
    w, h, bands = geom
    return torch.zeros((h, w) if bands == 1 else (h, w, 3), dtype=torch.uint8, device="cuda")


def decoded(b):
    """every frame of a finished batch through decode_device into packed tensors -> list of bytes"""
    ts = [packed(g) for g in b._geom]
    assert b.decode_device(ts) == b.n, b.lib.error_message()
    return [t.cpu().numpy().tobytes() for t in ts]


@pytest.mark.parametrize("name", NAMES)
def test_device_decodes_the_references_bytes(gpu, oracle, manifest, inputs, name):
    rec = RECORDS[name]
    data, args, models, md5 = dc.case_of(manifest, inputs, name, rec)
    geom = (rec["width"], rec["height"], rec["bands"])
    got = []
    for lib in (gpu,) if name in NO_ORACLE else (gpu, oracle):
        b, o = dc.staged(lib, data, args, models)
        try:
            out = b.encode()
            assert out[0] is not None and hashlib.md5(out[0]).hexdigest() == md5, (name, lib.error_message())
            if lib is gpu:
                assert b._geom == [geom]
                pixels = decoded(b)[0]
            got.append(dc.bands_of(b, 0, geom))
        finally:
            b.free(); o.delete()
    assert hashlib.md5(pixels).hexdigest() == rec["decoded_md5"], name
    for band, (a, c) in enumerate(zip(got[0], got[-1])):
        assert a == c, (name, band, sum(x != y for x, y in zip(a, c)))


MIXED = [("g256", (256, 256)), ("g160x120", (160, 120)), ("n128x96", (128, 96))]


@pytest.mark.parametrize("args", [["--basis-name", "medium.fco"], ["--basis-name", "long_a.fco"], [], ["--prediction"]],
                         ids=["medium", "long_a", "default", "prediction"])
def test_frames_of_different_sizes_share_a_flight(gpu, inputs, args):
    """Three frames of 256 x 256, 160 x 120 and 128 x 96 in one batch -- one flight of the decoder, whose descriptors,
    node tables and the long edge lists behind them (medium.fco, long_a.fco) are per frame -- decode to what each gives
    alone; under medium.fco the 256 x 256 one alone is the fixture's b_medium_g256.  long_a.fco as well, because with
    the oracle's edge lists cut at six entries b_longa_g256 and b_longa_g160_z1 decode wrongly and b_medium_g256 does
    not: these frames show states with long lists."""
    if dc.needs_share(args) and "b_medium_g256" not in NAMES:
        pytest.skip("the reference's medium.fco did not travel (oracle/ref_build.sh installs it in the build container)")
    frames = [inputs.data(n) for n, _ in MIXED]
    single = []
    for data in frames:
        b, o = dc.staged(gpu, data, args, None)
        assert None not in b.encode(), gpu.error_message()
        single.append(decoded(b)[0])
        b.free(); o.delete()
    if dc.needs_share(args):
        assert hashlib.md5(single[0]).hexdigest() == RECORDS["b_medium_g256"]["decoded_md5"]
    q, o = dc.options_from_args(gpu, args)
    b = fiasco_amd.Batch(gpu, frames, q, o)
    assert None not in b.encode(), gpu.error_message()
    assert b._geom == [(w, h, 1) for _, (w, h) in MIXED]
    gpu.reset_stats()
    got = decoded(b)
    st = gpu.get_stats()
    b.free(); o.delete()
    assert st.decoder_frames == 3
    for k, (g, s) in enumerate(zip(got, single)):
        assert g == s, (args, MIXED[k][0])


def test_a_long_basis_changes_what_the_decoder_reads(gpu, inputs):
    """Not hollow.  A stream names its initial basis and does not carry it, so no reader of the stream can show a
    (state, label) row of more than six edges; tests/test_decoder_pins.py counts those rows in the automaton the
    loader builds from medium.fco / large.fco / long_*.fco (up to 33 entries).  Here: the decoder's own account of
    its traffic (decoder_bytes: 2 bytes per pixel written and per (pixel, term) read) for the same frame differs
    between the built-in basis and medium.fco -- which any two automata would show: this is the fallback the stream
    format leaves, and the row count of the CPU file carries the weight.  Tried once by hand on the host decoder: with its edge loop cut at six
    entries ten --basis-name cases of the fixture decode wrongly (long_a, long_c, medium, large) and no other case."""
    if "b_medium_g256" not in NAMES:
        pytest.skip("the reference's medium.fco did not travel (oracle/ref_build.sh installs it in the build container)")
    seen = []
    for args in ([], ["--basis-name", "medium.fco"]):
        b, o = dc.staged(gpu, inputs.data("g256"), args, None)
        assert None not in b.encode(), gpu.error_message()
        gpu.reset_stats()
        decoded(b)
        st = gpu.get_stats()
        b.free(); o.delete()
        assert st.decoder_frames == 1
        seen.append(st.decoder_bytes)
    assert seen[0] != seen[1] and min(seen) > 3 * 256 * 256, seen


# ------------------------------------------------------------------ differential fuzz against the live dfiasco_ref

def device_codec(gpu, oracle):
    """the device as the library under test (decoder_cases.fuzz_one): the stream, the bytes decode_device wrote.
    A refusal is `not compared' with a "device coder" message, or where the oracle fails with the same message (the
    reference's own limits); any other failure is reported with its message and fails the seed."""
    def run(data, q, spec, geom):
        o = gpu.cli_options()
        apply(o, spec)
        b = fiasco_amd.Batch(gpu, [data], q, o)
        try:
            out = b.encode()[0]
            if out is None:
                msg = gpu.error_message()
                if "device coder" not in msg:
                    theirs = dc.oracle_codec(oracle)(data, q, spec, geom)
                    if theirs[0] is not None or theirs[2] != msg:
                        msg = "FAIL: the device says `%s', the oracle %s" % (msg, "codes it" if theirs[0] else "`%s'" % theirs[2])
                return None, None, msg
            return out, decoded(b)[0], ""
        finally:
            b.free(); o.delete()
    return run


@pytest.mark.parametrize("group", range(dc.GROUPS))
def test_device_decoder_equals_dfiasco_on_random_cases(gpu, oracle, tmp_path, group):
    """one seed alone: see the docstring of tests/decoder_cases.py (device_codec(gpu, oracle) in place of oracle_codec)"""
    if not os.path.exists(dc.DFIASCO):
        pytest.skip("the reference's binaries did not travel (oracle/ref_build.sh builds them in the build container)")
    assert dc.fuzz_group("device", device_codec(gpu, oracle), group, tmp_path) >= 4


@pytest.mark.parametrize("seed", dc.PINNED_SATURATED)
def test_device_decoder_on_the_seed_that_leaves_the_references_clipping_table(gpu, oracle, tmp_path, seed):
    """as test_decoder_pins.py's test of the same name: seed 5055, the rule and its reason are written there"""
    if not os.path.exists(dc.DFIASCO):
        pytest.skip("the reference's binaries did not travel (oracle/ref_build.sh builds them in the build container)")
    what, text = dc.fuzz_one(device_codec(gpu, oracle), seed, tmp_path, saturated_only=True)
    assert what == "compared", text


def test_device_fuzz_compares_enough_cases(gpu, oracle, tmp_path):
    if not os.path.exists(dc.DFIASCO):
        pytest.skip("the reference's binaries did not travel (oracle/ref_build.sh builds them in the build container)")
    total = sum(dc.fuzz_group("device", device_codec(gpu, oracle), g, tmp_path) for g in range(dc.GROUPS))
    print("fuzz device: %d of %d compared" % (total, dc.GROUPS * dc.PER_GROUP))
    assert total >= 18
