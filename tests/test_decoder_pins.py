"""Pin the oracle's DECODER (oracle/oracle_decoder.c) to the real reference's decoder over the option space, without
a GPU: for every case of tests/golden/DECODED_OPTIONS.json (tests/golden/make_decoded_options.py: the bytes
`dfiasco_ref -s 0 -o` wrote for the reference's own option, model, -z 3, prediction and edge-input streams) the oracle
writes the reference's stream and decodes the reference's pixels; and a differential fuzz against the live dfiasco_ref
(tests/decoder_cases.py, whose docstring holds the seed and the oracle's tally).  The device decoder meets the same
fixture and the same seeds in tests/test_gpu_decoder_options.py, and is compared band by band with this oracle there:
that comparison is worth what these tests make of the oracle.  Every comparison is byte equality."""
import ctypes
import hashlib
import os

import pytest

import decoder_cases as dc
from conftest import REF_SHARE

HAVE_SHARE = os.path.exists(os.path.join(REF_SHARE, "medium.fco"))
RECORDS = dc.fixture()


NAMES = dc.names()


def test_fixture_covers_the_selection(manifest):
    """every selected case of the manifest and every synthetic one is recorded, nothing else; the option space the
    issue names is in it; at least three quarters of the colour cases stay in the CPU check below"""
    want = [c["name"] for c, _ in dc.manifest_cases(manifest)] + [n for n, _, _ in dc.SYNTH_CASES]
    assert sorted(want) == sorted(RECORDS) and len(want) == len(set(want)) and len(want) >= 80
    args = {c["name"]: c["args"] for c, _ in dc.manifest_cases(manifest)}
    for opt in ("--basis-name", "--prediction", "--min-level", "--rpf-mantissa", "--rpf-range", "--dictionary-size",
                "--tiling-exponent", "--chroma-dictionary"):
        assert any(opt in a for a in args.values()), opt
    assert sum(1 for c, _ in dc.manifest_cases(manifest) if c.get("models")) >= 30
    colour = [rec for rec in RECORDS.values() if rec["bands"] == 3]
    assert len(colour) >= 20 and all("y_clipped" in rec for rec in colour)
    assert 4 * sum(1 for rec in colour if not rec["y_clipped"]) >= 3 * len(colour)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_decodes_the_references_bytes(oracle, manifest, inputs, name):
    rec = RECORDS[name]
    data, args, models, md5 = dc.case_of(manifest, inputs, name, rec)
    geom = (rec["width"], rec["height"], rec["bands"])
    b, o = dc.staged(oracle, data, args, models)
    try:
        out = b.encode()
        assert out[0] is not None and hashlib.md5(out[0]).hexdigest() == md5, (name, oracle.error_message())
        pix, clipped = dc.pixels_of_bands(dc.bands_of(b, 0, geom), geom)
    finally:
        b.free(); o.delete()
    if rec["bands"] == 3:
        assert clipped == rec["y_clipped"], name
        if clipped:
            return                      # Y cannot be recovered from its clipped byte: the device test compares RGB in full
    assert hashlib.md5(pix).hexdigest() == rec["decoded_md5"], name


class _Wfa(ctypes.Structure):
    """the head of struct fa_wfa (fiasco_amd/csrc/host/fa_host.h), up to the edge lists.  A change of that struct
    shows in longest_row(): small.fco and long_b.fco must give at most 6 and large.fco more, which a shifted `into'
    does not"""
    _fields_ = [("cap", ctypes.c_uint), ("states", ctypes.c_uint), ("basis_states", ctypes.c_uint), ("root_state", ctypes.c_uint),
                ("frame_type", ctypes.c_int), ("final_distribution", ctypes.c_void_p), ("level_of_state", ctypes.c_void_p),
                ("domain_type", ctypes.c_void_p), ("delta_state", ctypes.c_void_p), ("tree", ctypes.c_void_p),
                ("x", ctypes.c_void_p), ("y", ctypes.c_void_p), ("into", ctypes.POINTER(ctypes.c_int16))]


def longest_row(oracle, basis):
    """the longest (state, label) edge list of an initial basis as the coder's loader holds it.  Rows are 6 entries
    apart and a list of 6 or more runs on INTO the next rows on purpose (fa_wfa_append_edge; the reference's
    append_edge does the same): each row is walked from its start to the first NO_EDGE, across row ends, exactly as
    dec_prepare counts them in frame_decoder.inc"""
    L = oracle.L
    L.fa_wfa_alloc.restype = ctypes.POINTER(_Wfa)
    L.fa_wfa_alloc.argtypes = [ctypes.c_uint]
    L.fa_load_basis.argtypes = [ctypes.c_char_p, ctypes.POINTER(_Wfa)]
    L.fa_wfa_free.argtypes = [ctypes.POINTER(_Wfa)]
    w = L.fa_wfa_alloc(400)
    try:
        assert L.fa_load_basis(basis.encode(), w) == 1, oracle.error_message()
        best = 0
        for row in range(w.contents.basis_states * 2):
            n = 0
            while w.contents.into[row * 6 + n] != -1:
                n += 1
            best = max(best, n)
        return best
    finally:
        L.fa_wfa_free(w)


def test_the_named_bases_have_edge_lists_of_more_than_six_entries(oracle):
    """Not hollow: the --basis-name cases of the fixture do reach the decoders' long-list paths (the device's `n > 6`
    rows behind the nodes).  A stream names its basis and does not carry it, so there is nothing to read back from a
    stream: the rows are counted where both decoders get them, in the automaton the loader builds."""
    assert longest_row(oracle, "small.fco") <= 6 and longest_row(oracle, "long_b.fco") <= 6      # (make_basis.py: by design)
    for basis in ["long_a.fco", "long_c.fco"] + (["medium.fco", "large.fco"] if HAVE_SHARE else []):
        assert longest_row(oracle, basis) > 6, basis


# ------------------------------------------------------------------ differential fuzz against the live dfiasco_ref

@pytest.mark.parametrize("group", range(dc.GROUPS))
def test_oracle_decoder_equals_dfiasco_on_random_cases(oracle, tmp_path, group):
    """one seed alone: see the docstring of tests/decoder_cases.py"""
    if not os.path.exists(dc.DFIASCO):
        pytest.skip("the reference's binaries are not built here (oracle/ref_build.sh builds them in the build container)")
    assert dc.fuzz_group("oracle", dc.oracle_codec(oracle), group, tmp_path) >= 4


@pytest.mark.parametrize("seed", dc.PINNED_SATURATED)
def test_oracle_decoder_on_the_seed_that_leaves_the_references_clipping_table(oracle, tmp_path, seed):
    """5055, found while the base seed was chosen (docstring of tests/decoder_cases.py): no prediction, large.fco, a
    0 / 255 checker board at -q 2.  dfiasco_ref's bytes, except where this decoder's byte is saturated and the
    reference indexes its clipping table out of bounds; at most 1 % of the bytes may differ at all (an overshoot of
    more than 256 gray levels beyond black or white is ringing at a few edges, not a picture)."""
    if not os.path.exists(dc.DFIASCO):
        pytest.skip("the reference's binaries are not built here (oracle/ref_build.sh builds them in the build container)")
    what, text = dc.fuzz_one(dc.oracle_codec(oracle), seed, tmp_path, saturated_only=True)
    assert what == "compared", text


def test_oracle_fuzz_compares_enough_cases(oracle, tmp_path):
    if not os.path.exists(dc.DFIASCO):
        pytest.skip("the reference's binaries are not built here (oracle/ref_build.sh builds them in the build container)")
    total = sum(dc.fuzz_group("oracle", dc.oracle_codec(oracle), g, tmp_path) for g in range(dc.GROUPS))
    print("fuzz oracle: %d of %d compared" % (total, dc.GROUPS * dc.PER_GROUP))
    assert total >= 18
