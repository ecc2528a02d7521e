"""numpy restatement of the measuring kernel (fiasco_amd/csrc/hip/distortion.inc), the yardstick of
tests/test_gpu_device_distortion.py; pinned to the oracle's decode_psnr without a GPU by
tests/test_device_distortion_api.py.

Both sides as the bytes psnr_of() (csrc/host/fa_batch_decode.c) and fiasco_amd_batch_decode_plane() form --
clip255((p >> 4) + 128) with an arithmetic shift on the int16 12.4 values -- then per band the exact integer sum of
the squared differences and the largest absolute difference."""
import numpy as np


def bytes_of_planes(planes):
    """int16 planes (any shape) -> the bytes the PSNR calls compare, as int64"""
    planes = np.asarray(planes)
    assert planes.dtype == np.int16
    return np.clip((planes.astype(np.int64) >> 4) + 128, 0, 255)


def distortion_of_bytes(a, c):
    """two arrays of bytes, [bands, H, W] or [H, W] -> (sse, maxdiff): three Python integers each, 0 for absent bands"""
    a, c = np.asarray(a).astype(np.int64), np.asarray(c).astype(np.int64)
    assert a.shape == c.shape and a.ndim in (2, 3)
    if a.ndim == 2:
        a, c = a[None], c[None]
    assert a.shape[0] in (1, 3)
    d = np.abs(a - c).reshape(a.shape[0], -1)
    sse = [int((d[k] * d[k]).sum()) for k in range(a.shape[0])]
    mx = [int(d[k].max()) for k in range(a.shape[0])]
    pad = [0] * (3 - a.shape[0])
    return sse + pad, mx + pad


def distortion_of_planes(orig, dec):
    """two sets of int16 planes -> (sse, maxdiff)"""
    return distortion_of_bytes(bytes_of_planes(orig), bytes_of_planes(dec))


def legacy_mse(sse, width, height):
    """what psnr_of()'s float loop gives for an exact sum below 2^24: every partial sum of the loop is an integer a
    float holds exactly, so its sum is `sse' and its mean the one float division"""
    assert 0 <= sse < 2 ** 24
    return float(np.float32(sse) / np.float32(width * height))


# the golden cases (tests/golden/MANIFEST.json) both test files stage as batches: gray frames up to 256 x 256 at the
# CLI defaults and the three colour frames of an all-intra sequence
GOLDEN_CASES = ["g64x32_q20", "g96x64_q20", "g100x70_q20", "g256_q20", "seq3_color_carry48"]


def staged_case(lib, manifest, inputs, name, stage=None):
    """the inputs of a golden case as one batch with the case's options, encoded -> (batch, options, streams).
    stage: None = from PNM; else a function (lib, list of PNM bytes, quality, options) -> Batch"""
    import fiasco_amd
    from conftest import options_from_args
    case = [c for c in manifest["cases"] if c["name"] == name][0]
    q, o = options_from_args(lib, case["args"])
    pnms = [inputs.data(n) for n in case["inputs"]]
    b = stage(lib, pnms, q, o) if stage else fiasco_amd.Batch(lib, pnms, q, o)
    return b, o, b.encode()


def reference_of_batch(b, i):
    """(sse, maxdiff) of frame i of a finished batch from the batch's own host outlets: input_planes and decode_plane"""
    w, h, bands = b._geom[i]
    orig = bytes_of_planes(b.input_planes(i))
    dec = np.stack([np.frombuffer(b.decode_plane(i, k, w, h), dtype=np.uint8).reshape(h, w) for k in range(bands)])
    return distortion_of_bytes(orig, dec)
