"""The last step of the reference's decoder, restated in numpy: 12.4 fixed-point planes -> the bytes write_image puts
into a PGM / PPM (reference lib/image.c gray_write :450-480, color_write :534-582, init_chroma_tables :487-532).
The yardstick of tests/test_gpu_device_output.py; tests/test_device_output_api.py pins it to the reference's own
bytes (tests/golden/DECODED_RGB.json) without a GPU."""
import numpy as np

# T[v + 128] = (int) (k * v + 0.5) for v = -128 .. 127, in double, truncated toward zero (astype does that)
_V = np.arange(-128, 128, dtype=np.float64)
T_RR, T_RG, T_BG, T_BB = ((k * _V + 0.5).astype(np.int32) for k in (1.4022, -0.7145, -0.3456, 1.7710))


def rgb_of_ints(yval, cb, cr):
    """yval = (Y >> 4) + 128, cb = Cb >> 4, cr = Cr >> 4 (integer arrays of one shape) -> uint8 [..., 3]"""
    cb = np.clip(cb, -128, 127) + 128
    cr = np.clip(cr, -128, 127) + 128
    rgb = np.stack([yval + T_RR[cr], yval + T_RG[cr] + T_BG[cb], yval + T_BB[cb]], axis=-1)
    return np.clip(rgb, 0, 255).astype(np.uint8)


def pixels_of_planes(planes):
    """int16 planes H x W (gray) or 3 x H x W (Y, Cb, Cr) -> uint8 H x W or H x W x 3 (R, G, B interleaved)"""
    p = np.asarray(planes).astype(np.int32) >> 4          # arithmetic: HAVE_SIGNED_SHIFT
    if p.ndim == 2:
        return np.clip(p + 128, 0, 255).astype(np.uint8)
    return rgb_of_ints(p[0] + 128, p[1], p[2])
