"""Float64 restatement of the heat export (include/davo_hip.h: davo_forward_heat) IN THE REFERENCE'S ORDER
(generate_feature_map.py:204-265): resize every channel of cnv6 as tests/feature_export_ref.py does, then reduce over the
channels - np.sum(axis=-1), np.mean(axis=-1), max() of the resized block.  The library reduces first and resizes the one-channel
plane; that the two orders agree is what the tests show.  Imported by tests/test_heat_export.py (its own properties, CPU) and
tests/test_heat_export_gpu.py (the library against it); the library never calls it.

Also here: the index-image expression of the reference's color_map (:208-214), and float32 stand-ins for the device's arithmetic
- the fixed pairwise channel sum and TF's float32 lerp - with which the CPU tests show that the bar the GPU test holds the device
to is one the reference's order itself meets."""
import numpy as np

import feature_export_ref as FR

# |got - ref| <= BAR_REL * (largest of the output's four corner sums): at most 12 float32 roundings of 2^-24 in the channel sum
# (the library's tree is 8 deep) plus 3 in the lerp, each relative to a quantity no larger than that corner sum (cnv6 is
# non-negative, so partial sums only grow): 15 * 2^-24 < 2^-20
BAR_REL = 2.0 ** -20


def heat(cnv6, c6):
    """cnv6 [2B,h,w,2 c6] of a both-pairs forward -> {'rot', 'trans'}: (sum [B,4h,4w], mean [B,4h,4w], max [B]) in float64, the
    reduction of the RESIZED maps of the second PoseNN call (pair image 2b + 1)."""
    out = {}
    for name, resized in zip(("rot", "trans"), FR.features(cnv6, c6)):
        out[name] = (resized.sum(axis=-1), resized.mean(axis=-1), resized.max(axis=(1, 2, 3)))
    return out


def stored_heads(cnv6, c6):
    """-> {'rot', 'trans'}: the stored block [B,h,w,c6] of the second PoseNN call, in cnv6's dtype"""
    second = np.asarray(cnv6)[1::2]
    return {"rot": second[..., :c6], "trans": second[..., c6:2 * c6]}


def corner_sum_max(stored):
    """stored [B,h,w,C] -> [B,4h,4w]: the largest of the four corner channel sums (float64) of every output"""
    return FR.corner_max(np.asarray(stored, np.float64).sum(axis=-1)[..., None])[..., 0]


def index_image(feature, maximum):
    """color_map before the colour lookup (generate_feature_map.py:211-214), in the reference's float32; the library's driver
    writes zeros where the maximum is 0 (the reference divides by zero there)."""
    feature = np.asarray(feature, np.float32)
    if not np.float32(maximum) > 0:
        return np.zeros(feature.shape, np.uint8)
    feature = feature / np.float32(maximum) * 255
    return feature.astype(np.uint8)


def reference_images(resized):
    """resized [H,W,C] float32, one window's map as the reference holds it -> the four things it draws from it
    (generate_feature_map.py:249-263): (avg image, sum image)"""
    resized = np.asarray(resized, np.float32)
    total = np.sum(resized, axis=-1)
    return index_image(np.mean(resized, axis=-1), resized.max()), index_image(total, total.max())


# ---- float32 stand-ins for the device ---------------------------------------------------------------------------------
def pairwise_sum_f32(x):
    """[..., C] float32, C a power of two -> [...] float32: adjacent pairs, then adjacent pairs of those, ... - the library's
    tree ((c0 + c1) + (c2 + c3) per lane, then lane ^ 1, ^ 2, ...), log2(C) <= 8 roundings deep"""
    x = np.asarray(x, np.float32)
    assert x.shape[-1] & (x.shape[-1] - 1) == 0
    while x.shape[-1] > 1:
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def resize_x4_f32(x):
    """FR.resize_x4 in float32 and TF's order, no contraction: [N,h,w,C] float32 -> [N,4h,4w,C] float32"""
    x = np.asarray(x, np.float32)
    ylo, yhi, yl = FR._axis(x.shape[1])
    xlo, xhi, xl = FR._axis(x.shape[2])
    xl = xl.astype(np.float32)[None, None, :, None]
    yl = yl.astype(np.float32)[None, :, None, None]
    rows_t, rows_b = x[:, ylo], x[:, yhi]
    top = rows_t[:, :, xlo] + (rows_t[:, :, xhi] - rows_t[:, :, xlo]) * xl
    bot = rows_b[:, :, xlo] + (rows_b[:, :, xhi] - rows_b[:, :, xlo]) * xl
    out = top + (bot - top) * yl
    assert out.dtype == np.float32
    return out


def lerp_corners_f32(tl, tr, bl, br):
    """four float32 arrays [n] -> [n,4,4] float32: the 16 outputs (yl, xl in {0, 1/4, 1/2, 3/4}) of one input cell, TF's order"""
    tl, tr, bl, br = (np.asarray(a, np.float32)[:, None, None] for a in (tl, tr, bl, br))
    k = (np.arange(4, dtype=np.float32) * np.float32(0.25))
    xl, yl = k[None, None, :], k[None, :, None]
    top = tl + (tr - tl) * xl
    bot = bl + (br - bl) * xl
    out = top + (bot - top) * yl
    assert out.dtype == np.float32
    return out
