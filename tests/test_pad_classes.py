"""Class-sorted GEMM rows of the float32 dilated 3x3 layers (csrc/pad_classes.h through the hooks davo_pad_class_tables,
davo_pad_class_tile_order and davo_plan_layer_f32; host logic, no GPU): the row table is a permutation of the pixels, a tile's
tap mask is the union of its pixels' real taps - so no real tap is ever dropped - the walked share of the nine taps is what
enumeration gives and never above the filter-row skip of the natural order, and the tile orders leave the eight XCDs level."""
import ctypes
import functools

import numpy as np
import pytest

from davo_amd import _lib

BM = 128
MAPS = [(32, 104), (8, 104), (16, 24), (13, 43), (64, 208)]
RATES = [2, 4, 8]
COUNTS = [1, 2, 3, 9, 64]


@pytest.fixture(scope="module")
def L():
    return ctypes.CDLL(_lib.build())


def _i32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _u16(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16))


def tables(L, NB, Ho, Wo, rate):
    """(row_pixel, tile_taps) of NB images of an Ho x Wo map: stride 1, so the input is the map and SAME pads `rate` on every side"""
    M = NB * Ho * Wo
    mt = -(-M // BM)
    rows = np.full(mt * BM, -7, np.int32)
    taps = np.zeros(mt, np.uint16)
    rc = L.davo_pad_class_tables(NB, Ho, Wo, Ho, Wo, rate, rate, rate, _i32(rows), _u16(taps))
    assert rc in (0, 1)
    assert (rc == 0) == bool(np.array_equal(rows[:M], np.arange(M)))     # 0: the natural order, the layer then runs without tables
    return rows, taps


@functools.lru_cache(maxsize=None)
def pixel_masks(Ho, Wo, rate):
    """brute force, one image: bit ky * 3 + kx of [oy, ox] is set when 0 <= oy - pad_t + ky * rate < Hin and the same holds in x"""
    m = np.zeros((Ho, Wo), np.int64)
    for oy in range(Ho):
        for ox in range(Wo):
            for ky in range(3):
                for kx in range(3):
                    if 0 <= oy - rate + ky * rate < Ho and 0 <= ox - rate + kx * rate < Wo:
                        m[oy, ox] |= 1 << (ky * 3 + kx)
    return m.reshape(-1)


def popcount(a):
    a = np.asarray(a, np.int64)
    return sum((a >> b) & 1 for b in range(9))


def row_masks(rows, Ho, Wo, rate):
    """real-tap mask of every GEMM row (0 for the -1 rows), [tiles, 128]"""
    pm = pixel_masks(Ho, Wo, rate)
    return np.where(rows >= 0, pm[np.maximum(rows, 0) % (Ho * Wo)], 0).reshape(-1, BM)


def today_share(L, NB, Ho, Wo, rate):
    """share of the nine taps the natural order walks: three column taps of every filter row valid_filter_rows keeps"""
    M = NB * Ho * Wo
    ky0, nky = ctypes.c_int(), ctypes.c_int()
    kept = 0
    mt = -(-M // BM)
    for t in range(mt):
        assert L.davo_tile_filter_rows(t * BM, min(t * BM + BM, M) - 1, Ho, Wo, Ho, 1, rate, rate, ctypes.byref(ky0), ctypes.byref(nky), 0, None) == 0
        kept += 3 * nky.value
    return kept / (9.0 * mt)


def sorted_walk(Ho, Wo, rate, NB):
    """taps walked by the class-sorted order, restated: blocks of ceil(NB / 8) images, classes by (-tap count, mask), stable"""
    hw = Ho * Wo
    pm = pixel_masks(Ho, Wo, rate)
    G = -(-NB // 8)
    seq = []
    for n0 in range(0, NB, G):
        k = min(NB, n0 + G) - n0
        cls = sorted(set(pm.tolist()), key=lambda m: (-bin(m).count("1"), m))
        for c in cls:
            seq.append(np.full(k * int((pm == c).sum()), c, np.int64))
    seq = np.concatenate(seq)
    pad = (-len(seq)) % BM
    seq = np.concatenate([seq, np.zeros(pad, np.int64)]).reshape(-1, BM)
    return int(popcount(np.bitwise_or.reduce(seq, axis=1)).sum())


CASES = [(Ho, Wo, rate, NB) for (Ho, Wo) in MAPS for rate in RATES for NB in COUNTS]


@pytest.mark.parametrize("Ho,Wo,rate,NB", CASES)
def test_row_table_is_a_permutation(L, Ho, Wo, rate, NB):
    rows, _ = tables(L, NB, Ho, Wo, rate)
    M = NB * Ho * Wo
    assert np.array_equal(np.sort(rows[rows != -1]), np.arange(M))
    assert np.all(rows[:M] >= 0) and np.all(rows[M:] == -1)         # the -1 entries are the tail of the last tile, nothing else


@pytest.mark.parametrize("Ho,Wo,rate,NB", CASES)
def test_no_real_tap_is_missing_from_its_tile(L, Ho, Wo, rate, NB):
    """THE correctness condition: whatever else the masks are, every tap that lands inside the image for a pixel is walked by
    the tile that holds the pixel."""
    rows, taps = tables(L, NB, Ho, Wo, rate)
    rm = row_masks(rows, Ho, Wo, rate)
    assert not np.any(rm & ~taps.astype(np.int64)[:, None])


@pytest.mark.parametrize("Ho,Wo,rate,NB", CASES)
def test_tile_mask_is_the_union_of_its_rows(L, Ho, Wo, rate, NB):
    rows, taps = tables(L, NB, Ho, Wo, rate)
    rm = row_masks(rows, Ho, Wo, rate)
    assert np.array_equal(np.bitwise_or.reduce(rm, axis=1), taps.astype(np.int64))
    assert np.all(taps & 16)                                        # the centre tap is real everywhere: no tile has an empty walk


@pytest.mark.parametrize("Ho,Wo,rate,NB", CASES)
def test_blocks_and_class_order(L, Ho, Wo, rate, NB):
    """Blocks of ceil(NB / 8) consecutive images; inside a block descending tap count, ties by ascending mask, and (image, oy, ox)
    order - which is ascending pixel index - inside a class."""
    rows, taps = tables(L, NB, Ho, Wo, rate)
    hw = Ho * Wo
    px = rows[: NB * hw].astype(np.int64)
    if np.array_equal(px, np.arange(NB * hw)):
        # the natural order: only where the sorted rows would not walk fewer taps (checked against the sort restated here)
        assert popcount(taps).sum() <= sorted_walk(Ho, Wo, rate, NB)
        assert (Ho, Wo, NB) != (32, 104, 64)
        return
    assert popcount(taps).sum() == sorted_walk(Ho, Wo, rate, NB)
    G = -(-NB // 8)
    assert np.array_equal(px // hw // G, np.arange(NB * hw) // (G * hw))
    m = pixel_masks(Ho, Wo, rate)[px % hw]
    key = (px // hw // G) * 10**12 + (9 - popcount(m)) * 10**10 + m * 10**7      # pixel indices stay below 10^7
    full = key + px
    assert np.all(np.diff(full) > 0)


@pytest.mark.parametrize("rate,bound", [(2, 0.952), (4, 0.894), (8, 0.791)])
def test_walked_share_at_the_bench_shape(L, rate, bound):
    """(32, 104), 64 pair images: enumeration gives 0.9509 / 0.8932 / 0.7906 of the nine taps."""
    _, taps = tables(L, 64, 32, 104, rate)
    share = popcount(taps).sum() / (9.0 * len(taps))
    print("rate %d: walked share %.4f (natural order %.4f)" % (rate, share, today_share(L, 64, 32, 104, rate)))
    assert share <= bound


@pytest.mark.parametrize("Ho,Wo,rate,NB", CASES)
def test_never_walks_more_than_the_natural_order(L, Ho, Wo, rate, NB):
    _, taps = tables(L, NB, Ho, Wo, rate)
    share = popcount(taps).sum() / (9.0 * len(taps))
    assert share <= today_share(L, NB, Ho, Wo, rate) + 1e-12


def xcd_runs(nt):
    """xcd_remap (csrc/conv_igemm.h): XCD x runs the table entries [start, start + len)"""
    q, r = nt >> 3, nt & 7
    return [((x * (q + 1)) if x < r else (r * (q + 1) + (x - r) * q), q + (1 if x < r else 0)) for x in range(8)]


@pytest.mark.parametrize("layer,rate,npad", [("cnv4", 4, 128), ("cnv5", 8, 256), ("cnv6", 2, 256)])
def test_xcd_runs_are_level_at_the_bench_shape(L, layer, rate, npad):
    """B = 32 at 128x416: 64 pair images of a 32x104 map on 256 compute units.  Every launch of the layer's plan: the table is a
    permutation of the launch's tiles, every XCD's run has its long tiles first, and its summed cost (tap count of the tile's
    mask) lies within 2 % of the mean over the eight."""
    _, taps = tables(L, 64, 32, 104, rate)
    mtiles = len(taps)
    m0, ml, bn = (ctypes.c_int * 2)(), (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    n = L.davo_plan_layer_f32(mtiles, npad, 1, 256, m0, ml, bn)
    assert n in (1, 2) and sum(ml[i] for i in range(n)) == mtiles
    for i in range(n):
        ntn = npad // bn[i]
        nt = ml[i] * ntn
        order = np.full(nt, -1, np.int32)
        assert L.davo_pad_class_tile_order(_u16(taps), m0[i], ml[i], ntn, _i32(order)) == 0
        assert np.array_equal(np.sort(order), np.arange(nt))
        cost = popcount(taps[m0[i] + order // ntn])
        sums = []
        for start, ln in xcd_runs(nt):
            run = cost[start:start + ln]
            assert np.all(np.diff(run) <= 0), "long tiles first"
            sums.append(int(run.sum()))
        mean = sum(sums) / 8.0
        print("%s launch %d (%d M tiles x %d): XCD sums %s" % (layer, i, ml[i], ntn, sums))
        assert max(abs(s - mean) for s in sums) <= 0.02 * mean


@pytest.mark.parametrize("nt_m,ntn", [(1, 1), (3, 2), (7, 1), (13, 4), (14, 3)])
def test_tile_order_of_small_launches(L, nt_m, ntn):
    """fewer tiles than XCDs, ragged eighths: still a permutation"""
    _, taps = tables(L, 3, 13, 43, 4)
    assert nt_m <= len(taps)
    order = np.full(nt_m * ntn, -1, np.int32)
    assert L.davo_pad_class_tile_order(_u16(taps), len(taps) - nt_m, nt_m, ntn, _i32(order)) == 0
    assert np.array_equal(np.sort(order), np.arange(nt_m * ntn))


def test_hooks_reject_bad_arguments(L):
    rows, taps = np.zeros(BM, np.int32), np.zeros(1, np.uint16)
    assert L.davo_pad_class_tables(0, 8, 8, 8, 8, 2, 2, 2, _i32(rows), _u16(taps)) < 0
    assert L.davo_pad_class_tables(1, 8, 8, 8, 8, 2, 2, 2, None, _u16(taps)) < 0
    assert L.davo_pad_class_tile_order(_u16(taps), 0, 0, 1, _i32(rows)) < 0
    m = (ctypes.c_int * 2)()
    assert L.davo_plan_layer_f32(0, 128, 1, 256, m, m, m) < 0
