// pad_classes.h — class-sorted GEMM rows for the float32 dilated 3x3 layers (cnv4, cnv5, cnv6).  Pure host code, no HIP calls.
//
// A tile of conv_igemm_f32 is 128 GEMM rows; in natural order those are a flat run of 128 output pixels, 1.23 rows of a 104-pixel
// map, so every tile sees all three column taps and (valid_filter_rows, params.h) drops a filter row only in the top and bottom
// `rate` map rows.  Every load and store of that kernel addresses one pixel's run of channels on its own, so WHICH 128 pixels form
// a tile is free: here the pixels are grouped by the set of filter taps that reach inside the image (3 row zones x 3 column zones:
// nine classes of 9, 6 or 4 real taps on the maps of the network), and a tile walks exactly the taps of its pixels.  The taps a tile
// drops are zero padding for every one of its pixels - exact zero terms of the float32 fma chains - so results do not change.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace davo {

constexpr int PAD_CLASS_BLOCKS = 8;      // images are taken in blocks of ceil(NB / 8): one block per XCD's run of tiles at whole batches

// bit ky * 3 + kx: tap (ky, kx) of a stride-1 3x3 filter with dilation `rate` lands inside the Hin x Win input for output pixel (oy, ox)
inline unsigned real_tap_mask(int oy, int ox, int Hin, int Win, int pad_t, int pad_l, int rate) {
    unsigned rows = 0, cols = 0;
    for (int k = 0; k < 3; ++k) {
        const int iy = oy - pad_t + k * rate, ix = ox - pad_l + k * rate;
        if (iy >= 0 && iy < Hin) rows |= 1u << k;
        if (ix >= 0 && ix < Win) cols |= 1u << k;
    }
    unsigned m = 0;
    for (int ky = 0; ky < 3; ++ky)
        if (rows >> ky & 1) m |= cols << (3 * ky);
    return m;
}

inline int tap_count(unsigned mask) { return __builtin_popcount(mask & 0x1ffu); }

// row_pixel[Mpad]: GEMM row -> flattened output pixel n * Hout * Wout + oy * Wout + ox (-1 behind the last pixel, up to the next
// multiple of `bm`).  Inside every block of ceil(NB / 8) consecutive images the pixels are sorted by class - descending tap count,
// ties by ascending mask - and stay in (image, oy, ox) order inside a class.
// tile_taps[mtiles]: union of the real-tap masks of a tile's rows (a tile may straddle classes, blocks or images).
// Shapes at which the sorted rows would walk no fewer taps than the natural order get the natural order (see the end) and
// false is returned: such a layer runs the kernel without tables.
inline bool pad_class_tables(int NB, int Hout, int Wout, int Hin, int Win, int pad_t, int pad_l, int rate, int bm,
                             std::vector<int32_t>* row_pixel, std::vector<uint16_t>* tile_taps) {
    const int hw = Hout * Wout;
    const long M = (long)NB * hw;
    const long mtiles = (M + bm - 1) / bm;
    row_pixel->assign((size_t)(mtiles * bm), -1);
    tile_taps->assign((size_t)mtiles, 0);
    std::vector<uint16_t> pmask(hw);
    std::vector<int> by_class[512];
    std::vector<int> classes;
    for (int oy = 0; oy < Hout; ++oy)
        for (int ox = 0; ox < Wout; ++ox) {
            const unsigned m = real_tap_mask(oy, ox, Hin, Win, pad_t, pad_l, rate);
            pmask[oy * Wout + ox] = (uint16_t)m;
            if (by_class[m].empty()) classes.push_back((int)m);
            by_class[m].push_back(oy * Wout + ox);
        }
    std::sort(classes.begin(), classes.end(), [](int a, int b) {
        const int ca = tap_count(a), cb = tap_count(b);
        return ca != cb ? ca > cb : a < b;
    });
    const int G = (NB + PAD_CLASS_BLOCKS - 1) / PAD_CLASS_BLOCKS;
    long row = 0;
    for (int n0 = 0; n0 < NB; n0 += G) {
        const int n1 = std::min(NB, n0 + G);
        for (int cls : classes)
            for (int n = n0; n < n1; ++n)
                for (int pos : by_class[cls]) {
                    (*row_pixel)[(size_t)row] = n * hw + pos;
                    (*tile_taps)[(size_t)(row / bm)] |= pmask[pos];
                    ++row;
                }
    }
    // Where few images share a block (small batches) or the classes are small against a tile, the tiles that straddle classes walk
    // the union of their classes' taps and the sort can lose more than it drops.  The natural order with its tiles' true unions is
    // the other candidate (it never walks more than valid_filter_rows keeps): the tables are whichever walks fewer taps, the
    // natural order on a tie.
    std::vector<uint16_t> flat((size_t)mtiles, 0);
    for (long m = 0; m < M; ++m) flat[(size_t)(m / bm)] |= pmask[m % hw];
    long walked_sorted = 0, walked_flat = 0;
    for (long t = 0; t < mtiles; ++t) { walked_sorted += tap_count((*tile_taps)[(size_t)t]); walked_flat += tap_count(flat[(size_t)t]); }
    if (walked_flat <= walked_sorted) {
        for (long m = 0; m < M; ++m) (*row_pixel)[(size_t)m] = (int32_t)m;
        *tile_taps = flat;
        return false;
    }
    return true;
}

// Which tile the i-th workgroup of a launch takes (ConvParams::tile_order) where the tiles walk their own taps.  The launch covers
// M tiles [mtile0, mtile0 + mtiles) x ntiles_n column tiles (tile t: M tile t / ntiles_n); a tile costs the tap count of its mask.
// xcd_remap (conv_igemm.h) gives XCD x the entries [start_x, start_x + len_x) of the table.  Class-sorted rows put a block's short
// tiles at its end and the launches of a layer cut the blocks where whole rounds of the CUs end, so contiguous runs would leave the
// XCDs with unequal work: instead the tiles of every cost - long ones first - are dealt out in natural order as eight contiguous
// pieces, one per XCD (neighbouring tiles, whose dilated taps overlap, keep sharing an L2), each next tile's piece growing on the
// XCD with the least work so far that still has room.  Inside an XCD's run the long tiles then come first.
inline void pad_class_tile_order(const uint16_t* tile_taps, int mtile0, int mtiles, int ntiles_n, std::vector<int>* order) {
    const int nt = mtiles * ntiles_n;
    order->assign((size_t)nt, 0);
    const int q = nt >> 3, r = nt & 7;
    int cap[8], start[8];
    long load[8];
    std::vector<int> runs[8];
    for (int x = 0; x < 8; ++x) {
        start[x] = x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q;
        cap[x] = q + (x < r ? 1 : 0);
        load[x] = 0;
    }
    std::vector<int> same;
    for (int want = 9; want >= 0; --want) {
        same.clear();
        for (int t = 0; t < nt; ++t)
            if (tap_count(tile_taps[mtile0 + t / ntiles_n]) == want) same.push_back(t);
        if (same.empty()) continue;
        int cnt[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (size_t i = 0; i < same.size(); ++i) {
            int best = -1;
            for (int x = 0; x < 8; ++x)
                if (cap[x] > 0 && (best < 0 || load[x] < load[best])) best = x;
            ++cnt[best]; --cap[best]; load[best] += want;
        }
        size_t i = 0;
        for (int x = 0; x < 8; ++x)
            for (int k = 0; k < cnt[x]; ++k) runs[x].push_back(same[i++]);
    }
    for (int x = 0; x < 8; ++x)
        for (size_t k = 0; k < runs[x].size(); ++k) (*order)[(size_t)start[x] + k] = runs[x][k];
}

}  // namespace davo
