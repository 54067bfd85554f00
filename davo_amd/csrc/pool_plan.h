// pool_plan.h — the pooled flow-attention variants' window geometry (att_source 14..17, params.h): pure host logic, no HIP, in the
// manner of frame_plan (window_gather.h).  (H, W, att_source) -> the descriptor's cells in descriptor order, and the squeeze's
// work items (se_pool.h).  davo_pool_plan (include/davo_hip.h) exports the cells.
//
// gp2x2 (nets/attention_module.py:68-77): hh = H / 2, hw = W / 2; the quadrants [:hh | hh:] x [:hw | hw:] in the order TL, TR, BL,
//   BR, each an exact mean over its own pixels.
// spp, per level n of the variant's list (nets/attention_module.py:137-167, tf.nn.avg_pool SAME):
//   hs = ceil(H / n), ws = ceil(W / n); tf.pad appends zeros below and right up to Hp = n hs, Wp = n ws (they add nothing to a
//   sum and count in the divisor); avg_pool takes ksize [1, hs, hs, 1] - the height twice, as the reference writes it - at
//   strides (hs, ws).  On Hp x Wp the output is n x n, rows need no SAME padding, columns max(hs - ws, 0) in total, left = total / 2,
//   and SAME padding is excluded from the divisor.  Cell (i, j): rows [i hs, (i + 1) hs), columns [j ws - left, j ws - left + hs)
//   cut to [0, Wp); value = (sum over its real pixels) / (hs x its columns inside [0, Wp)).  tf.reshape: level, i, j, (x, y).
// A cell's rectangle here is cut to the real image [0, H) x [0, W); one that lies wholly in tf.pad's zeros is empty (its descriptor
// entries are exactly 0).
#pragma once
#include <vector>

#include "params.h"

namespace davo {

struct PoolCell {
    int y0, y1, x0, x1;       // rows [y0, y1), columns [x0, x1) of the real image; empty where y1 <= y0 or x1 <= x0
    float inv_div;            // 1 / divisor
};
// One workgroup's share of the squeeze: a cell, or a slab of whole rows of a cell of more than POOL_SLAB_PIXELS pixels (so that
// gp2x2's four quadrants are not the whole grid at B = 1).  A cell's items are consecutive and in row order.
struct PoolItem { int y0, y1, x0, x1; };
constexpr int POOL_SLAB_PIXELS = 4096;

struct PoolPlan {
    std::vector<PoolCell> cells;          // descriptor entries 2 i, 2 i + 1 belong to cells[i]
    std::vector<PoolItem> items;
    std::vector<int> cell_first;          // cells.size() + 1 entries: cell i owns items [cell_first[i], cell_first[i + 1])
};

// the SPP levels of a pooled source, in list order; 0 levels = gp2x2 (or a source that does not pool)
inline int pool_levels(int att_source, int lv[3]) {
    switch (att_source) {
        case ATT_POOL_SPP21: lv[0] = 2; lv[1] = 1; return 2;
        case ATT_POOL_SPP2: lv[0] = 2; return 1;
        case ATT_POOL_SPP864: lv[0] = 8; lv[1] = 6; lv[2] = 4; return 3;
        default: return 0;
    }
}

inline PoolPlan pool_plan(int H, int W, int att_source) {
    PoolPlan p;
    if (!att_pooled(att_source) || H < 1 || W < 1) { p.cell_first.push_back(0); return p; }
    auto clamp = [](int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); };
    auto add = [&](int y0, int y1, int x0, int x1, long div) {
        PoolCell c;
        c.y0 = clamp(y0, 0, H); c.y1 = clamp(y1, 0, H);
        c.x0 = clamp(x0, 0, W); c.x1 = clamp(x1, 0, W);
        if (c.y1 <= c.y0 || c.x1 <= c.x0) c.y0 = c.y1 = c.x0 = c.x1 = 0;
        c.inv_div = 1.0f / (float)div;
        p.cells.push_back(c);
    };
    if (att_source == ATT_POOL_GP2X2) {
        const int hh = H / 2, hw = W / 2;
        add(0, hh, 0, hw, (long)hh * hw);
        add(0, hh, hw, W, (long)hh * (W - hw));
        add(hh, H, 0, hw, (long)(H - hh) * hw);
        add(hh, H, hw, W, (long)(H - hh) * (W - hw));
    } else {
        int lv[3];
        const int nl = pool_levels(att_source, lv);
        for (int l = 0; l < nl; ++l) {
            const int n = lv[l];
            const int hs = (H + n - 1) / n, ws = (W + n - 1) / n, Wp = n * ws;
            const int left = (hs > ws ? hs - ws : 0) / 2;
            for (int i = 0; i < n; ++i)
                for (int j = 0; j < n; ++j) {
                    const int c0 = j * ws - left, c1 = c0 + hs;
                    const int ncols = clamp(c1, 0, Wp) - clamp(c0, 0, Wp);      // >= 1: c0 < Wp and c1 > 0 always
                    add(i * hs, (i + 1) * hs, c0, c1, (long)hs * ncols);
                }
        }
    }
    for (const PoolCell& c : p.cells) {
        p.cell_first.push_back((int)p.items.size());
        const int w = c.x1 - c.x0, h = c.y1 - c.y0;
        if (w <= 0 || h <= 0) continue;
        int rows = h;
        if ((long)w * h > POOL_SLAB_PIXELS) { rows = POOL_SLAB_PIXELS / w; if (rows < 1) rows = 1; }
        for (int y = c.y0; y < c.y1; y += rows) p.items.push_back(PoolItem{y, y + rows < c.y1 ? y + rows : c.y1, c.x0, c.x1});
    }
    p.cell_first.push_back((int)p.items.size());
    return p;
}

}  // namespace davo
