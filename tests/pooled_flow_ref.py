"""float64 restatement of the pooled flow-attention variants (att_source 14..17: -se_gp2x2_flow_nobottle, -se_spp21_flow,
-se_spp2_flow, -se_spp864_flow), written from the reference graph (davo.py:1088-1102 transform, 1181-1210 the branches,
1404-1442 masking; nets/attention_module.py:68-77 gp2x2, 137-167 spatial_pyramid_pool, 89-101 the dense layers) for the tests.
The checker only: the library never calls it.  Unpinned against TensorFlow.

All four are se(se_input_flows[i], "se_flow", ...): variables under pose_exp_net/se_flow, both target maps ones (use_se_flow,
davo.py:1404-1412), the flow transform applied per pixel before pooling.  The descriptor:

  gp2x2   hh = H // 2, hw = W // 2; exact means of [:hh, :hw], [:hh, hw:], [hh:, :hw], [hh:, hw:], each (x, y).  D = 8.
  spp     per level n in list order: hs = ceil(H / n), ws = ceil(W / n); tf.pad appends zeros below and right up to
          Hp = n hs, Wp = n ws (after the transform; they add 0 and count in the divisor); tf.nn.avg_pool with
          ksize [1, hs, hs, 1] - the height twice, as written - strides (hs, ws), SAME: output n x n, no row padding, columns
          max(hs - ws, 0) in total, left = total // 2, excluded from the divisor.  Cell (i, j): rows [i hs, (i + 1) hs),
          columns [j ws - left, j ws - left + hs) cut to [0, Wp); value = sum over its real pixels / (hs x its columns inside
          [0, Wp)).  Flattened level, i, j, (x, y).

`cells' is those rules; `avg_pool_same' is TF's SAME average pool stated on its own (pad, window, count the in-bounds elements),
which tests/test_pooled_flow.py holds against the cells.  Tables, packing and the network come from the oracle package's
attention_map, preprocess_image and posenet and from class_table_ref's helpers; nothing from the product but the parser."""
import math

import numpy as np

from davo_amd.version import NUM_SEG_CLASSES, att_source_id
from oracle import davo_oracle as O

import class_table_ref as C

LEVELS = {"se_gp2x2_flow_nobottle": None, "se_spp21_flow": (2, 1), "se_spp2_flow": (2,), "se_spp864_flow": (8, 6, 4)}
WIDTHS = {"se_gp2x2_flow_nobottle": (8, 19), "se_spp21_flow": (10, 8), "se_spp2_flow": (8, 8), "se_spp864_flow": (232, 8)}
SUBSTRING = {"se_gp2x2_flow_nobottle": "-se_gp2x2_flow_nobottle", "se_spp21_flow": "-se_spp21_flow",
             "se_spp2_flow": "-se_spp2_flow", "se_spp864_flow": "-se_spp864_flow"}
PARTS = ("bottleneck_fc/kernel", "bottleneck_fc/bias", "recover_fc/kernel", "recover_fc/bias")


def _clip(v, lo, hi):
    return max(lo, min(hi, v))


def level_cells(H, W, n):
    """One SPP level: [(level n, (y0, y1), (x0, x1), divisor)] in (i, j) order; the rectangle is the cell's share of the real
    image, (0, 0), (0, 0) where it has none."""
    hs, ws = math.ceil(H / n), math.ceil(W / n)
    Wp = n * ws
    left = max(hs - ws, 0) // 2
    out = []
    for i in range(n):
        for j in range(n):
            c0 = j * ws - left
            c1 = c0 + hs
            ncols = _clip(c1, 0, Wp) - _clip(c0, 0, Wp)
            y = (_clip(i * hs, 0, H), _clip((i + 1) * hs, 0, H))
            x = (_clip(c0, 0, W), _clip(c1, 0, W))
            if y[1] <= y[0] or x[1] <= x[0]:
                y, x = (0, 0), (0, 0)
            out.append((n, y, x, hs * ncols))
    return out


def cells(H, W, att_source):
    """The descriptor's cells in descriptor order: [(level or 0 for gp2x2, (y0, y1), (x0, x1), divisor)]."""
    levels = LEVELS[att_source]
    if levels is None:
        hh, hw = H // 2, W // 2
        quads = [((0, hh), (0, hw)), ((0, hh), (hw, W)), ((hh, H), (0, hw)), ((hh, H), (hw, W))]
        return [(0, y, x, (y[1] - y[0]) * (x[1] - x[0])) for y, x in quads]
    out = []
    for n in levels:
        out += level_cells(H, W, n)
    return out


def plan_arrays(H, W, att_source):
    """(rects int32 [n,4] = y0, y1, x0, x1; inv_div float32 [n]): the form davo_pool_plan returns."""
    cs = cells(H, W, att_source)
    rects = np.array([[y[0], y[1], x[0], x[1]] for _, y, x, _ in cs], np.int32).reshape(-1, 4)
    inv = np.array([np.float32(1.0) / np.float32(d) for _, _, _, d in cs], np.float32)
    return rects, inv


def outside_mask(H, W, att_source):
    """[H,W] bool: the pixels no window covers."""
    m = np.ones((H, W), bool)
    for _, y, x, _ in cells(H, W, att_source):
        m[y[0]:y[1], x[0]:x[1]] = False
    return m


def avg_pool_same(x, kh, kw, sh, sw):
    """tf.nn.avg_pool(x [H,W,C], ksize [1,kh,kw,1], strides [1,sh,sw,1], 'SAME') stated on its own: output ceil(in / stride);
    total padding max((out - 1) stride + k - in, 0), the smaller half first; a window's mean is over its in-bounds elements."""
    H, W, Cn = x.shape
    oh, ow = -(-H // sh), -(-W // sw)
    pt = max((oh - 1) * sh + kh - H, 0) // 2
    pl = max((ow - 1) * sw + kw - W, 0) // 2
    out = np.zeros((oh, ow, Cn))
    for i in range(oh):
        for j in range(ow):
            y0, y1 = max(i * sh - pt, 0), min(i * sh - pt + kh, H)
            x0, x1 = max(j * sw - pl, 0), min(j * sw - pl + kw, W)
            out[i, j] = x[y0:y1, x0:x1].sum(axis=(0, 1)) / ((y1 - y0) * (x1 - x0))
    return out


def literal_descriptor(t, att_source):
    """The descriptor of ONE transformed flow plane t [H,W,2] float64 by the reference's own steps (tf.pad, avg_pool, reshape) -
    the cross-check of `cells'."""
    H, W, _ = t.shape
    levels = LEVELS[att_source]
    if levels is None:
        hh, hw = H // 2, W // 2
        return np.concatenate([t[:hh, :hw].mean(axis=(0, 1)), t[:hh, hw:].mean(axis=(0, 1)),
                               t[hh:, :hw].mean(axis=(0, 1)), t[hh:, hw:].mean(axis=(0, 1))])
    out = []
    for n in levels:
        hs, ws = math.ceil(H / n), math.ceil(W / n)
        padded = np.pad(t, ((0, n * hs - H), (0, n * ws - W), (0, 0)))
        out.append(avg_pool_same(padded, hs, hs, hs, ws).reshape(-1))
    return np.concatenate(out)


def transformed(cfg, flow):
    """[B,2,H,W,2] float64: the SE input transform of the two source frames' flow (planes 0, 1), on the values handed in."""
    return C.se_flow_input(cfg, np.asarray(flow)[:, :2].astype(np.float64))


def descriptor(cfg, flow, dtype=np.float64):
    """[B,2,D].  dtype float64: exact sums.  dtype float32: the transform, numpy's pairwise sums and the product with the
    float32 reciprocal divisor all in float32 - the arithmetic class of a device squeeze."""
    B, _, H, W, _ = np.shape(flow)
    cs = cells(H, W, cfg.att_source)
    if dtype == np.float32:
        f = np.asarray(flow)[:, :2].astype(np.float32)
        if cfg.norm_flow:
            f = (f - np.float32(0.32140523)) / np.float32(15.384229)
        t = f.copy()
        if cfg.abs_mode in ("h", "all"):
            t[..., 0] = np.abs(f[..., 0])
        if cfg.abs_mode in ("v", "all"):
            t[..., 1] = np.abs(f[..., 1])
    else:
        t = transformed(cfg, flow)
    out = np.zeros((B, 2, 2 * len(cs)), dtype)
    for k, (_, y, x, div) in enumerate(cs):
        # the cell's pixels as the contiguous last axis: numpy adds that axis pairwise
        px = np.ascontiguousarray(np.moveaxis(t[:, :, y[0]:y[1], x[0]:x[1]], -1, 2)).reshape(B, 2, 2, -1)
        s = px.sum(axis=-1, dtype=dtype)
        out[:, :, 2 * k:2 * k + 2] = s * (np.float32(1.0) / np.float32(div)) if dtype == np.float32 else s / div
    return out


def descriptor_bar(cfg, flow):
    """[B,2,D]: the se_desc bar, 2^-20 x (sum of |t(flow)| over the cell) x inv_div per entry (the export tests' form and constant)."""
    B, _, H, W, _ = np.shape(flow)
    t = np.abs(transformed(cfg, flow))
    cs = cells(H, W, cfg.att_source)
    out = np.zeros((B, 2, 2 * len(cs)))
    for k, (_, y, x, div) in enumerate(cs):
        out[:, :, 2 * k:2 * k + 2] = t[:, :, y[0]:y[1], x[0]:x[1]].reshape(B, 2, -1, 2).sum(axis=2) / div
    return 2.0 ** -20 * out


def mlp(cfg, weights):
    p = "pose_exp_net/se_flow/"
    return tuple(np.asarray(weights[p + n], np.float64) for n in PARTS)


def tables_from_descriptor(cfg, desc, weights, dtype=np.float64):
    """[B,3,19]: the target's row is ones, rows 1, 2 = sigmoid(act(d W1 + b1) W2 + b2)."""
    w1, b1, w2, b2 = (a.astype(dtype) for a in mlp(cfg, weights))
    d = np.asarray(desc, dtype)
    tab = np.ones((d.shape[0], 3, NUM_SEG_CLASSES), dtype)
    e = O._act(cfg.se_act, d.dot(w1) + b1).astype(dtype)
    tab[:, 1:] = O._sigmoid(e.dot(w2) + b2)
    return tab


def class_tables(cfg, flow, weights):
    return tables_from_descriptor(cfg, descriptor(cfg, flow), weights)


def pack(cfg, img_u8, flow, seg, weights):
    """Masked PoseNN inputs of the two pairs [B,2,H,W,2*cin_per_frame] (davo.py:1404-1442); the target is never masked."""
    B, H, W3, _ = img_u8.shape
    W = W3 // 3
    x = O.preprocess_image(img_u8, np.float64)
    src0, tgt, src1 = x[:, :, :W], x[:, :, W:2 * W], x[:, :, 2 * W:]
    tab = class_tables(cfg, flow, weights)
    att = [O.attention_map(tab[:, 1], seg[:, 0]), O.attention_map(tab[:, 2], seg[:, 2])]
    c = cfg.cin_per_frame
    out = np.zeros((B, 2, H, W, 2 * c))
    for s, src in enumerate((src0, src1)):
        out[:, s, ..., 0:3] = tgt
        out[:, s, ..., c:c + 3] = src * att[s] if cfg.mask_rgb else src
        if cfg.use_flow_info:
            f = np.asarray(flow)[:, s].astype(np.float64)
            out[:, s, ..., c + 3:c + 5] = f * att[s] if cfg.mask_info else f
    return out


def forward(cfg, img_u8, flow, seg, weights, conv=None):
    """Poses [B,2,6].  conv=None: O.posenet in float64; else the convolutions through `conv`."""
    x = pack(cfg, img_u8, flow, seg, weights)
    B, _, H, W, Cn = x.shape
    x = x.reshape(B * 2, H, W, Cn)
    poses = O.posenet(x, weights) if conv is None else C._posenet_with(conv, x, weights)
    return np.asarray(poses).reshape(B, 2, 6)


# ---- inputs and their preconditions -----------------------------------------------------------------------------------------
def make_flow(B, H, W, first_window=0):
    """float32 [B,4,H,W,2]: the raw synthetic draw has mean |flow| near 12.5, which saturates a tanh bottleneck and hides where
    the flow sits; this one is that draw scaled by 0.02 plus smooth waves of amplitude ~1.5 that differ per window, plane and
    component, so that window means differ from cell to cell and from the global mean."""
    from davo_amd import synth
    raw = synth.make_inputs(B, H, W, first_window=first_window)[1]
    y = (np.arange(H, dtype=np.float64) / H)[:, None]
    x = (np.arange(W, dtype=np.float64) / W)[None, :]
    out = np.empty_like(raw)
    for b in range(B):
        for p in range(4):
            ph = 0.9 * (first_window + b) + 1.7 * p
            fx = 1.5 * np.sin(2 * np.pi * (1.3 * x + 0.7 * y) + ph) + 0.4
            fy = 1.5 * np.cos(2 * np.pi * (0.6 * x - 1.1 * y) + 0.5 * ph) - 0.3
            out[b, p, ..., 0] = (0.02 * raw[b, p, ..., 0] + fx).astype(np.float32)
            out[b, p, ..., 1] = (0.02 * raw[b, p, ..., 1] + fy).astype(np.float32)
    return out


def make_inputs(B, H, W, first_window=0):
    """(img, flow, seg): synth's images and label maps (with labels outside the classes), make_flow's flow."""
    from davo_amd import synth
    img, _, seg = synth.make_inputs(B, H, W, first_window=first_window)
    seg[0, 0, :3, :5] = np.nan
    seg[-1, 2, :2] = 19.0
    return img, make_flow(B, H, W, first_window), seg


def level_slices(H, W, att_source):
    """[(first cell, cells)] of each level (gp2x2: one `level' of four)."""
    levels = LEVELS[att_source]
    if levels is None:
        return [(0, 4)]
    out, at = [], 0
    for n in levels:
        out.append((at, n * n))
        at += n * n
    return out


def check_preconditions(cfg, flow, weights, table_tol, need_outside=None):
    """What every input of the GPU tests must satisfy, asserted before a device result is looked at (and by the CPU tests on the
    same inputs): with the pooled descriptor replaced by the broadcast global mean, and with two cells of one level swapped, the
    float64 table moves by more than 100 table_tol - the table tells where the flow sits.  need_outside: True asserts that
    pixels outside every window exist (None: reported only).  -> dict of the figures."""
    B, _, H, W, _ = np.shape(flow)
    d = descriptor(cfg, flow)
    tab = tables_from_descriptor(cfg, d, weights)
    t = transformed(cfg, flow)
    glob = np.tile(t.mean(axis=(2, 3)), (1, 1, d.shape[2] // 2))
    moved_global = np.abs(tables_from_descriptor(cfg, glob, weights) - tab)[:, 1:].max(axis=(1, 2)).min()      # every window
    first, count = level_slices(H, W, cfg.att_source)[0]
    dc = d.reshape(B, 2, -1, 2)[:, :, first:first + count]
    moved_swap = np.inf
    for b in range(B):                                        # per window: the two cells of the first level that differ most (source 0)
        diff = np.abs(dc[b, 0][:, None] - dc[b, 0][None]).sum(-1)
        i, j = np.unravel_index(int(np.argmax(diff)), diff.shape)
        sw = d[b:b + 1].copy().reshape(1, 2, -1, 2)
        sw[:, :, [first + i, first + j]] = sw[:, :, [first + j, first + i]]
        m = np.abs(tables_from_descriptor(cfg, sw.reshape(1, 2, -1), weights) - tab[b:b + 1])[:, 1:].max()
        moved_swap = min(moved_swap, m)
    outside = int(outside_mask(H, W, cfg.att_source).sum())
    figures = {"moved_global": float(moved_global), "moved_swap": float(moved_swap), "outside": outside, "bar": 100 * table_tol}
    assert moved_global > 100 * table_tol, figures
    assert moved_swap > 100 * table_tol, figures
    if need_outside:
        assert outside > 0, figures
    return figures


def version(att_source, masking="-segmask_all", act="-fc_tanh", transform="-abs_flow"):
    return "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128" + masking + SUBSTRING[att_source] + transform + act


assert all(att_source_id(k) == 14 + i for i, k in enumerate(LEVELS))
