"""float64 restatement of the class-table attention sources (att_source 4..10: -se_seg_wo_tgt, -se_rgb_wo_tgt_to_seg,
-se_rgb_to_seg, -se_SegFlow_to_seg[_8][_wo_tgt]), written from the reference graph (davo.py:1274-1292, 1304-1310, 1341-1374,
1404-1442; nets/attention_module.py:9-103) for the tests.  The checker only: the library never calls it.

The oracle package's pack_inputs / c_oracle.forward know the static and se_flow sources only; this module reuses its
preprocess_image, attention_map and posenet and adds the per-frame descriptors, the two dense layers and the packing."""
import numpy as np

from davo_amd.version import NUM_SEG_CLASSES
from oracle import davo_oracle as O

FRAME_SEG_PLANE = (1, 0, 2)         # frames (tgt, src0, src1) in the seg file order src0, tgt, src1 (davo.py:998-1004)
FRAME_STRIP_SLOT = (1, 0, 2)        # ... and in the strip src0 | tgt | src1 (data_loader.py:537-557)


def label_histogram(seg_plane):
    """mean over H, W of one_hot(int32(label), 19): [B,H,W,1] -> [B,19].  Same label rule as attention_map: only finite
    values in (-1, 19) select a class (truncated); the rest are zero rows that still count in the denominator."""
    s = seg_plane[..., 0].astype(np.float64)
    inside = np.isfinite(s) & (s > -1.0) & (s < float(NUM_SEG_CLASSES))
    ids = np.where(inside, np.trunc(np.where(inside, s, 0.0)), -1).astype(np.int64)
    B = s.shape[0]
    hw = s.shape[1] * s.shape[2]
    out = np.zeros((B, NUM_SEG_CLASSES))
    for b in range(B):
        v = ids[b].ravel()
        out[b] = np.bincount(v[v >= 0], minlength=NUM_SEG_CLASSES)[:NUM_SEG_CLASSES] / hw
    return out


def se_flow_input(cfg, f):
    """The SE input transform of a flow [...,2] (davo.py:1088-1102)."""
    f = np.asarray(f, np.float64)
    if cfg.norm_flow:
        f = (f - 0.32140523) / 15.384229
    if cfg.abs_mode == "h":
        f = np.stack([np.abs(f[..., 0]), f[..., 1]], -1)
    elif cfg.abs_mode == "v":
        f = np.stack([f[..., 0], np.abs(f[..., 1])], -1)
    elif cfg.abs_mode == "all":
        f = np.abs(f)
    return f


def descriptors(cfg, img_u8, flow, seg):
    """[B,3,nin] SE descriptors of the frames (tgt, src0, src1)."""
    B, H, W3, _ = img_u8.shape
    W = W3 // 3
    x = O.preprocess_image(img_u8, np.float64)
    out = []
    for i in range(3):
        if cfg.se_scope == "se_rgb":
            k = FRAME_STRIP_SLOT[i]
            d = x[:, :, k * W:(k + 1) * W].mean(axis=(1, 2))                                  # [B,3]
        else:
            d = label_histogram(seg[:, FRAME_SEG_PLANE[i]])
            if cfg.se_scope == "se_segflow":
                f = np.zeros((B, H, W, 2)) if i == 0 else flow[:, i - 1]                      # tgt flow is zeros_like (davo.py:978)
                d = np.concatenate([d, se_flow_input(cfg, f).mean(axis=(1, 2))], -1)
        out.append(d)
    return np.stack(out, 1)


def class_tables(cfg, img_u8, flow, seg, weights):
    """[B,3,19] sigmoid class tables; a `_wo_tgt' source's target table is ones (its map is ones_like)."""
    p = "pose_exp_net/%s/" % cfg.se_scope
    w1, b1, w2, b2 = (np.asarray(weights[p + n], np.float64) for n in
                      ("bottleneck_fc/kernel", "bottleneck_fc/bias", "recover_fc/kernel", "recover_fc/bias"))
    d = descriptors(cfg, img_u8, flow, seg)
    e = O._act(cfg.se_act, d.dot(w1) + b1)
    tab = O._sigmoid(e.dot(w2) + b2)
    if not cfg.tgt_attended:
        tab[:, 0] = 1.0
    return tab


def pack(cfg, img_u8, flow, seg, weights):
    """Masked PoseNN inputs of the two pairs [B,2,H,W,2*cin_per_frame] (davo.py:1404-1442): use_se_flow is false for these
    sources, so the second pair's target map is the first's."""
    B, H, W3, _ = img_u8.shape
    W = W3 // 3
    x = O.preprocess_image(img_u8, np.float64)
    src0, tgt, src1 = x[:, :, :W], x[:, :, W:2 * W], x[:, :, 2 * W:]
    tab = class_tables(cfg, img_u8, flow, seg, weights)
    att_tgt = O.attention_map(tab[:, 0], seg[:, 1]) if cfg.tgt_attended else np.ones((B, H, W, 1))
    att = [O.attention_map(tab[:, 1], seg[:, 0]), O.attention_map(tab[:, 2], seg[:, 2])]
    c = cfg.cin_per_frame
    out = np.zeros((B, 2, H, W, 2 * c))
    for s, src in enumerate((src0, src1)):
        out[:, s, ..., 0:3] = tgt * att_tgt if cfg.mask_rgb else tgt
        out[:, s, ..., c:c + 3] = src * att[s] if cfg.mask_rgb else src
        if cfg.use_flow_info:
            f = flow[:, s].astype(np.float64)
            out[:, s, ..., c + 3:c + 5] = f * att[s] if cfg.mask_info else f
    return out


def _posenet_with(conv, x, weights):
    """O.posenet's network with another convolution (c_oracle.conv2d_same: float32, threaded) for the full-size cases."""
    h = x
    for name, stride, rate in O._TRUNK:
        h = conv(h, weights["pose_exp_net/%s/weights" % name], weights["pose_exp_net/%s/biases" % name], stride, rate)
    outs = []
    for head in ("rotation", "translation"):
        p = "pose_exp_net/pose/%s/" % head
        c6 = conv(h, weights[p + "cnv6/weights"], weights[p + "cnv6/biases"], 1, 2)
        c7 = conv(c6, weights[p + "cnv7/weights"], weights[p + "cnv7/biases"], 2, 1)
        pred = conv(c7, weights[p + "pred/weights"], weights[p + "pred/biases"], 1, 1, relu=False)
        outs.append(np.asarray(pred, np.float64).mean(axis=(1, 2)))
    return 0.01 * np.concatenate(outs, axis=-1)


def forward(cfg, img_u8, flow, seg, weights, conv=None):
    """Poses [B,2,6].  conv=None: O.posenet in float64; else the convolutions through `conv`."""
    x = pack(cfg, img_u8, flow, seg, weights)
    B, _, H, W, C = x.shape
    x = x.reshape(B * 2, H, W, C)
    poses = O.posenet(x, weights) if conv is None else _posenet_with(conv, x, weights)
    return np.asarray(poses).reshape(B, 2, 6)
