"""float64 restatement of the depth-split flow attention (att_source 13: -se_flow_on_depthseg_seplayers), written from the
reference graph (davo.py:1088-1102 squeeze input, 1136-1155 the branch, 1404-1442 masking; nets/attention_module.py:54-103
se(..., 'gp')) for the tests.  The checker only: the library never calls it.  Unpinned against TensorFlow.

With m_f the SE-transformed flow mean of source frame f - exactly the flagship's squeeze, so the oracle's own
attention_tables evaluates it -

    t_near[f] = sigmoid(act(m_f Wn1 + bn1) Wn2 + bn2)        scope se_flow_near
    t_far [f] = sigmoid(act(m_f Wf1 + bf1) Wf2 + bf2)        scope se_flow_far
    near[f]   = float32(depth_f) < float32(thr)              strict; NaN compares false: far (tf.where, davo.py:1143)
    att[f]    = (near ? t_near[f] : t_far[f])[int(seg_f)]    0 for a label outside [0, 19)

The collection scope pose_exp_net/se_flow matches se_flow_near, se_flow_far and se_flow/depth_threshold, so use_se_flow holds
(davo.py:1404-1412): the target's map, and the second pair's target map, are ones.  The compare is the one step taken in
float32, on the values the device holds, so that no pixel sits on the other side of the threshold in the checker.

Built from the oracle package's preprocess_image, attention_tables, attention_map and posenet; nothing from the product."""
import dataclasses

import numpy as np

from oracle import davo_oracle as O

import depth_source_ref as D

FRAME_PLANE = D.FRAME_PLANE             # frames (tgt, src0, src1) in the file order src0, tgt, src1
SCOPES = ("se_flow_near", "se_flow_far")
PARTS = ("bottleneck_fc/kernel", "bottleneck_fc/bias", "recover_fc/kernel", "recover_fc/bias")
THRESHOLD = "pose_exp_net/se_flow/depth_threshold"


def flagship_cfg(cfg):
    """The -se_flow configuration of the same base string: same squeeze transform, activation and masking."""
    return dataclasses.replace(cfg, att_source="se_flow")


def flagship_weights(weights, scope):
    """`weights' with the MLP of `scope' (se_flow_near | se_flow_far) under the flagship's names, the branch's own names gone."""
    w = {k: v for k, v in weights.items() if "/se_flow" not in k}
    for part in PARTS:
        w["pose_exp_net/se_flow/" + part] = weights["pose_exp_net/%s/%s" % (scope, part)]
    return w


def with_mlps(weights, near=None, far=None, thr=None):
    """A copy of `weights' with the near / far MLP replaced by that of another scope's tensors {part: array}, or the threshold."""
    w = dict(weights)
    for scope, mlp in (("se_flow_near", near), ("se_flow_far", far)):
        if mlp is not None:
            for part in PARTS:
                w["pose_exp_net/%s/%s" % (scope, part)] = mlp[part]
    if thr is not None:
        w[THRESHOLD] = np.asarray(thr, np.float32).reshape(())
    return w


def mlp_of(weights, scope):
    return {part: weights["pose_exp_net/%s/%s" % (scope, part)] for part in PARTS}


def class_tables(cfg, flow, weights):
    """(near, far): two [B,3,19] float64 tables for the frames (tgt, src0, src1); the target's rows are ones."""
    assert cfg.att_source == "se_flow_depthseg_sep"
    f = flagship_cfg(cfg)
    return tuple(O.attention_tables(f, flow, flagship_weights(weights, scope), np.float64) for scope in SCOPES)


def near_mask(depth, thr):
    """[B,3,H,W] bool, file order: float32 compare, strict; NaN is far."""
    with np.errstate(invalid="ignore"):
        return np.asarray(depth, np.float32)[..., 0] < np.float32(thr)


def attention(cfg, flow, seg, depth, weights):
    """[3][B,H,W,1] float64 maps of the frames (tgt, src0, src1)."""
    near_t, far_t = class_tables(cfg, flow, weights)
    near = near_mask(depth, weights[THRESHOLD])
    B, _, H, W, _ = np.shape(seg)
    out = [np.ones((B, H, W, 1))]
    for frame in (1, 2):
        plane = FRAME_PLANE[frame]
        a_near = O.attention_map(near_t[:, frame], seg[:, plane])
        a_far = O.attention_map(far_t[:, frame], seg[:, plane])
        out.append(np.where(near[:, plane][..., None], a_near, a_far))
    return out


def pack(cfg, img_u8, flow, seg, depth, weights):
    """Masked PoseNN inputs of the two pairs [B,2,H,W,2*cin_per_frame] (davo.py:1404-1442); the target is never masked."""
    B, H, W3, _ = img_u8.shape
    W = W3 // 3
    x = O.preprocess_image(img_u8, np.float64)
    src0, tgt, src1 = x[:, :, :W], x[:, :, W:2 * W], x[:, :, 2 * W:]
    att = attention(cfg, flow, seg, depth, weights)[1:]
    c = cfg.cin_per_frame
    out = np.zeros((B, 2, H, W, 2 * c))
    for s, src in enumerate((src0, src1)):
        out[:, s, ..., 0:3] = tgt
        out[:, s, ..., c:c + 3] = src * att[s] if cfg.mask_rgb else src
        if cfg.use_flow_info:
            f = flow[:, s].astype(np.float64)
            out[:, s, ..., c + 3:c + 5] = f * att[s] if cfg.mask_info else f
    return out


def forward(cfg, img_u8, flow, seg, depth, weights, conv=None):
    """Poses [B,2,6].  conv=None: O.posenet in float64; else the convolutions through `conv`."""
    x = pack(cfg, img_u8, flow, seg, depth, weights)
    B, _, H, W, C = x.shape
    x = x.reshape(B * 2, H, W, C)
    poses = O.posenet(x, weights) if conv is None else D._posenet_with(conv, x, weights)
    return np.asarray(poses).reshape(B, 2, 6)


def near_shares(depth, thr):
    """[B,2]: the share of depth < thr on the two source planes (file planes 0 and 2) of every window."""
    n = near_mask(depth, thr)
    return n[:, (0, 2)].reshape(n.shape[0], 2, -1).mean(axis=2)
