"""float64 restatement of the depth-source class tables (att_source 11, 12: -se_depth_wo_tgt_to_seg, -se_depth_to_seg),
written from the reference graph (davo.py:960, 991-996, 1109, 1211-1227, 1404-1442; nets/attention_module.py:54-103) for
the tests.  The checker only: the library never calls it.  Unpinned against TensorFlow.

davo.py:1109 is `se_input_depths = [d for d in pred_depths] + pred_depths[0]`: a Python list plus a tf.Tensor is not list
concatenation - list.__add__ gives up, Tensor.__radd__ packs the list into one [3,B,H,W,1] tensor and adds the target's
depth by broadcasting.  So the SE input of frame i (order tgt, src0, src1) is depth_i + depth_tgt, and the target's own
input is 2 * depth_tgt.  descriptors() below says exactly that.

Built from the oracle package's preprocess_image, attention_map and posenet; nothing from the product."""
import numpy as np

from oracle import davo_oracle as O

FRAME_PLANE = (1, 0, 2)             # frames (tgt, src0, src1) in the file order src0, tgt, src1 (davo.py:991-996, 998-1004)


def _act(name, x):
    return np.tanh(x) if name == "tanh" else np.where(x > 0, x, 0.2 * x) if name == "lrelu" else np.maximum(x, 0)


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def descriptors(cfg, depth):
    """[B,3,1]: mean over (h, w) of depth_i + depth_tgt for the frames (tgt, src0, src1) (davo.py:1109, mode 'gp')."""
    d = np.asarray(depth, np.float64)[..., 0]                       # [B,3,H,W], file order
    tgt = d[:, 1]
    return np.stack([(d[:, FRAME_PLANE[i]] + tgt).mean(axis=(1, 2)) for i in range(3)], 1)[..., None]


def class_tables(cfg, depth, weights):
    """[B,3,19] sigmoid class tables; -se_depth_wo_tgt_to_seg's target table is ones (davo.py:1219: ones_like)."""
    assert cfg.se_scope == "se_depth"
    p = "pose_exp_net/se_depth/"
    w1, b1, w2, b2 = (np.asarray(weights[p + n], np.float64) for n in
                      ("bottleneck_fc/kernel", "bottleneck_fc/bias", "recover_fc/kernel", "recover_fc/bias"))
    e = _act(cfg.se_act, descriptors(cfg, depth).dot(w1) + b1)
    tab = _sigmoid(e.dot(w2) + b2)
    if not cfg.tgt_attended:
        tab[:, 0] = 1.0
    return tab


def pack(cfg, img_u8, flow, seg, depth, weights):
    """Masked PoseNN inputs of the two pairs [B,2,H,W,2*cin_per_frame] (davo.py:1404-1442): no se_flow scope, so the
    second pair's target map is the first's."""
    B, H, W3, _ = img_u8.shape
    W = W3 // 3
    x = O.preprocess_image(img_u8, np.float64)
    src0, tgt, src1 = x[:, :, :W], x[:, :, W:2 * W], x[:, :, 2 * W:]
    tab = class_tables(cfg, depth, weights)
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
    """O.posenet's network with another convolution (a float32, threaded one for the full-size cases)."""
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


def forward(cfg, img_u8, flow, seg, depth, weights, conv=None):
    """Poses [B,2,6].  conv=None: O.posenet in float64; else the convolutions through `conv`."""
    x = pack(cfg, img_u8, flow, seg, depth, weights)
    B, _, H, W, C = x.shape
    x = x.reshape(B * 2, H, W, C)
    poses = O.posenet(x, weights) if conv is None else _posenet_with(conv, x, weights)
    return np.asarray(poses).reshape(B, 2, 6)


# ---- inputs and weights the tests share ---------------------------------------------------------------------------------
def sensitive_weights(cfg, weights, depth):
    """A copy of `weights' whose se_depth bottleneck kernel is scaled down by the batch's mean descriptor, so that the
    units' pre-activations are O(1) instead of O(descriptor): synth.make_weights draws dense kernels at sqrt(2 / fan_in),
    and with ONE input of size 10..160 every tanh unit saturates and the table stops depending on depth."""
    w = dict(weights)
    k = "pose_exp_net/se_depth/bottleneck_fc/kernel"
    w[k] = (np.asarray(weights[k], np.float64) / descriptors(cfg, depth).mean()).astype(np.float32)
    return w


def other_depth(depth):
    """A different positive field of the same range: the planes reversed along both image axes and rescaled per plane."""
    d = np.asarray(depth)[:, :, ::-1, ::-1] * np.float32(1.0)
    scale = np.array([1.7, 0.45, 1.3], np.float32).reshape(1, 3, 1, 1, 1)
    return np.ascontiguousarray(d * scale)
