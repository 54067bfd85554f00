"""float64 restatement of the feature-attention PoseNN (`-se_insert': "Ours w/ feature attention"), written from the
reference graph (davo.py:1010-1011; nets/posenn.py:219-246; nets/attention_module.py:9-52) for the tests.  The checker
only: the library never calls it.  Unpinned against TensorFlow.

nets/posenn.py:222-228 loops over the heads `rotation', `translation' and, inside the loop, RE-BINDS the loop-carried name:
    cnv5 = se_block(cnv5, 'cnv5_se_attention', ratio=8)
    cnv6 = slim.conv2d(cnv5, ...)
so the translation head's block runs on the tensor the rotation head's block has already scaled: rotation/cnv6 reads
cnv5 * s_r, translation/cnv6 reads (cnv5 * s_r) * s_t with s_t = block_t(cnv5 * s_r).  heads() below does exactly that,
literally: it re-binds and takes the mean of the scaled tensor (not s_r * mean(cnv5), which the library uses and the tests
check against this).  se_block passes no activation, so the bottleneck is ReLU whatever `-fc_*' says.

Built from the oracle package's pack_inputs and conv2d_same; nothing from the product."""
import numpy as np

from oracle import davo_oracle as O

HEADS = ("rotation", "translation")
RATIO = 8


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def block_weights(weights, head):
    p = "pose_exp_net/pose/%s/cnv5_se_attention/" % head
    return tuple(np.asarray(weights[p + n], np.float64) for n in
                 ("bottleneck_fc/kernel", "bottleneck_fc/bias", "recover_fc/kernel", "recover_fc/bias"))


def excite(d, weights, head):
    """[N,256] descriptor -> [N,256] scales: dense(256 // 8, relu), dense(256, sigmoid) (nets/attention_module.py:37-49)."""
    w1, b1, w2, b2 = block_weights(weights, head)
    return _sigmoid(np.maximum(d.dot(w1) + b1, 0.0).dot(w2) + b2)


def se_block(x, weights, head, keep=None):
    """nets/attention_module.py:9-52, mode 'gp': x [N,h,w,256] -> x * sigmoid(dense(relu(dense(mean_{h,w} x))))."""
    d = x.mean(axis=(1, 2))
    s = excite(d, weights, head)
    if keep is not None:
        keep[head + "/descriptor"], keep[head + "/scale"] = d, s
    return x * s[:, None, None, :]


def heads(cnv5, weights, keep=None, independent=False):
    """The loop of nets/posenn.py:222-246 on cnv5 [N,h,w,256] (float64) -> poses [N,6].
    independent=True is the WRONG reading (each head scales the raw cnv5), kept so the tests can show the two differ."""
    x = np.asarray(cnv5, np.float64)
    raw = x
    outs = []
    for head in HEADS:
        p = "pose_exp_net/pose/%s/" % head
        x = se_block(raw if independent else x, weights, head, keep)          # re-binds the loop-carried tensor
        c6 = O.conv2d_same(x, weights[p + "cnv6/weights"], weights[p + "cnv6/biases"], 1, 2)
        c7 = O.conv2d_same(c6, weights[p + "cnv7/weights"], weights[p + "cnv7/biases"], 2, 1)
        pred = O.conv2d_same(c7, weights[p + "pred/weights"], weights[p + "pred/biases"], 1, 1, relu=False)
        if keep is not None:
            keep[head + "/cnv6_in"], keep[head + "/cnv6"], keep[head + "/cnv7"] = x, c6, c7
        outs.append(pred.mean(axis=(1, 2)))
    return 0.01 * np.concatenate(outs, axis=-1)


def trunk(cfg, img_u8, flow, seg, weights):
    """cnv5 [2B,h,w,256] in float64 (nets/posenn.py:211-215 on the packed pairs)."""
    x = O.pack_inputs(cfg, img_u8, flow, seg, weights, np.float64)
    B, _, H, W, C = x.shape
    h = x.reshape(2 * B, H, W, C)
    for name, stride, rate in O._TRUNK:
        h = O.conv2d_same(h, weights["pose_exp_net/%s/weights" % name], weights["pose_exp_net/%s/biases" % name], stride, rate)
    return h


def forward(cfg, img_u8, flow, seg, weights, keep=None, independent=False, cnv5=None):
    """Poses [B,2,6].  cnv5: the trunk's output if the caller has it already (it does not depend on the SE weights)."""
    assert cfg.posenn_se == "insert" and cfg.att_source == "ones"
    if cnv5 is None:
        cnv5 = trunk(cfg, img_u8, flow, seg, weights)
    if keep is not None:
        keep["cnv5"] = cnv5
    return heads(cnv5, weights, keep, independent).reshape(-1, 2, 6)


def scale_table(cnv5, weights):
    """What the library's `cnv5_se_scale' holds, from a given cnv5 [N,h,w,256], by the literal reading: [N,2,256] with row 0 =
    s_r and row 1 = s_r * s_t, s_t from the mean of the scaled tensor."""
    x = np.asarray(cnv5, np.float64)
    s_r = excite(x.mean(axis=(1, 2)), weights, "rotation")
    s_t = excite((x * s_r[:, None, None, :]).mean(axis=(1, 2)), weights, "translation")
    return np.stack([s_r, s_r * s_t], axis=1)


# ---- weights the tests share ------------------------------------------------------------------------------------------
def sensitive_weights(cfg, weights, d):
    """A copy of `weights' in which each block's bottleneck kernel is divided by the mean of that block's descriptor, so that the
    units' pre-activations are O(1).  d: {head: [N,256] descriptor of that head's block} (heads(..., keep=...) gives them under
    "<head>/descriptor"; the translation block's depends on the rotation block's weights, so it is taken with the rotation
    kernel already scaled: descriptors() below).  With plain synth.make_weights at 128x416 the descriptors are O(10), the
    sigmoids saturate (scales 0.000 .. 1.000) and a wrong descriptor would not show."""
    w = dict(weights)
    for head in HEADS:
        k = "pose_exp_net/pose/%s/cnv5_se_attention/bottleneck_fc/kernel" % head
        w[k] = (np.asarray(weights[k], np.float64) / float(np.mean(d[head]))).astype(np.float32)
    return w


def descriptors(cnv5, weights):
    """{head: [N,256]} for sensitive_weights: the rotation block's descriptor, and the translation block's under the rotation
    kernel sensitive_weights will install (the rotation block's scales decide what the translation block sees)."""
    x = np.asarray(cnv5, np.float64)
    d_r = x.mean(axis=(1, 2))
    w = sensitive_weights(None, weights, {"rotation": d_r, "translation": np.ones(1)})
    s_r = excite(d_r, w, "rotation")
    return {"rotation": d_r, "translation": (x * s_r[:, None, None, :]).mean(axis=(1, 2))}


def scale_stats(table):
    """(share of s_r in (0.05, 0.95), share of s_t there, largest across-image spread of a channel's s_r, of its s_r s_t)
    of a [N,2,256] scale table."""
    s_r, s_rt = table[:, 0], table[:, 1]
    s_t = s_rt / s_r
    inside = lambda s: float(np.mean((s > 0.05) & (s < 0.95)))
    spread = lambda s: float((s.max(axis=0) - s.min(axis=0)).max())
    return inside(s_r), inside(s_t), spread(s_r), spread(s_rt)
