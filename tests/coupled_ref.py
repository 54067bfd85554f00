"""float64 restatement of the coupled shared PoseNN (`-sharedNN-dilatedCouplePoseNN': couple_sharednet_v0_dilation), written from
the reference graph (davo.py:1027-1049, 1404-1450, 1456-1457; nets/posenn.py:133-187) for the tests.  The checker only: the library
never calls it.  Unpinned against TensorFlow.

Per pair image concat(tgt, src) the network is the pair network's trunk cnv1..cnv5 (nets/posenn.py:155-159), then under the scope
pose/ ONE cnv6 (3x3, rate 2, 256 -> cnv6_out, ReLU), ONE cnv7 (3x3, stride 2, cnv6_out -> 256, ReLU: it reads all of cnv6) and a
linear 1x1 pred of six columns (:176-178); pose_final = 0.01 * reshape(mean_{h,w}(pred), [-1, 1, 6]) (:179-181): the six columns are
the pose of that pair, unpermuted.  The two calls of a window (davo.py:1456-1457) fill its two rows.

The masked inputs in front of cnv1 are the pair network's: the oracle package's pack_inputs, or the pack() of the restatement that
belongs to the attention source (class tables, depth sources, depth-split, pooled flow) beside this file.  Nothing from the product
but the parser's VariantConfig."""
import numpy as np

from davo_amd.version import ATT_SOURCE, POOLED_ATT_SOURCE
from oracle import davo_oracle as O

HEAD = "pose_exp_net/pose/"
PACK8 = [0, 1, 2, 5, 6, 7, 8, 9]         # the library's 8 packed channels among concat(tgt, src)'s 10 (v1): the target's two zero channels dropped


def pack(cfg, img_u8, flow, seg, weights, depth=None):
    """Masked PoseNN inputs of the two pairs [B,2,H,W,2*cin_per_frame], float64 (davo.py:1404-1442), by the attention source."""
    if cfg.att_source in POOLED_ATT_SOURCE:
        import pooled_flow_ref as P
        return P.pack(cfg, img_u8, flow, seg, weights)
    if cfg.att_source == "se_flow_depthseg_sep":
        import depthseg_attention_ref as DS
        return DS.pack(cfg, img_u8, flow, seg, depth, weights)
    if cfg.needs_depth:
        import depth_source_ref as D
        return D.pack(cfg, img_u8, flow, seg, depth, weights)
    if ATT_SOURCE[cfg.att_source] >= 4:
        import class_table_ref as R
        return R.pack(cfg, img_u8, flow, seg, weights)
    return O.pack_inputs(cfg, img_u8, flow, seg, weights, np.float64)


def _g(weights, name):
    return np.asarray(weights[name], np.float64)


def trunk(x, weights, keep=None):
    """cnv1..cnv5 (nets/posenn.py:155-159) on x [N,H,W,10|6] -> [N,h,w,256], float64."""
    h = np.asarray(x, np.float64)
    for name, stride, rate in O._TRUNK:
        h = O.conv2d_same(h, _g(weights, "pose_exp_net/%s/weights" % name), _g(weights, "pose_exp_net/%s/biases" % name), stride, rate)
        if keep is not None:
            keep[name] = h
    return h


def pose_from_cnv7(c7, weights):
    """[N,h,w,256] -> [N,6]: the six-column pred, the spatial mean, x 0.01 (nets/posenn.py:177-181), float64."""
    pred = O.conv2d_same(np.asarray(c7, np.float64), _g(weights, HEAD + "pred/weights"), _g(weights, HEAD + "pred/biases"), 1, 1, relu=False)
    return 0.01 * pred.mean(axis=(1, 2))


def head(cnv5, weights, keep=None):
    """The one head (nets/posenn.py:161-181) on cnv5 -> [N,6]."""
    c6 = O.conv2d_same(cnv5, _g(weights, HEAD + "cnv6/weights"), _g(weights, HEAD + "cnv6/biases"), 1, 2)
    c7 = O.conv2d_same(c6, _g(weights, HEAD + "cnv7/weights"), _g(weights, HEAD + "cnv7/biases"), 2, 1)
    if keep is not None:
        keep["cnv6"], keep["cnv7"] = c6, c7
    return pose_from_cnv7(c7, weights)


def forward(cfg, img_u8, flow, seg, weights, depth=None, keep=None, x=None):
    """Poses [B,2,6] in float64.  x: pack()'s tensor if the caller has it already."""
    assert cfg.heads == "coupled" and cfg.posenn == "pairs"
    if x is None:
        x = pack(cfg, img_u8, flow, seg, weights, depth)
    B, _, H, W, C = x.shape
    if keep is not None:
        keep["packed"] = x
    return head(trunk(x.reshape(2 * B, H, W, C), weights, keep), weights, keep).reshape(B, 2, 6)


def shapes(cfg, H, W):
    """{tensor: per-pair-image shape} of what debug_read returns on a coupled context."""
    up = lambda n: -(-n // 2)      # noqa: E731
    H1, W1 = up(H), up(W)
    H2, W2 = up(H1), up(W1)
    return {"packed": (H, W, 8), "cnv1": (H1, W1, 16), "cnv2": (H2, W2, 32), "cnv3": (H2, W2, 64), "cnv4": (H2, W2, 128),
            "cnv5": (H2, W2, 256), "cnv6": (H2, W2, cfg.cnv6_out if cfg is not None else 0), "cnv7": (up(H2), up(W2), 256)}


def layers(cfg, weights):
    """tests/layer_check.py's layers() for the coupled network: cnv6 one group of cnv6_out columns from all of cnv5, cnv7 one group
    of 256 columns from ALL cnv6_out channels."""
    assert cfg.cin_per_frame == 5, "the 8-channel packed layout drops the target's two flow channels"
    g = lambda n: (weights["pose_exp_net/%s/weights" % n], weights["pose_exp_net/%s/biases" % n])      # noqa: E731
    w1, b1 = g("cnv1")
    out = [("cnv1", "packed", 2, 1, [(w1[:, :, PACK8], b1, slice(None), slice(None))])]
    for name, prev, stride, rate in (("cnv2", "cnv1", 2, 1), ("cnv3", "cnv2", 1, 2), ("cnv4", "cnv3", 1, 4), ("cnv5", "cnv4", 1, 8),
                                     ("pose/cnv6", "cnv5", 1, 2), ("pose/cnv7", "cnv6", 2, 1)):
        w, b = g(name)
        out.append((name.split("/")[-1], prev, stride, rate, [(w, b, slice(None), slice(None))]))
    return out


# ---- the duplicated-head identity against the oracle's decoupled network ---------------------------------------------------------
def duplicated(cfg, weights):
    """(decoupled VariantConfig's version string, its weights): a decoupled pair network whose two heads both hold the coupled cnv6 and
    cnv7, with pred = P[:, :3] for rotation and P[:, 3:] for translation, gives the coupled poses in exact arithmetic."""
    assert cfg.heads == "coupled"
    version = cfg.version.replace("-dilatedCouplePoseNN", "-dilatedPoseNN")
    w = {n: a for n, a in weights.items() if not n.startswith(HEAD)}
    pw, pb = np.asarray(weights[HEAD + "pred/weights"]), np.asarray(weights[HEAD + "pred/biases"])
    for k, h in enumerate(("rotation", "translation")):
        p = "%s%s/" % (HEAD, h)
        for n in ("cnv6/weights", "cnv6/biases", "cnv7/weights", "cnv7/biases"):
            w[p + n] = weights[HEAD + n]
        w[p + "pred/weights"] = np.ascontiguousarray(pw[..., 3 * k:3 * k + 3])
        w[p + "pred/biases"] = np.ascontiguousarray(pb[3 * k:3 * k + 3])
    return version, w
