"""The cases tests/test_feature_attention.py (input conditions, on the restatement alone) and
tests/test_feature_attention_gpu.py (the library against the restatement) share, built once per process.

A case is (cfg, (img, flow, seg), weights, float64 cnv5 of the restatement).  The weights are synth.make_weights' with each
block's bottleneck kernel scaled by feature_attention_ref.sensitive_weights, so that the scales are not saturated."""
from davo_amd import synth
from davo_amd.version import parse_version

import feature_attention_ref as F

PUBLISHED = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-no_segmask-se_insert"          # doc/arch-variants.md
PLAIN = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-no_segmask"

# (H, W, B, engine max_batch, cnv6 width): 16 pixels per pair image, six images inside one tile, B below the workspace's batch;
# 225 pixels per image (odd: tiles straddle images mid-row); 3,328 pixels = 13 whole tiles per image at the small-batch plans;
# the other three cnv6 widths
SHAPES = [(16, 16, 3, 4, 128), (36, 100, 2, 2, 128), (128, 416, 1, 1, 128), (128, 416, 2, 2, 128),
          (36, 100, 2, 2, 32), (36, 100, 2, 2, 64), (36, 100, 2, 2, 256)]
IDS = ["%dx%d-B%d-cnv6_%d" % (h, w, b, c6) for h, w, b, _, c6 in SHAPES]

FIRST_WINDOW = 3
_TRUNKS = {}
_CASES = {}


def version(c6):
    return PUBLISHED.replace("-cnv6_128", "-cnv6_%d" % c6)


def inputs(B, H, W):
    img, flow, seg = synth.make_inputs(B, H, W, first_window=FIRST_WINDOW)
    return img, flow, seg


def _trunk(cfg, H, W, B, w0):
    """cnv5 of the restatement; cnv1..cnv5 have the same names, shapes and so values at every cnv6 width, and windows are
    reproducible on their own: the full-size B = 1 case is the first window of the B = 2 case (one float64 trunk for both)."""
    if (H, W, B) not in _TRUNKS:
        if (H, W, B) == (128, 416, 1):
            _TRUNKS[(H, W, B)] = _trunk(cfg, H, W, 2, w0)[:2]
        else:
            _TRUNKS[(H, W, B)] = F.trunk(cfg, *inputs(B, H, W), w0)
    return _TRUNKS[(H, W, B)]


def case(H, W, B, c6=128):
    key = (H, W, B, c6)
    if key not in _CASES:
        cfg = parse_version(version(c6))
        inp = inputs(B, H, W)
        w0 = synth.make_weights(cfg)
        cnv5 = _trunk(cfg, H, W, B, w0)
        if (H, W, B) == (128, 416, 1):             # the B = 2 case's weights: its first window's poses are this case's
            w = case(H, W, 2, c6)[2]
        else:
            w = F.sensitive_weights(cfg, w0, F.descriptors(cnv5, w0))
        _CASES[key] = (cfg, inp, w, cnv5)
    return _CASES[key]


_POSES = {}


def reference(H, W, B, c6=128, keep=None, independent=False):
    """float64 poses [B,2,6] of a case by the restatement (the literal reading's are kept: both precisions ask for them)."""
    cfg, inp, w, cnv5 = case(H, W, B, c6)
    if keep is not None or independent:
        return F.forward(cfg, *inp, w, keep=keep, independent=independent, cnv5=cnv5)
    key = (H, W, B, c6)
    if key not in _POSES:
        if (H, W, B) == (128, 416, 1):             # pair images are independent of each other: the first window of B = 2
            _POSES[key] = reference(H, W, 2, c6)[:1]
        else:
            _POSES[key] = F.forward(cfg, *inp, w, cnv5=cnv5)
    return _POSES[key]
