"""The cases tests/test_three_frame.py (conditions on the inputs, on the restatement alone) and tests/test_three_frame_gpu.py
(the library against the restatement) share, built once per process and left unchanged."""
import numpy as np

from davo_amd import synth
from davo_amd.version import parse_version

import three_frame_ref as T

BASE = "v1-decay100k-dilatedPoseNN-cnv6_128"
FLAGSHIP3 = BASE + "-segmask_all-se_flow-abs_flow-fc_tanh"                # the flagship's string without `-sharedNN'
# the six versions that must run: se_flow, no attention, the two static sources, a with-target class table, v0
VERSIONS = [FLAGSHIP3, BASE + "-no_segmask", BASE + "-segmask_all-static", BASE + "-segmask_all",
            BASE + "-segmask_all-se_rgb_to_seg-fc_tanh", "v0-dilatedPoseNN-segmask-se_flow-abs_flow-fc_tanh"]
# versions that stay rejected: an attention nobody applies, a coupled net, no PoseNN substring, -se_insert, a depth source
REJECTED = ["v1-dilatedPoseNN-se_flow", "v1-dilatedCouplePoseNN-no_segmask", "v1-no_segmask", "v1-dilatedPoseNN-no_segmask-se_insert",
            BASE + "-segmask_all-se_depth_to_seg-fc_tanh", "v1-couplePoseNN-no_segmask"]

# (H, W, B): less than one cnv1 tile in a direction (8 x 8 outputs); ragged tiles both ways (18 x 50 outputs); whole tiles
SHAPES = [(16, 16, 3), (36, 100, 2), (128, 416, 1)]
IDS = ["%dx%d-B%d" % s for s in SHAPES]
SMALL = (36, 100, 2)
FIRST_WINDOW = 5

_INPUTS = {}
_WEIGHTS = {}
_POSES = {}


def inputs(H, W, B):
    """synth.make_inputs' windows with, in every label plane of window 0, one pixel of each of the 19 classes and one of the ignore
    label 255 (flattened pixels 0..19), so that every table entry and the zero row are looked up whatever the draw."""
    key = (H, W, B)
    if key not in _INPUTS:
        img, flow, seg = synth.make_inputs(B, H, W, first_window=FIRST_WINDOW)
        seg = seg.copy()
        for p in range(3):
            flat = seg[0, p].reshape(-1)
            flat[:19] = np.arange(19, dtype=np.float32)
            flat[19] = 255.0
        for a in (img, flow, seg):
            a.setflags(write=False)
        _INPUTS[key] = (img, flow, seg)
    return _INPUTS[key]


FLOW_WEIGHT_SCALE = 2.0 ** -5


def weights(version):
    """synth.make_weights' with cnv1's kernel on the four flow channels scaled by 2^-5 (exact): the synthetic flow has a standard
    deviation of 15.4 against the rgb channels' 0.58, and at equal weights the nine rgb channels would be a hundredth of cnv1's
    sums - a library that dropped one would pass.  15.4 / 32 = 0.48 puts the flow beside them.  (tests/test_three_frame.py asserts
    that every channel shows.)"""
    if version not in _WEIGHTS:
        cfg = parse_version(version)
        w = synth.make_weights(cfg)
        if cfg.use_flow_info:
            k1 = w["pose_exp_net/cnv1/weights"].copy()
            for ch in (8, 9, 13, 14):                          # flow0, flow1 among concat(tgt, src0, src1)'s 15 channels
                k1[:, :, ch] *= np.float32(FLOW_WEIGHT_SCALE)
            w["pose_exp_net/cnv1/weights"] = k1
        _WEIGHTS[version] = w
    return _WEIGHTS[version]


def case(H, W, B, version=FLAGSHIP3):
    return parse_version(version), inputs(H, W, B), weights(version)


def reference(H, W, B, version=FLAGSHIP3):
    """float64 poses [B,2,6] of a case by the restatement, computed once."""
    key = (H, W, B, version)
    if key not in _POSES:
        cfg, inp, w = case(H, W, B, version)
        _POSES[key] = T.forward(cfg, *inp, w)
    return _POSES[key]
