"""The cases tests/test_coupled.py (the parser, the variables, conditions on the inputs, the plan table; no GPU) and
tests/test_coupled_gpu.py (the library against the restatement of tests/coupled_ref.py) share, built once per process and left
unchanged."""
import numpy as np

from davo_amd import synth
from davo_amd.version import parse_version

import coupled_ref as C
import three_frame_cases as K3

BASE = "v1-decay100k-sharedNN-dilatedCouplePoseNN-cnv6_128"
FLAGSHIP_C = BASE + "-segmask_all-se_flow-abs_flow-fc_tanh"               # the flagship's string with the coupled head
WIDTHS = (32, 64, 128, 256)
# the versions that must parse and run: se_flow, no attention, the two static sources, a with-target class table, a depth source,
# a pooled flow source, v0
VERSIONS = [FLAGSHIP_C, BASE + "-no_segmask", BASE + "-segmask_all-static", BASE + "-segmask_all",
            BASE + "-segmask_all-se_rgb_to_seg-fc_tanh", BASE + "-segmask_all-se_depth_to_seg-fc_tanh",
            BASE + "-segmask_all-se_spp21_flow-fc_tanh", "v0-sharedNN-dilatedCouplePoseNN-segmask-se_flow-abs_flow-fc_tanh"]
# (version, word of the message) of the neighbours that stay rejected
REJECTED = [(BASE + "-no_segmask-se_insert", "not supported with the coupled"), ("v1-sharedNN-dilatedCouplePoseNN-se_flow", "never read"),
            ("v1-dilatedCouplePoseNN-no_segmask", "couple_net_v0_dilation"), ("v1-sharedNN-couplePoseNN-no_segmask", "couplePoseNN")]

# (H, W, B): less than one cnv1 tile, P = H3 W3 = 4 (the tiny-map pose head); ragged tiles both ways, P = 65; P = 154 and six pair
# images = 924 rows of cnv7, so 128-row tiles straddle images and the last is cut short; whole tiles
SHAPES = [(16, 16, 3), (36, 100, 2), (52, 172, 3), (128, 416, 1)]
IDS = ["%dx%d-B%d" % s for s in SHAPES]
SMALL = (36, 100, 2)


def version(width):
    return FLAGSHIP_C.replace("-cnv6_128", "-cnv6_%d" % width)


def inputs(H, W, B):
    """tests/three_frame_cases.py's windows: every class and the ignore label 255 planted in every label plane of window 0."""
    return K3.inputs(H, W, B)


def depth_planes(H, W, B):
    return synth.make_depth(B, H, W, first_window=K3.FIRST_WINDOW)


_WEIGHTS = {}
_POSES = {}


def weights(ver):
    """synth.make_weights' with cnv1's kernel on the source's two flow channels scaled by 2^-5 (exact), as the three-frame cases
    have it: the synthetic flow's standard deviation is 15.4 against the rgb channels' 0.58."""
    if ver not in _WEIGHTS:
        cfg = parse_version(ver)
        w = synth.make_weights(cfg)
        if cfg.use_flow_info:
            k1 = w["pose_exp_net/cnv1/weights"].copy()
            for ch in (8, 9):                                   # the source's flow among concat(tgt, src)'s 10 channels
                k1[:, :, ch] *= np.float32(K3.FLOW_WEIGHT_SCALE)
            w["pose_exp_net/cnv1/weights"] = k1
        _WEIGHTS[ver] = w
    return _WEIGHTS[ver]


def case(H, W, B, ver=FLAGSHIP_C):
    return parse_version(ver), inputs(H, W, B), weights(ver)


def reference(H, W, B, ver=FLAGSHIP_C):
    """float64 poses [B,2,6] of a case by the restatement, computed once."""
    key = (H, W, B, ver)
    if key not in _POSES:
        cfg, inp, w = case(H, W, B, ver)
        _POSES[key] = C.forward(cfg, *inp, w, depth=depth_planes(H, W, B) if cfg.needs_depth else None)
    return _POSES[key]


# ---- the plan table ------------------------------------------------------------------------------------------------------
# plan.h's tile ids by (rows, columns), as davo_plan_layer reports a tile and Engine.last_plan names it
TILE_ID = {(128, 32): 0, (256, 64): 1, (256, 128): 2, (128, 256): 3, (128, 128): 4, (256, 256): 5, (208, 256): 6}
PLAN_H, PLAN_W = 128, 416
PLAN_BATCHES = range(1, 33)

# width -> [(B, cnv6's tiles, cnv7's tiles)] at 128x416: the smallest B of 1..32 at which (cnv6, cnv7) take each tuple of launches.
# cnv6 is one GEMM of M = 2 B 32 104 rows and N = width columns, cnv7 one of M = 2 B 16 52 rows and N = 256 columns, one group each.
# Width 256's cnv6 is the flagship's GEMM (256 columns, K = 2304): the forward plans it with the "wave128" scale on the efficiencies
# (plan.hip, others_scale), which moves B = 23 and 24 from the 208x256 tile davo_plan_layer names to [256x256, 256x128]; both tuples
# are listed at smaller batch sizes where the two planners agree, and ((5, 2), (4,)) at B = 23 is the forward's own.
PLAN_CASES = {
    32: [(1, (0,), (0,)), (3, (0,), (4,)), (10, (0,), (2,)), (20, (0,), (2, 0)), (30, (0,), (6,))],
    64: [(1, (0,), (0,)), (3, (0,), (4,)), (5, (1,), (4,)), (10, (0,), (2,)), (13, (1,), (2,)), (20, (1, 0), (2, 0)), (23, (1, 0), (4,)),
         (30, (1,), (6,))],
    128: [(1, (0,), (0,)), (2, (4,), (0,)), (3, (4,), (4,)), (5, (2,), (4,)), (10, (2, 0), (2,)), (12, (4,), (2,)), (15, (2,), (2,)),
          (20, (2, 0), (2, 0)), (21, (4,), (2, 0)), (30, (2, 0), (6,)), (31, (4,), (6,))],
    256: [(1, (4,), (0,)), (3, (2,), (4,)), (5, (2, 0), (4,)), (6, (4,), (4,)), (8, (6,), (4,)), (9, (5,), (4,)), (10, (5, 0), (2,)),
          (11, (5, 4), (2,)), (13, (5, 2), (2,)), (15, (6,), (2,)), (18, (5,), (2,)), (20, (5, 0), (2, 0)), (21, (5, 4), (2, 0)),
          (23, (5, 2), (4,)), (25, (5, 4), (4,)), (30, (5, 0), (6,)), (31, (5, 4), (6,))],
}
# the batch sizes of width 256 at which the forward's cnv6 plan is not davo_plan_layer's (see above): B -> davo_plan_layer's tiles
PLANNER_DIFFERS_256 = {23: (6,), 24: (6,)}

# float32 (plan_layer, plan.hip): width -> [(B, cnv6's launches, cnv7's launches)] as the N tile's columns per launch, the
# smallest B of each tuple.  Default options merge cnv6's two launches into one grid where the main tile is 128 columns
# wide ("merge_rem_f32" 1; last_plan then reports one launch of 128); cnv7 keeps its two.
F32_CASES = {
    32: [(1, (32,), (32,)), (8, (32,), (64,)), (10, (32,), (128,)), (23, (32,), (128, 32)), (28, (32,), (128, 64))],
    64: [(1, (32,), (32,)), (8, (64,), (64,)), (10, (32,), (128,)), (15, (64, 32), (128,)), (18, (64,), (128,)), (23, (64, 32), (128, 32)),
         (28, (64,), (128, 64))],
    128: [(1, (32,), (32,)), (4, (64,), (32,)), (5, (128,), (32,)), (8, (128,), (64,)), (10, (32,), (128,)), (12, (128, 32), (128,)),
          (14, (128, 64), (128,)), (15, (128,), (128,)), (20, (128, 32), (32,)), (23, (128, 32), (128, 32)), (24, (128, 64), (128, 32)),
          (25, (128,), (128, 32)), (28, (128,), (128, 64))],
    256: [(1, (32,), (32,)), (2, (64,), (32,)), (3, (128,), (32,)), (6, (128, 32), (32,)), (7, (128, 64), (32,)), (8, (128,), (64,)),
          (10, (128, 32), (128,)), (12, (128, 64), (128,)), (13, (128,), (128,)), (23, (128,), (128, 32)), (25, (128, 32), (128, 32)),
          (27, (128, 64), (128, 32)), (28, (128,), (128, 64))],
}


def gemms(width, B, H=PLAN_H, W=PLAN_W):
    """((M, N) of cnv6, (M, N) of cnv7): the maps are the input's size over 4 and over 8, rounded up (SAME padding)."""
    up = lambda n, k: -(-n // k)      # noqa: E731
    h2, w2 = up(up(H, 2), 2), up(up(W, 2), 2)
    return (2 * B * h2 * w2, parse_version(version(width)).cnv6_out), (2 * B * up(h2, 2) * up(w2, 2), 256)


def plan_case_id(width, B):
    return "cnv6_%d-B%d" % (width, B)


def plan_cases():
    return [(w,) + c for w in WIDTHS for c in PLAN_CASES[w]]
