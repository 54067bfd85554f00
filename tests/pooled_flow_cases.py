"""The cases tests/test_pooled_flow_gpu.py runs and tests/test_pooled_flow.py checks the preconditions of: one list, so that
the CPU tests look at every input the GPU tests use."""
import numpy as np

from davo_amd import synth, parse_version

import pooled_flow_ref as R

SOURCES = list(R.LEVELS)                                  # att_source 14..17
SHAPES = [(36, 100, 3), (64, 64, 2), (20, 100, 2), (128, 416, 1)]
ACTS = ["-fc_tanh", ""]                                   # tanh, relu
MASKINGS = ["-segmask_all", "-segmask_rgb"]
MASKING_SOURCE = "se_spp864_flow"                         # the one variant that runs both maskings
ENTRY_SHAPE = (36, 100, 3)                                # entry points, one-pair batches, exports, repeats
ENTRY_SOURCES = ["se_spp864_flow", "se_gp2x2_flow_nobottle"]
# The `se_desc' bar is 2^-20 x (sum of |t(flow)| over the cell) x inv_div per entry, times the factor below where the float32
# restatement (numpy pairwise sums) keeps less than 4x margin under it: the bar is then 4x that restatement's own error.
# se_spp864_flow at 64x64 (cells of 64, 121 and 256 pixels): margin 3.55x measured by tests/test_pooled_flow.py::
# test_preconditions_and_bars_hold_on_the_gpu_tests_inputs, so 4 / 3.55 = 1.13.  Every other case keeps 4.2x or more: factor 1.
DESC_BAR_FACTOR = {("se_spp864_flow", 64, 64): 1.13}


def desc_bar_factor(src, H, W):
    return DESC_BAR_FACTOR.get((src, H, W), 1.0)


def layer_cases():
    """(att_source, masking, act, transform, H, W, B) of the layer-by-layer walk."""
    out = []
    for src in SOURCES:
        for act in ACTS:
            for H, W, B in SHAPES:
                out.append((src, "-segmask_all", act, "-abs_flow", H, W, B))
    for act in ACTS:
        for H, W, B in SHAPES:
            out.append((MASKING_SOURCE, "-segmask_rgb", act, "-abs_flow", H, W, B))
    out.append(("se_spp864_flow", "-segmask_all", "-fc_tanh", "-norm_flow", 20, 100, 2))       # a cell row wholly in padding, normalised flow
    out.append(("se_spp21_flow", "-segmask_all", "-fc_tanh", "-norm_flow-abs_flow_h", 36, 100, 3))
    return out


def case_id(case):
    src, masking, act, transform, H, W, B = case
    return "%s%s%s%s-%dx%d-B%d" % (src, masking, transform, act or "-relu", H, W, B)


_INPUTS = {}


def inputs(B, H, W, first_window=0):
    """(img, flow, seg) of a shape: computed once, handed out read-only."""
    key = (B, H, W, first_window)
    if key not in _INPUTS:
        arrs = R.make_inputs(B, H, W, first_window)
        for a in arrs:
            a.setflags(write=False)
        _INPUTS[key] = arrs
    return _INPUTS[key]


def config(case):
    src, masking, act, transform = case[:4]
    cfg = parse_version(R.version(src, masking, act, transform))
    assert cfg.att_source == src
    return cfg, synth.make_weights(cfg)


def has_outside(src, H, W):
    return bool(R.outside_mask(H, W, src).any())


def nan_outside(flow, src):
    """A copy of `flow' with NaN in every pixel (both source planes, both components) that no window covers."""
    out = np.array(flow, copy=True)
    m = R.outside_mask(flow.shape[2], flow.shape[3], src)
    out[:, :, m] = np.nan
    return out
