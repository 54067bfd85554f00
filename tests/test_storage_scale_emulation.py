"""The f16x3 range guard's floor, derived on the CPU: the float64 oracle with every stored tensor rounded the way the f16x3
epilogues store it (layer_check.pair_store: packed at scale 2^0, cnv1..cnv5 and the two heads' cnv6 at a power-of-two scale
that puts the layer's largest value into a chosen binade).  Kernel arithmetic is not modelled (it adds ~3e-7 of the pose).

A checkpoint whose six stored layers all sit in the lowest binade the guard accepts is an ordinary one (ReLU layers are
homogeneous: rescaled weights, the same poses), and Engine.forward / DAVO.inference do not calibrate.  So the poses must
meet the pose bar (helpers.assert_pose_close) there, with margin: layer_check.GUARD_FLOOR is the lowest binade at which
they stay 8x under it at every small frame the suite runs; one binade lower (2^-7) they do not, nor at the old floor 2^-11."""
import numpy as np
import pytest

from davo_amd import synth, parse_version, FLAGSHIP_VERSION
from oracle import davo_oracle as O

import layer_check as LC
from helpers import ABS_TOL, REL_TOL

MARGIN = 8.0
OLD_FLOOR_LOG2 = -11
# (H, W, B, first_window): the frames of the issue's table, and tests/test_hip_parity.py::test_minimum_sizes
SHAPES = [(16, 16, 1, 3), (20, 48, 2, 3), (36, 100, 3, 3), (64, 96, 2, 0), (128, 416, 2, 0),
          (16, 16, 1, 0), (16, 20, 3, 0), (20, 16, 2, 0), (16, 416, 1, 0), (128, 16, 2, 0)]

_CFG = parse_version(FLAGSHIP_VERSION)
_WEIGHTS = synth.make_weights(_CFG)
_REF = {}


def _conv(x, name, stride, rate, relu=True):
    return O.conv2d_same(x, _WEIGHTS[name + "/weights"], _WEIGHTS[name + "/biases"], stride, rate, relu)


def _shift(vmax, lo_log2):
    if lo_log2 == LC.CEIL_BINADE_LOG2:
        return LC.edge_shifts({"x": vmax}, "ceiling")["x"]               # [2^15, 65504): below the clamp
    return LC.binade_shift(vmax, lo_log2)


def emulate(img, flow, seg, lo_log2):
    """Poses [B,2,6] of the oracle with every stored tensor pair-rounded, each layer's maximum in [2^lo_log2, 2^(lo_log2+1))
    (or [2^15, 65504) for lo_log2 = 15: the top binade, where the clamp never bites)."""
    packed = O.pack_inputs(_CFG, img, flow, seg, _WEIGHTS, np.float64)
    B, _, H, W, C = packed.shape
    h = LC.pair_store(packed.reshape(2 * B, H, W, C), 0)
    for name, stride, rate in O._TRUNK:
        h = _conv(h, "pose_exp_net/" + name, stride, rate)
        h = LC.pair_store(h, _shift(np.abs(h).max(), lo_log2))
    heads = ("rotation", "translation")
    c6 = [_conv(h, "pose_exp_net/pose/%s/cnv6" % k, 1, 2) for k in heads]
    s6 = _shift(max(np.abs(c).max() for c in c6), lo_log2)          # one stored tensor, one scale
    outs = []
    for k, c in zip(heads, c6):
        c7 = _conv(LC.pair_store(c, s6), "pose_exp_net/pose/%s/cnv7" % k, 2, 1)
        outs.append(_conv(c7, "pose_exp_net/pose/%s/pred" % k, 1, 1, relu=False).mean(axis=(1, 2)))
    return (0.01 * np.concatenate(outs, -1)).reshape(B, 2, 6)


def _case(H, W, B, fw):
    key = (H, W, B, fw)
    if key not in _REF:
        inputs = synth.make_inputs(B, H, W, first_window=fw)
        _REF[key] = inputs, O.forward(_CFG, *inputs, _WEIGHTS, np.float64)
    return _REF[key]


def _margin(H, W, B, fw, lo_log2):
    """-> (pose bar / max|emulated - float64 oracle|, the error)."""
    inputs, ref = _case(H, W, B, fw)
    err = float(np.abs(emulate(*inputs, lo_log2) - ref).max())
    bar = min(ABS_TOL, REL_TOL * float(np.abs(ref).max()))
    return bar / err, err


def test_emulation_without_rounding_is_the_oracle():
    """At the top binade with no rounding left to speak of the emulation is the oracle: the plumbing is right."""
    inputs, ref = _case(20, 48, 2, 3)
    got = emulate(*inputs, LC.CEIL_BINADE_LOG2)
    assert np.abs(got - ref).max() <= 1e-7 * np.abs(ref).max()


@pytest.mark.parametrize("H,W,B,fw", SHAPES)
def test_pose_bar_holds_with_every_layer_at_the_guards_floor(H, W, B, fw):
    m, err = _margin(H, W, B, fw, LC.GUARD_FLOOR_LOG2)
    assert m >= MARGIN, "%dx%d B=%d: every layer in [2^%d, 2^%d): pose err %.3g, %.1fx under the bar (want >= %g)" % (
        H, W, B, LC.GUARD_FLOOR_LOG2, LC.GUARD_FLOOR_LOG2 + 1, err, m, MARGIN)


@pytest.mark.parametrize("H,W,B,fw", SHAPES)
def test_pose_bar_holds_with_every_layer_at_the_ceiling(H, W, B, fw):
    m, err = _margin(H, W, B, fw, LC.CEIL_BINADE_LOG2)
    assert m >= MARGIN, "%dx%d B=%d: every layer in [2^15, 65504): pose err %.3g" % (H, W, B, err)


@pytest.mark.parametrize("H,W,B,fw", [(16, 16, 1, 3), (20, 48, 2, 3)])
def test_the_old_floor_misses_the_pose_bar(H, W, B, fw):
    """The test bites: at 2^-11 (the floor before) the poses are outside the bar itself, and one binade under the floor
    the 8x margin is gone."""
    assert _margin(H, W, B, fw, OLD_FLOOR_LOG2)[0] < 1.0
    assert _margin(H, W, B, fw, LC.GUARD_FLOOR_LOG2 - 1)[0] < MARGIN
