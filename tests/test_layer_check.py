"""The per-layer checker (tests/layer_check.py) on the CPU: float64 oracle layers at 64x96 with injected errors that the
pose bar (helpers.assert_pose_close) lets through, and the whole check_forward path on an engine stand-in that serves the
oracle's tensors."""
import numpy as np
import pytest

from davo_amd import synth, parse_version, FLAGSHIP_VERSION
from davo_amd.version import NUM_SEG_CLASSES
from oracle import davo_oracle as O

import class_table_ref as R
import layer_check as LC
from helpers import assert_pose_close

H, W, B = 64, 96, 1
SEG_WO_TGT = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all-se_seg_wo_tgt-fc_tanh"


@pytest.fixture(scope="module")
def net():
    cfg = parse_version(FLAGSHIP_VERSION)
    img, flow, seg = synth.make_inputs(B, H, W)
    weights = synth.make_weights(cfg)
    keep = {}
    pose = O.forward(cfg, img, flow, seg, weights, np.float64, keep)
    return cfg, weights, (img, flow, seg), keep, pose


def _spec(cfg, weights, name):
    return {n: (prev, stride, rate, groups) for n, prev, stride, rate, groups in LC.layers(cfg, weights)}[name]


def _flags(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


def _flags_layer(cfg, weights, keep, name, got):
    prev, stride, rate, groups = _spec(cfg, weights, name)
    return _flags(lambda: LC.check_layer(name, got, keep[prev], groups, stride, rate, LC.TAU["f16x3"][name], floor=LC.STORE_FLOOR))


def _pose_from_cnv5(cfg, weights, c5):
    _, _, _, groups = _spec(cfg, weights, "cnv6")
    c6 = np.empty(c5.shape[:3] + (2 * cfg.cnv6_out,))
    for w, b, cin, cout in groups:
        c6[..., cout] = LC.conv64(c5[..., cin], w, b, 1, 2)
    return LC.pose_from_cnv6(c6, cfg, weights).reshape(-1, 2, 6)


def test_tau_is_within_the_cap():
    assert all(t <= LC.TAU_CAP for taus in LC.TAU.values() for t in taus.values())


def test_exact_layers_pass(net):
    cfg, weights, _, keep, pose = net
    keep = dict(keep, packed=keep["packed"].reshape(2 * B, H, W, 10)[..., LC.PACK8])
    keep["cnv6"] = np.concatenate([keep["rotation/cnv6"], keep["translation/cnv6"]], -1)
    keep["cnv7"] = np.concatenate([keep["rotation/cnv7"], keep["translation/cnv7"]], -1)
    for name, prev, stride, rate, groups in LC.layers(cfg, weights):
        a, b = LC.check_layer(name, keep[name], keep[prev], groups, stride, rate, LC.TAU["f16x3"][name])
        assert a < 1e-13 and b < 1e-13, name
    np.testing.assert_allclose(LC.pose_from_cnv7(keep["cnv7"], weights).reshape(B, 2, 6), pose, rtol=1e-12, atol=0)
    np.testing.assert_allclose(LC.pose_from_cnv6(keep["cnv6"], cfg, weights).reshape(B, 2, 6), pose, rtol=1e-12, atol=0)


@pytest.mark.parametrize("case", ["pixel_1pct", "right_edge_0.1pct"])
def test_cnv5_errors_are_flagged_and_pass_the_pose_bar(net, case):
    """A wrong pixel or a wrong right-edge tile of cnv5: the layer check flags it, the pose bar does not (the pose is a
    spatial mean, which averages a local error away) - why the per-layer check exists."""
    cfg, weights, _, keep, pose = net
    bad = keep["cnv5"].copy()
    if case == "pixel_1pct":
        bad[0, 10, 13, :] *= 1.01
    else:
        bad[0, :, -4:, :] *= 1.001                          # one right-edge tile of one pair image
    assert _flags_layer(cfg, weights, keep, "cnv5", bad)
    assert_pose_close(_pose_from_cnv5(cfg, weights, bad), pose, case)


def test_missing_border_tap_is_flagged(net):
    """cnv4 (3x3, dilation 4) without one filter tap on the top row of one image: the bug of a tile that skips a filter
    row which is not all padding."""
    cfg, weights, _, keep, _ = net
    prev, stride, rate, groups = _spec(cfg, weights, "cnv4")
    w, b, _, _ = groups[0]
    w_bad = w.copy()
    w_bad[2, 0] = 0.0                                        # bottom-left tap: real input for the top row
    bad = keep["cnv4"].copy()
    bad[1, 0] = LC.conv64(keep[prev][1:2], w_bad, b, stride, rate)[0, 0]
    assert not np.array_equal(bad, keep["cnv4"])
    assert _flags_layer(cfg, weights, keep, "cnv4", bad)


@pytest.mark.parametrize("short", [8, 1])
def test_short_class_histogram_is_flagged(short):
    """-se_seg_wo_tgt with `short' labelled pixels of one source frame missing from their bin (as if a squeeze chunk
    dropped them): the class table moves by more than the table bar."""
    cfg = parse_version(SEG_WO_TGT)
    img, flow, seg = synth.make_inputs(2, H, W)
    weights = synth.make_weights(cfg)
    want, rows = LC.ref_tables(cfg, img, flow, seg, weights)
    bad_seg = seg.copy()
    bad_seg[1, 0, H - 1, W - short:, 0] = -5.0               # counted in the denominator, in no bin
    assert np.all(seg[1, 0, H - 1, W - short:, 0] < NUM_SEG_CLASSES)
    got = R.class_tables(cfg, img, flow, bad_seg, weights)
    assert rows == [1, 2]
    assert _flags(lambda: LC.check_table(got, want, rows))
    LC.check_table(want + 0.5 * LC.TABLE_TOL, want, rows)    # and within the bar passes


class _Stand_in:
    """Serves the oracle's float32-rounded tensors the way Engine.debug_read does ([2B,...] pair-image major)."""

    def __init__(self, cfg, weights, inputs, fused, plan=((0, 0),)):
        keep = {}
        img, flow, seg = inputs
        self.poses = O.forward(cfg, img, flow, seg, weights, np.float64, keep).astype(np.float32)
        n = img.shape[0]
        self.t = {"att_table": LC.ref_tables(cfg, img, flow, seg, weights)[0],
                  "packed": keep["packed"].reshape(2 * n, img.shape[1], img.shape[2] // 3, 10)[..., LC.PACK8]}
        for k in ("cnv1", "cnv2", "cnv3", "cnv4", "cnv5"):
            self.t[k] = keep[k]
        for k in ("cnv6", "cnv7"):
            self.t[k] = np.concatenate([keep["rotation/" + k], keep["translation/" + k]], -1)
        if fused:
            del self.t["cnv7"]
        self.t = {k: v.astype(np.float32) for k, v in self.t.items()}
        self.plan = plan

    def debug_read(self, name, shape):
        if name not in self.t:
            raise RuntimeError("cnv7 was not materialised")
        assert self.t[name].shape == tuple(shape), (name, self.t[name].shape, shape)
        return self.t[name].copy()

    def last_plan(self, layer):
        return [p for p in self.plan if p[0]]

    def activation_range(self):
        return {}, {k: 0 for k in ("cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6")}


@pytest.mark.parametrize("fused", [True, False])
def test_check_forward_on_oracle_tensors(net, fused):
    """check_forward end to end on float32-rounded oracle tensors: passes, and flags a one-element error in the last
    pair image (the ordering of pair images and the channel slices of the two heads are exercised)."""
    cfg, weights, inputs, _, _ = net
    s = _Stand_in(cfg, weights, inputs, fused)
    stats = LC.check_forward(s, cfg, weights, *inputs, s.poses, "f16x3", what="stand-in")
    assert ("pose(fused)" in stats) == fused and ("cnv7" in stats) != fused
    for name in ("packed", "cnv2", "cnv6") + (() if fused else ("cnv7",)):
        s2 = _Stand_in(cfg, weights, inputs, fused)
        t = s2.t[name]
        t[-1, t.shape[1] // 2, -1, -1] += 1e-3 * np.abs(t).max()
        assert _flags(lambda: LC.check_forward(s2, cfg, weights, *inputs, s2.poses, "f16x3")), name


def test_subset_of_pair_images():
    """plan_images: first two, last two, and the images holding the first and last rows of every launch."""
    cfg = parse_version(FLAGSHIP_VERSION)

    class P:
        def last_plan(self, layer):
            return [(26, 5), (1, 4)] if layer == 4 else [(17, 99)] if layer == 0 else []

    got = LC.plan_images(P(), cfg, 20, 128, 416)            # 40 pair images of 32x104 = 26 rows of 128 each
    assert got == [0, 1, 38, 39]

    class Q:
        def last_plan(self, layer):
            return [(533, 5), (507, 4)] if layer == 4 else []

    assert LC.plan_images(Q(), cfg, 20, 128, 416) == [0, 1, 20, 38, 39]   # row 533 * 128 is in image 20 (3328 rows each)


# ---- storage scales at the edges of the range guard's window ------------------------------------------------------------
def test_guard_floor_is_the_librarys():
    """layer_check.GUARD_FLOOR is range_value_fails' "too small" threshold in csrc/params.h."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "davo_amd", "csrc", "params.h")).read()
    body = src[src.index("inline bool range_value_fails"):]
    body = body[:body.index("}")]
    assert re.search(r"vmax < 0x1p%df" % LC.GUARD_FLOOR_LOG2, body), body
    assert "vmax < 65504.f" in body and LC.GUARD_CEIL == 65504.0


def test_edge_shifts():
    m = {"cnv1": 28.06, "cnv2": 1.0, "cnv3": 2.0 ** -40 * 1.5, "cnv4": 65504.0 / 2 ** 3, "cnv5": 2.0 ** -6 * (1 + 2 ** -12),
         "cnv6": 0.3}
    fl = LC.edge_shifts(m, "floor")
    ce = LC.edge_shifts(m, "ceiling")
    for k, v in m.items():
        lo = v * 2.0 ** fl[k]
        hi = v * 2.0 ** ce[k]
        assert LC.GUARD_FLOOR * (1 + LC.EDGE_BAND) <= lo < 4 * LC.GUARD_FLOOR, (k, lo)
        assert 2.0 ** 14 <= hi < LC.GUARD_CEIL * (1 - LC.EDGE_BAND), (k, hi)
    assert fl["cnv2"] == -5 and fl["cnv5"] == 1 and ce["cnv4"] == 2 and ce["cnv2"] == 15      # the guard bands step inwards
    assert m["cnv1"] * 2.0 ** fl["cnv1"] < 2 * LC.GUARD_FLOOR and m["cnv1"] * 2.0 ** ce["cnv1"] >= 2.0 ** 15
    mixed = LC.edge_shifts(m, {"cnv1": "floor", "cnv2": "ceiling"})
    assert mixed == dict({k: 0 for k in m}, cnv1=fl["cnv1"], cnv2=ce["cnv2"])


def _edge_layer(cfg, weights, keep, name, lo_log2):
    """cnv`name' of the oracle on its float64 input, stored at the shift that puts its maximum at 2^lo_log2's binade."""
    prev, stride, rate, groups = _spec(cfg, weights, name)
    w, b, _, _ = groups[0]
    ref = LC.conv64(keep[prev], w, b, stride, rate)
    where = "floor" if lo_log2 == LC.GUARD_FLOOR_LOG2 else "ceiling"
    return prev, stride, rate, groups, ref, LC.edge_shifts({name: np.abs(ref).max()}, where)[name]


def _flags_at(cfg, weights, keep, name, got, shift):
    prev, stride, rate, groups = _spec(cfg, weights, name)
    return _flags(lambda: LC.check_layer(name, got, keep[prev], groups, stride, rate, LC.TAU["f16x3"][name],
                                         floor=LC.STORE_FLOOR * 2.0 ** -shift, a_floor=True))


@pytest.mark.parametrize("name", ["cnv2", "cnv5"])
def test_pair_storage_at_the_floor(net, name):
    """Exact pair storage with the layer's maximum in the guard's lowest binade passes both bars (with the bar-(a) floor
    term); the same layer with its subnormal lo halves flushed to zero, or computed from an input whose subnormal lo halves
    were dropped (an MFMA that flushes fp16 denormals), is flagged."""
    cfg, weights, _, keep, _ = net
    prev, stride, rate, groups, ref, s = _edge_layer(cfg, weights, keep, name, LC.GUARD_FLOOR_LOG2)
    assert LC.GUARD_FLOOR <= np.abs(ref).max() * 2.0 ** s < 2 * LC.GUARD_FLOOR
    assert not _flags_at(cfg, weights, keep, name, LC.pair_store(ref, s), s)
    assert _flags_at(cfg, weights, keep, name, LC.pair_store(ref, s, flush_lo=True), s)
    # the input stored at ITS floor scale, decoded exactly for the checker, but convolved without its subnormal lo halves
    s_in = LC.edge_shifts({prev: np.abs(keep[prev]).max()}, "floor")[prev]
    x = LC.pair_store(keep[prev], s_in)
    x_flushed = LC.pair_store(keep[prev], s_in, flush_lo=True)
    w, b, _, _ = groups[0]
    keep_in = dict(keep, **{prev: x})
    assert not _flags_at(cfg, weights, keep_in, name, LC.pair_store(LC.conv64(x, w, b, stride, rate), s), s)
    assert _flags_at(cfg, weights, keep_in, name, LC.pair_store(LC.conv64(x_flushed, w, b, stride, rate), s), s)


@pytest.mark.parametrize("name", ["cnv2", "cnv5"])
def test_pair_storage_at_the_ceiling(net, name):
    """Exact pair storage with the maximum in [2^15, 65504) passes; an epilogue that clamps at 2^15 instead of 65504 is
    flagged."""
    cfg, weights, _, keep, _ = net
    _, _, _, _, ref, s = _edge_layer(cfg, weights, keep, name, LC.CEIL_BINADE_LOG2)
    assert 2.0 ** 15 <= np.abs(ref).max() * 2.0 ** s < LC.GUARD_CEIL
    assert not _flags_at(cfg, weights, keep, name, LC.pair_store(ref, s), s)
    assert _flags_at(cfg, weights, keep, name, LC.pair_store(ref, s, clamp=2.0 ** 15), s)
