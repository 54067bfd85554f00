"""f16x3 storage scales layer by layer (tests/layer_check.py), and the range guard's window [2^-6, 65504) on each layer's
stored maximum.  Every storing epilogue applies out_scale = 2^(s_out - s_in) / wscale and bias_scale = wscale 2^s_in; with
all shifts at 0 an epilogue that reads the wrong layer's shift still gets the right answer, so here they are not 0:
  - calibrated scales (each layer's maximum in [2^9, 2^10), what run_kitti_pose.py does) on every default plan and every
    f16x3 launch option of tests/test_plan_layers_gpu.py;
  - every layer at the guard's floor, every layer at the ceiling [2^15, 65504), and floor / ceiling alternating, on cases that
    reach every kernel family, stored cnv7 and fused pose head;
  - each layer just inside and one binade outside either edge, alone: passes untouched / trips the guard, host and device
    path, with and without the automatic recovery;
  - a checkpoint whose every layer sits at the floor by its weights (no calibration): poses at the bar;
  - calibration from scales far off in both directions.
Every forward also checks the range record against what its kernels stored (layer_check.check_range_record)."""
import json

import numpy as np
import pytest

from davo_amd import DAVO, DavoRangeError, Engine, synth, parse_version, FLAGSHIP_VERSION

import layer_check as LC
import test_plan_layers_gpu as TP
from helpers import assert_pose_close

pytestmark = pytest.mark.gpu

CFG = parse_version(FLAGSHIP_VERSION)
WEIGHTS = synth.make_weights(CFG)
WORST = {}                      # (scale set, layer) -> worst bar-(b) ratio


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    yield
    print("worst |err| / L1 mass per scale set:", json.dumps({"%s/%s" % k: v for k, v in sorted(WORST.items())}))


def _note(scale_set, stats):
    for k, v in stats.items():
        if isinstance(v, tuple):
            WORST[(scale_set, k)] = max(WORST.get((scale_set, k), 0.0), v[1])


def _engine(H, W, B, weights=WEIGHTS):
    e = Engine(CFG, H, W, B)
    e.load_weights(weights)
    e.set_precision("f16x3")
    return e


def _check(e, inputs, shifts, what, a_floor=False, checked=None, plan_check=None, images="bounds"):
    """One forward at `shifts`: the range record, then every layer; -> (stats, {layer: (row of the maximum, launches)})."""
    img = inputs[0]
    B, H, W = img.shape[0], img.shape[1], img.shape[2] // 3
    poses, rec = LC.range_record_forward(e, *inputs, shifts)
    if plan_check is not None:
        assert plan_check(e), (what, [e.last_plan(li) for li in range(7)])
    assert e.activation_range()[1] == (shifts or dict.fromkeys(LC.STORED, 0)), what
    where = LC.check_range_record(e, CFG, B, H, W, rec, what)
    stats = LC.check_forward(e, CFG, WEIGHTS, *inputs, poses, "f16x3", images=images, what=what, a_floor=a_floor,
                             checked=checked)
    return stats, where, rec


# ---- calibrated scales -------------------------------------------------------------------------------------------------
# Left out for time (float64 checking): the default plan at B = 128 (B = 32's kernels in one piece, 20 s) and merge_order
# 1 and 2 (merge_order 0's kernels in another order of the merged grid).
CALIBRATED = [pytest.param(H, W, B, 11, {}, None, id="default-%dx%dx%d" % (H, W, B)) for H, W, B in TP.DEFAULT_PLANS if B <= 32] + \
             [pytest.param(H, W, B, 3, opts, chk, id=name) for name, B, H, W, opts, chk in TP.F16X3_OPTIONS
              if name not in ("merge_order1", "merge_order2")]


@pytest.mark.parametrize("H,W,B,first_window,options,plan_check", CALIBRATED)
def test_calibrated_scales(H, W, B, first_window, options, plan_check):
    """calibrate() on the batch moves all six shifts (maxima to [2^9, 2^10)); the layers then pass the unchanged bars."""
    inputs = synth.make_inputs(B, H, W, first_window=first_window)
    e = _engine(H, W, B)
    for k, v in options.items():
        e.set_option(k, v)
    if "fuse_pack" in options:
        e.profile(1)
    shifts = e.calibrate(*inputs)
    assert all(s != 0 for s in shifts.values()), shifts
    stats, _, rec = _check(e, inputs, shifts, "calibrated %dx%d B=%d %s" % (H, W, B, options), plan_check=plan_check)
    assert all(2.0 ** 9 <= rec[k] * 2.0 ** shifts[k] < 2.0 ** 10 for k in LC.STORED), (rec, shifts)     # davo_calibrate's target
    _note("calibrated", stats)
    e.close()


# ---- every layer at the floor / the ceiling ------------------------------------------------------------------------------
SETS = {"floor": "floor", "ceiling": "ceiling",
        "alternating": {k: ("floor", "ceiling")[i % 2] for i, k in enumerate(LC.STORED)}}
# the launch options (tests/test_plan_layers_gpu.py: F16X3_OPTIONS) whose plans reach each kernel family
FAMILIES = {
    "deep_ring0": "conv_patch_h3 (cnv1-cnv3: tiles 99/98/97), conv_igemm_h3 (cnv4-cnv7), deep ring off",
    "fuse_pack1_ragged": "fused-pack cnv1 (mask + pack inside the cnv1 patch kernel)",
    "split_k1": "split-K cnv6 / cnv7 with the separate fix-up kernel",
    "fold_fixup": "split-K with the fix-up folded into pose_tail.h",
    "force_tile6": "conv_igemm_h3s (208x256) on cnv5 / cnv6",
    "force_tile8": "conv_igemm_h3s four-wave 208x128 on cnv4",
    "wave128_2": "conv_igemm_h3w main launches of cnv5 / cnv6, conv_igemm_h3w64 on their remainder rows",
    "wave128_3": "conv_igemm_h3w128 on cnv4",
    "deep_ring1": "deep ring on",
    "share_taps0": "share-taps off",
}
EDGE_CASES = [pytest.param(name, B, H, W, opts, chk, id=name) for name, B, H, W, opts, chk in TP.F16X3_OPTIONS if name in FAMILIES]
assert len(EDGE_CASES) == len(FAMILIES)


@pytest.mark.parametrize("name,B,H,W,options,plan_check", EDGE_CASES)
def test_edge_scale_sets(name, B, H, W, options, plan_check):
    """Each scale set of SETS with fuse_pose 0 (stored cnv7, separate pose head) and 1 (fused pose head, where the frame
    has one: TP._fuses; fuse_pack1_ragged's 36x100 never does): bars (a) with the storage floor and (b), and the range
    record.  The B = 32 (wave128) cases run fuse_pose 1 in the floor set only, checked on the first and last pair image
    (each B = 32 forward reads 1 GB of tensors back), and show that their plans for cnv1-cnv6 - the h3w, h3w64 and h3w128
    launches - do not change with fuse_pose."""
    inputs = synth.make_inputs(B, H, W, first_window=3)
    e = _engine(H, W, B)
    for k, v in options.items():
        e.set_option(k, v)
    if "fuse_pack" in options:
        e.profile(1)
    _, maxima = LC.range_record_forward(e, *inputs)
    for set_name, where in SETS.items():
        shifts = LC.edge_shifts(maxima, where)
        checked = {}
        plans = None
        for fuse_pose in (0, 1) if B <= 8 or set_name == "floor" else (0,):
            e.set_option("fuse_pose", fuse_pose)
            what = "%s %s fuse_pose %d" % (name, set_name, fuse_pose)
            images = "bounds" if B <= 8 or fuse_pose == 0 else [0, 2 * B - 1]
            stats, _, rec = _check(e, inputs, shifts, what, a_floor=True, checked=checked, plan_check=plan_check,
                                   images=images)
            if plans is None:
                plans = [e.last_plan(li) for li in range(6)]
            else:
                assert [e.last_plan(li) for li in range(6)] == plans, (what, plans)
            for k in LC.STORED:
                w = where if isinstance(where, str) else where[k]
                lo, hi = (LC.GUARD_FLOOR, 4 * LC.GUARD_FLOOR) if w == "floor" else (2.0 ** 14, LC.GUARD_CEIL)
                assert lo <= rec[k] * 2.0 ** shifts[k] < hi, (what, k, rec[k], shifts[k])
            assert ("cnv7" in stats) != TP._fuses(H, W, fuse_pose), stats
            _note(set_name, stats)
    e.close()


def test_maxima_in_the_second_launch():
    """Where a layer runs as two launches, the range record must hold the second launch's rows too: the last window made
    louder (flow x 4) puts every layer's maximum into its last pair image, i.e. the remainder launch's rows, and the
    record still equals what was stored (at the floor: the ceiling's record is checked by the edge sets)."""
    name, B, H, W, options, plan_check = [c for c in TP.F16X3_OPTIONS if c[0] == "merge_rem0"][0]
    img, flow, seg = synth.make_inputs(B, H, W, first_window=3)
    flow[-1] *= 4.0
    inputs = (img, flow, seg)
    e = _engine(H, W, B)
    for k, v in options.items():
        e.set_option(k, v)
    _, maxima = LC.range_record_forward(e, *inputs)
    two = set()
    for set_name in ("floor",):
        shifts = LC.edge_shifts(maxima, set_name)
        stats, where, _ = _check(e, inputs, shifts, "loud last window, %s" % set_name, a_floor=True, plan_check=plan_check,
                                 images=[0, 2 * B - 2, 2 * B - 1])                 # the loud window's two pair images
        _note(set_name, stats)
        for k, (row, launches) in where.items():
            if len(launches) == 2:
                two.add(k)
                assert row >= launches[1][0], ("the maximum is not in the second launch", k, row, launches)
    print("layers run as two launches, maximum in the second:", sorted(two))
    assert {"cnv5", "cnv6"} <= two, two
    e.close()


# ---- the guard's edges, one layer at a time --------------------------------------------------------------------------------
GH, GW, GB = 64, 96, 2


@pytest.fixture(scope="module")
def guard_case(c_oracle):
    inputs = synth.make_inputs(GB, GH, GW)
    want = c_oracle.forward(CFG, *inputs, WEIGHTS)
    e = _engine(GH, GW, GB)
    _, maxima = LC.range_record_forward(e, *inputs)
    e.close()
    return inputs, want, maxima


@pytest.mark.parametrize("edge", ["floor", "ceiling"])
@pytest.mark.parametrize("layer", LC.STORED)
def test_guard_edge(guard_case, layer, edge):
    """`layer' alone with its stored maximum just inside the window: nothing re-issued, the layer check passes.  One
    binade outside: with "auto_range" 0 DavoRangeError names the layer; by default one re-calibration and one re-issue,
    and the poses meet the bar.  On cnv1 and cnv6 the same through forward_device + synchronize."""
    inputs, want, maxima = guard_case
    inside = dict.fromkeys(LC.STORED, 0)
    inside[layer] = LC.edge_shifts({layer: maxima[layer]}, edge)[layer]
    outside = dict(inside)
    outside[layer] = LC.binade_shift(maxima[layer], LC.GUARD_FLOOR_LOG2 - 1 if edge == "floor" else 16)
    e = _engine(GH, GW, GB)
    st = e.range_stats()
    stats, _, rec = _check(e, inputs, inside, "%s at the %s" % (layer, edge), a_floor=edge == "floor")
    _note("edge-" + edge, stats)
    stored = rec[layer] * 2.0 ** inside[layer]
    assert (LC.GUARD_FLOOR <= stored < 4 * LC.GUARD_FLOOR) if edge == "floor" else (2.0 ** 14 <= stored < LC.GUARD_CEIL), stored
    assert e.range_stats() == st
    e.set_option("auto_range", 0)
    e.set_activation_shifts(outside)
    with pytest.raises(DavoRangeError, match="%s activations" % layer):
        e.forward(*inputs)
    e.set_option("auto_range", 1)
    e.set_activation_shifts(outside)
    got = e.forward(*inputs)
    st2 = e.range_stats()
    assert st2 == {"recalibrations": st["recalibrations"] + 1, "f32_batches": st["f32_batches"],
                   "reissued": st["reissued"] + 1}, (st, st2, e.range_report())
    assert_pose_close(got, want, "%s one binade past the %s, recovered" % (layer, edge))
    if layer in ("cnv1", "cnv6"):
        img, flow, seg = inputs
        bufs = (e.alloc(img.nbytes).upload(img), e.alloc(flow.nbytes).upload(flow), e.alloc(seg.nbytes).upload(seg),
                e.alloc(GB * 48))
        e.set_activation_shifts(inside)
        st = e.range_stats()
        e.forward_device(GB, *bufs)
        e.synchronize()
        assert e.range_stats() == st
        assert_pose_close(bufs[3].download((GB, 2, 6)), want, "device path, %s at the %s" % (layer, edge))
        e.set_option("auto_range", 0)
        e.set_activation_shifts(outside)
        e.forward_device(GB, *bufs)
        with pytest.raises(DavoRangeError, match="%s activations" % layer):
            e.synchronize()
        e.synchronize()
        e.set_option("auto_range", 1)
        e.set_activation_shifts(outside)
        e.forward_device(GB, *bufs)
        e.synchronize()
        st2 = e.range_stats()
        assert st2["reissued"] == st["reissued"] + 1 and st2["recalibrations"] == st["recalibrations"] + 1, (st, st2)
        assert_pose_close(bufs[3].download((GB, 2, 6)), want, "device path, %s past the %s, recovered" % (layer, edge))
        for b in bufs:
            b.free()
    e.close()


# ---- a checkpoint that sits at the floor by its weights ---------------------------------------------------------------------
def rescaled_checkpoint(weights, shifts):
    """The same network with every stored layer's activations x 2^shifts[layer] (ReLU layers are homogeneous): cnv_l's
    weights x 2^(s_l - s_(l-1)) and biases x 2^s_l, cnv7's weights x 2^-s_6, so cnv7 and the poses are unchanged."""
    w2 = dict(weights)
    prev = 0
    names = {"cnv6": ["pose/rotation/cnv6", "pose/translation/cnv6"]}
    for k in LC.STORED:
        f = np.float32(2.0 ** (shifts[k] - prev))
        for n in names.get(k, [k]):
            w2["pose_exp_net/%s/weights" % n] = weights["pose_exp_net/%s/weights" % n] * f
            w2["pose_exp_net/%s/biases" % n] = weights["pose_exp_net/%s/biases" % n] * np.float32(2.0 ** shifts[k])
        prev = shifts[k]
    for n in ("pose/rotation/cnv7", "pose/translation/cnv7"):
        w2["pose_exp_net/%s/weights" % n] = weights["pose_exp_net/%s/weights" % n] * np.float32(2.0 ** -prev)
    return w2


@pytest.mark.parametrize("binade", ["floor", "old_floor"])
@pytest.mark.parametrize("H,W,B", [(16, 16, 1), (20, 48, 2), (36, 100, 3)])
def test_rescaled_checkpoint(c_oracle, H, W, B, binade):
    """Every layer's natural maximum in the guard's lowest binade (floor: no re-issue), or in [2^-11, 2^-10), the lowest
    one before the floor was raised (the guard trips, re-calibrates and re-issues): through Engine and DAVO.inference,
    with no calibration, the poses meet the bar against the C oracle on the original weights."""
    inputs = synth.make_inputs(B, H, W, first_window=3)
    want = c_oracle.forward(CFG, *inputs, WEIGHTS)
    e = _engine(H, W, B)
    _, maxima = LC.range_record_forward(e, *inputs)
    e.close()
    if binade == "floor":
        shifts = LC.edge_shifts(maxima, "floor")
    else:
        shifts = {k: LC.binade_shift(m, -11) for k, m in maxima.items()}
    w2 = rescaled_checkpoint(WEIGHTS, shifts)
    e = _engine(H, W, B, w2)
    got = e.forward(*inputs)
    err = assert_pose_close(got, want, "%dx%d B=%d rescaled to the %s, Engine" % (H, W, B, binade))
    st = e.range_stats()
    mx, sh = e.activation_range()
    print("rescaled %s %dx%d B=%d: pose err %.3g, range stats %s" % (binade, H, W, B, err, st))
    if binade == "floor":
        assert st == {"recalibrations": 0, "f32_batches": 0, "reissued": 0}, st
        assert sh == dict.fromkeys(LC.STORED, 0) and all(LC.GUARD_FLOOR <= mx[k] < 4 * LC.GUARD_FLOOR for k in mx), (mx, sh)
    else:
        assert st == {"recalibrations": 1, "f32_batches": 0, "reissued": 1}, st
    e.close()
    d = DAVO(version=FLAGSHIP_VERSION)
    d.load_weights(w2)
    d.setup_inference(H, W, "davo", 3, B, inputs[0], None, inputs[1], None, inputs[2])
    assert_pose_close(d.inference(None, "pose")["pose"], want, "%dx%d B=%d rescaled to the %s, DAVO.inference" % (H, W, B, binade))
    d.engine.close()


# ---- calibration from a bad start ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [(20, -30, 25, -20, 18, -25), (-30, 20, -25, 20, -18, 25)])
def test_calibration_from_a_bad_start(bad):
    """calibrate() from scales far off in both directions (clamped layers and layers at 2^-20 of the fp16 range) returns
    the scales a calibration from zero returns."""
    inputs = synth.make_inputs(GB, GH, GW)
    e = _engine(GH, GW, GB)
    plain = e.calibrate(*inputs)
    e.set_activation_shifts(dict(zip(LC.STORED, bad)))
    assert e.calibrate(*inputs) == plain, bad
    e.close()
