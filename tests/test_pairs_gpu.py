"""Pair selection on the GPU (include/davo_hip.h: davo_set_pairs): with one pair selected a batch of B windows runs B pair
images, image n being window n's selected pair.  Held against a both-pairs forward of the same inputs - bit for bit where a
layer is a single K chain (fuse_pose 0, split_k 0: the property of test_batching_is_per_sample_and_deterministic, here on odd
pair-image counts), to 1e-6 of max|both| at the default options (the tolerance of the batch-position tests) - and against the
float64 oracle and the project's restatements at the parity bar of tests/helpers.py.  The row of the pair that was not selected
is exactly +0.0.  Frames are 64x96 (cnv2..cnv6 maps 16x24, cnv7 8x12) unless a test says otherwise; max_batch is 8."""

import numpy as np
import pytest

from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION
from davo_amd import sequence as S

import class_table_ref as R
import depth_source_ref as D
import feature_attention_cases as FA
import feature_attention_ref as F
import layer_check as LC
from helpers import assert_pose_close, hip_free_bytes

pytestmark = pytest.mark.gpu

H, W, MAXB = 64, 96, 8
BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
V0 = "v0-sharedNN-dilatedPoseNN-segmask-se_flow-abs_flow-fc_tanh"
PRECISIONS = ["f16x3", "f32"]
SELECTIONS = ["src0", "src1"]
ROW = {"src0": 0, "src1": 1}
BATCHES = [1, 2, 3, 5]
STORED = ("cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6", "cnv7")


def _engine(cfg, weights, precision, h=H, w=W, max_batch=MAXB):
    e = Engine(cfg, h, w, max_batch)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


_FLAGSHIP = {}


def _flagship(c_oracle=None):
    """(cfg, inputs of five windows, weights, the oracle's poses), computed once"""
    if not _FLAGSHIP:
        cfg = parse_version(FLAGSHIP_VERSION)
        _FLAGSHIP.update(cfg=cfg, inputs=synth.make_inputs(5, H, W), weights=synth.make_weights(cfg))
    if c_oracle is not None and "want" not in _FLAGSHIP:
        _FLAGSHIP["want"] = c_oracle.forward(_FLAGSHIP["cfg"], *_FLAGSHIP["inputs"], _FLAGSHIP["weights"])
    return _FLAGSHIP


def _first(inputs, B):
    return tuple(a[:B] for a in inputs)


def _assert_unselected_row_is_plus_zero(poses, sel, what=""):
    other = poses[:, 1 - ROW[sel]]
    assert np.array_equal(other.view(np.uint32), np.zeros(other.shape, np.uint32)), (what, other)


def _kernels(e, inputs, **kw):
    e.profile(1)
    e.profile_reset()
    e.forward(*inputs, **kw)
    names = {k for k, (n, _) in e.profile_entries().items() if n > 0}
    e.profile(0)
    return names


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B", BATCHES)
def test_every_stored_layer_equals_the_both_pairs_forward_to_the_bit(B, precision):
    f = _flagship()
    cfg, inputs = f["cfg"], _first(f["inputs"], B)
    e = _engine(cfg, f["weights"], precision)
    e.set_option("fuse_pose", 0)
    e.set_option("split_k", 0)
    sh = LC.shapes(cfg, H, W)
    both = e.forward(*inputs)
    layers = {name: e.debug_read(name, (2 * B,) + sh[name]) for name in STORED}
    assert ("se_excite" not in _kernels(e, inputs)) == (B <= 2)          # B = 1, 2: the excitation folded into the squeeze
    for sel in SELECTIONS:
        what = "B=%d %s %s" % (B, sel, precision)
        e.set_pairs(sel)
        assert e.pairs == sel
        got = e.forward(*inputs)
        assert got.shape == (B, 2, 6)
        assert np.array_equal(got[:, ROW[sel]], both[:, ROW[sel]]), what
        _assert_unselected_row_is_plus_zero(got, sel, what)
        for name in STORED:
            one = e.debug_read(name, (B,) + sh[name])                     # B images: image n is window n's selected pair
            assert np.array_equal(one, layers[name][ROW[sel]::2]), (what, name)
        with pytest.raises(ValueError):
            e.debug_read("cnv1", (2 * B,) + sh["cnv1"])
        assert ("se_excite" not in _kernels(e, inputs)) == (B <= 2)
    e.set_pairs("both")
    assert np.array_equal(e.forward(*inputs), both)
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B", BATCHES)
def test_default_options_stay_within_rounding_of_both_pairs_and_at_the_bar(c_oracle, B, precision):
    """fused pose head where the map allows it, split-K where the planner picks it"""
    f = _flagship(c_oracle)
    cfg, inputs, want = f["cfg"], _first(f["inputs"], B), f["want"][:B]
    e = _engine(cfg, f["weights"], precision)
    both = e.forward(*inputs)
    assert_pose_close(both, want, "both pairs")
    for sel in SELECTIONS:
        what = "B=%d %s %s" % (B, sel, precision)
        e.set_pairs(sel)
        got = e.forward(*inputs)
        err = np.abs(got[:, ROW[sel]] - both[:, ROW[sel]]).max()
        print("%s: max|one pair - both| %.3g, max|both| %.3g" % (what, err, np.abs(both).max()))
        assert err <= 1e-6 * np.abs(both).max(), what
        assert_pose_close(got[:, ROW[sel]], want[:, ROW[sel]], what + " vs the oracle")
        _assert_unselected_row_is_plus_zero(got, sel, what)
        for _ in range(3):
            assert np.array_equal(e.forward(*inputs), got), what
    e.close()


def _variant_case(sub, c_oracle):
    """(cfg, inputs of three windows - depth last where the variant reads it, weights, reference poses)"""
    B, conv = 3, c_oracle.conv2d_same
    if sub == "v0":
        cfg = parse_version(V0)
        inputs, w = synth.make_inputs(B, H, W, first_window=2), synth.make_weights(cfg)
        return cfg, inputs, w, c_oracle.forward(cfg, *inputs, w)
    if sub == "-no_segmask-se_insert":
        cfg = parse_version(FA.PUBLISHED)
        inputs, w0 = FA.inputs(B, H, W), synth.make_weights(cfg)
        cnv5 = F.trunk(cfg, *inputs, w0)
        w = F.sensitive_weights(cfg, w0, F.descriptors(cnv5, w0))
        return cfg, inputs, w, F.forward(cfg, *inputs, w, cnv5=cnv5)
    cfg = parse_version(BASE + sub + "-fc_tanh")
    inputs = synth.make_inputs(B, H, W, first_window=2)
    inputs[2][0, 0, :3, :5] = np.nan                          # labels outside the 19 classes: no table row
    inputs[2][-1, 2, :2] = 19.0
    if cfg.needs_depth:
        depth = synth.make_depth(B, H, W, first_window=2)
        w = D.sensitive_weights(cfg, synth.make_weights(cfg), depth)
        return cfg, inputs + (depth,), w, D.forward(cfg, *inputs, depth, w, conv=conv)
    w = synth.make_weights(cfg)
    return cfg, inputs, w, R.forward(cfg, *inputs, w, conv=conv)


def _call(e, inputs, fn=None):
    fn = fn or e.forward
    return fn(*inputs[:3], depth=inputs[3]) if len(inputs) == 4 else fn(*inputs)


_VARIANTS = {}


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("sub", ["-se_rgb_to_seg", "-se_SegFlow_to_seg", "-se_depth_to_seg", "-no_segmask-se_insert", "v0"])
def test_variants(c_oracle, sub, precision):
    """B = 3 (the excitation as a launch of its own, an odd pair-image count): the target attended (-se_rgb_to_seg), the
    seg+flow descriptor, depth as a fourth input, the feature-attention block on cnv5 (one evaluation per pair image), a v0
    string (rgb only)."""
    if sub not in _VARIANTS:
        _VARIANTS[sub] = _variant_case(sub, c_oracle)
    cfg, inputs, w, want = _VARIANTS[sub]
    e = _engine(cfg, w, precision)
    both = _call(e, inputs)
    assert_pose_close(both, want, sub + " both pairs")
    for sel in SELECTIONS:
        what = "%s %s %s" % (sub, sel, precision)
        e.set_pairs(sel)
        got = _call(e, inputs)
        assert np.abs(got[:, ROW[sel]] - both[:, ROW[sel]]).max() <= 1e-6 * np.abs(both).max(), what
        assert_pose_close(got[:, ROW[sel]], np.asarray(want)[:, ROW[sel]], what + " vs the restatement")
        _assert_unselected_row_is_plus_zero(got, sel, what)
        assert np.array_equal(_call(e, inputs), got), what
    e.close()


@pytest.mark.parametrize("option", ["fuse_pack", "impl_direct"])
@pytest.mark.parametrize("B", [1, 3])
def test_options_that_change_the_index_deriving_kernels(B, option):
    """fuse_pack 1: cnv1's patch fill maps a pair image to its window and source itself; impl 1: mask_pack<10> and the
    two-kernel pose head.  Single K chains (fuse_pose 0, split_k 0): the selected row to the bit."""
    f = _flagship()
    inputs = _first(f["inputs"], B)
    e = _engine(f["cfg"], f["weights"], "f16x3" if option == "fuse_pack" else "f32")
    e.set_option("fuse_pose", 0)
    e.set_option("split_k", 0)
    if option == "fuse_pack":
        e.set_option("fuse_pack", 1)
    else:
        e.set_impl("direct")
    both = e.forward(*inputs)
    if option == "fuse_pack":
        assert "mask_pack" not in _kernels(e, inputs)
    for sel in SELECTIONS:
        e.set_pairs(sel)
        got = e.forward(*inputs)
        assert np.array_equal(got[:, ROW[sel]], both[:, ROW[sel]]), (option, B, sel)
        _assert_unselected_row_is_plus_zero(got, sel)
    e.close()


def _poisoned(inputs, sel):
    """the unselected source frame's third of the strip replaced by other bytes, its flow, label and depth planes by NaN"""
    out = [a.copy() for a in inputs]
    other = 1 - ROW[sel]                                      # source frame index: 0 = src0, 1 = src1
    third = slice(0, W) if other == 0 else slice(2 * W, 3 * W)
    out[0][:, :, third] = 255 - out[0][:, :, third]
    out[1][:, other] = np.nan
    for a in out[2:]:
        a[:, 2 * other] = np.nan                              # file order src0, tgt, src1
    return tuple(out)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("sub", ["flagship", "-se_rgb_to_seg", "-se_depth_to_seg"])
def test_an_unselected_frames_bytes_reach_nothing(sub, precision):
    B = 3
    if sub == "flagship":
        f = _flagship()
        cfg, inputs, w = f["cfg"], _first(f["inputs"], B), f["weights"]
    else:
        cfg = parse_version(BASE + sub + "-fc_tanh")
        inputs = synth.make_inputs(B, H, W, first_window=2)
        w = synth.make_weights(cfg)
        if cfg.needs_depth:
            inputs += (synth.make_depth(B, H, W, first_window=2),)
            w = D.sensitive_weights(cfg, w, inputs[3])
    e = _engine(cfg, w, precision)

    def device(parts):
        bufs = [e.alloc(a.nbytes).upload(a) for a in parts] + [e.alloc(B * 2 * 6 * 4)]
        e.forward_device(B, bufs[0], bufs[1], bufs[2], bufs[-1], **({"depth": bufs[3]} if len(parts) == 4 else {}))
        e.synchronize()
        got = bufs[-1].download((B, 2, 6))
        for b in bufs:
            b.free()
        return got

    for sel in SELECTIONS:
        e.set_pairs(sel)
        dirty = _poisoned(inputs, sel)
        assert np.isnan(dirty[1]).any() and not np.array_equal(dirty[0], inputs[0])
        for path in ("forward", "forward_device"):
            run = (lambda parts: _call(e, parts)) if path == "forward" else device
            e.activation_range(reset=True)
            clean = run(inputs)
            clean_range = e.activation_range(reset=True)
            got = run(dirty)
            got_range = e.activation_range(reset=True)
            assert np.isfinite(clean).all() and clean[:, ROW[sel]].any()
            assert np.array_equal(got, clean), (sub, sel, path)
            assert got_range == clean_range, (sub, sel, path)
    st = e.range_stats()
    assert st["reissued"] == 0 and st["f32_batches"] == 0, st
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_switching_on_one_engine_equals_fresh_engines(precision):
    f = _flagship()
    cfg, w, inputs = f["cfg"], f["weights"], _first(f["inputs"], 3)
    fresh = {}
    for sel in ("both", "src1", "src0"):
        e = _engine(cfg, w, precision)
        e.set_pairs(sel)
        fresh[sel] = e.forward(*inputs)
        e.close()
    e = _engine(cfg, w, precision)
    for sel in ("both", "src1", "both", "src0", "src1", "both"):
        e.set_pairs(sel)
        assert np.array_equal(e.forward(*inputs), fresh[sel]), sel
    # streamed, two in flight, the selection switched between consecutive submits: each batch is delivered as submitted
    e.set_inflight(2)
    order = ["both", "src1", "src0", "src1", "both", "src0", "both", "src1", "src1", "both"]
    outs = [np.full((3, 2, 6), np.nan, np.float32) for _ in order]
    bufs = [a.copy() for a in inputs]
    for sel, out in zip(order, outs):
        for buf, a in zip(bufs, inputs):
            buf[...] = a
        e.set_pairs(sel)
        e.submit(*bufs, out)                                  # hold = 0: consumed on return
        for buf in bufs:
            buf[...] = 255 if buf.dtype == np.uint8 else np.nan
    e.set_pairs("src0")                                       # ... and a switch behind the last submit changes nothing in flight
    e.wait()
    for sel, out in zip(order, outs):
        assert np.array_equal(out, fresh[sel]), sel
    with pytest.raises(ValueError):
        e.set_pairs("trajectory")
    with pytest.raises(ValueError, match="pairs"):
        e._check(e._L.davo_set_pairs(e._ctx, 0))
    assert e.pairs == "src0"
    e.close()


def _rescaled(weights, shift):
    """the same network with cnv3's activations 2^shift larger (ReLU is homogeneous): trips the f16x3 range guard
    (tests/test_stream.py)"""
    w = dict(weights)
    s = np.float32(2.0 ** shift)
    w["pose_exp_net/cnv3/weights"] = weights["pose_exp_net/cnv3/weights"] * s
    w["pose_exp_net/cnv3/biases"] = weights["pose_exp_net/cnv3/biases"] * s
    w["pose_exp_net/cnv4/weights"] = weights["pose_exp_net/cnv4/weights"] / s
    return w


def test_a_tripped_batch_is_reissued_with_the_selection_it_was_submitted_under(c_oracle):
    f = _flagship(c_oracle)
    cfg, inputs, want = f["cfg"], _first(f["inputs"], 3), f["want"][:3]
    e = _engine(cfg, _rescaled(f["weights"], 16), "f16x3")
    e.set_inflight(2)
    before = e.range_stats()
    bufs = [a.copy() for a in inputs]
    out = np.full((3, 2, 6), np.nan, np.float32)
    e.set_pairs("src1")
    e.submit(*bufs, out)
    for buf in bufs:
        buf[...] = 255 if buf.dtype == np.uint8 else np.nan      # recycled before the verdict
    e.set_pairs("both")                                       # right behind the submit
    e.wait()
    after = e.range_stats()
    assert after["reissued"] == before["reissued"] + 1, (before, after, e.range_report())
    assert_pose_close(out[:, 1], want[:, 1], "re-issued with src1")
    _assert_unselected_row_is_plus_zero(out, "src1")
    # the scales are settled now; the next batch runs both pairs, as the context says
    out2 = np.full((3, 2, 6), np.nan, np.float32)
    e.submit(*inputs, out2)
    e.synchronize()
    assert e.range_stats()["reissued"] == after["reissued"]
    assert_pose_close(out2, want, "both pairs after the recovery")
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_pair_of_four_windows_runs_the_plan_of_both_pairs_of_two(precision):
    f = _flagship()
    e = _engine(f["cfg"], f["weights"], precision)
    e.forward(*_first(f["inputs"], 2))
    want = [(e.last_plan(l), e.last_split(l)) for l in range(7)]
    e.set_pairs("src1")
    e.forward(*_first(f["inputs"], 4))
    assert [(e.last_plan(l), e.last_split(l)) for l in range(7)] == want
    e.set_pairs("both")
    e.forward(*_first(f["inputs"], 4))
    assert [e.last_plan(l) for l in range(7)] != [p for p, _ in want]
    e.close()


def test_create_set_pairs_stream_and_close_leaves_no_device_memory_behind():
    f = _flagship()
    inputs = _first(f["inputs"], 2)
    w = _rescaled(f["weights"], 16)
    free = []
    for k in range(10):
        e = _engine(f["cfg"], w, "f16x3")
        e.set_inflight(2)
        outs = [np.empty((2, 2, 6), np.float32) for _ in range(3)]
        for sel, out in zip(("src1", "both", "src0"), outs):
            e.set_pairs(sel)
            e.submit(*inputs, out)
        e.wait()
        e.synchronize()
        assert e.range_stats()["reissued"] >= 1
        e.close()
        free.append(hip_free_bytes())
    assert free[9] == free[0], free


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("sub", ["flagship", "-no_segmask-se_insert"])
def test_full_size_frames_odd_pair_image_count_under_the_fused_pose_head(c_oracle, sub, precision):
    """128x416, B = 3, src1, default options: three pair images of 832 cnv7 pixels under the fused pose head.  The feature-attention
    case is held against the restatement on the windows tests/feature_attention_cases.py shares (the first two of the three;
    one float64 trunk per process) - the C oracle has no such block."""
    h, w_, B = 128, 416, 3
    if sub == "flagship":
        cfg = parse_version(FLAGSHIP_VERSION)
        inputs, w = synth.make_inputs(B, h, w_), synth.make_weights(cfg)
        want = c_oracle.forward(cfg, *inputs, w)
    else:
        cfg, two, w, _ = FA.case(h, w_, 2)
        inputs = FA.inputs(B, h, w_)
        assert all(np.array_equal(a[:2], b) for a, b in zip(inputs, two))
        want = np.asarray(FA.reference(h, w_, 2))
    e = _engine(cfg, w, precision, h, w_, B)
    both = e.forward(*inputs)
    e.set_pairs("src1")
    got = e.forward(*inputs)
    assert np.abs(got[:, 1] - both[:, 1]).max() <= 1e-6 * np.abs(both).max()
    n = want.shape[0]
    assert_pose_close(got[:n, 1], want[:, 1], "%s src1 %s" % (sub, precision))
    _assert_unselected_row_is_plus_zero(got, "src1")
    with pytest.raises(Exception, match="fused"):             # the pose head did run fused
        e.debug_read("cnv7", (B, 16, 52, 512))
    for _ in range(3):
        assert np.array_equal(e.forward(*inputs), got)
    e.close()


def _cli(args, out_dir):
    from davo_amd import run_kitti_pose as cli
    cli.main(list(args) + ["--output_dir", str(out_dir), "--img_height", str(H), "--img_width", str(W), "--test_seq", "9"])
    return open(str(out_dir / "09-pred_kitti_pose.txt"), "rb").read()


def test_cli_trajectory_mode_writes_the_file_of_the_poses_under_the_per_batch_selections(tmp_path):
    """run_kitti_pose --synthetic 13 --batch_size 4 --no_calibrate --pairs trajectory: eleven windows, batches of 4, 4 and a
    ragged 3.  The file is byte for byte the stitch of poses computed here with Engine.forward on the same (padded) batches
    under the same selections: both pairs for the first, src1 for the other two."""
    n_frames, B = 13, 4
    common = ["--synthetic", str(n_frames), "--batch_size", str(B), "--no_calibrate"]
    got = _cli(common + ["--pairs", "trajectory"], tmp_path / "trajectory")
    load = S.synthetic_window_loader(H, W)
    cfg = parse_version(FLAGSHIP_VERSION)
    e = _engine(cfg, synth.make_weights(FLAGSHIP_VERSION), "f16x3", max_batch=B)
    poses = np.zeros((n_frames - 2, 2, 6), np.float32)
    for s in range(0, n_frames - 2, B):
        end = min(s + B, n_frames - 2)
        parts, n = S._pad_parts(load(s, end), B)
        e.set_pairs("both" if s == 0 else "src1")
        poses[s:end] = e.forward(*parts)[:n]
    e.close()
    assert poses[:B, 0].any() and not poses[B:, 0].any() and poses[:, 1].any(axis=1).all()
    S.write_kitti_poses(str(tmp_path / "want.txt"), S.stitch_trajectory(poses))
    assert got == open(str(tmp_path / "want.txt"), "rb").read()
    assert len(got.splitlines()) == n_frames
    # the default mode is the launch without the flag, byte for byte - and the trajectory mode's file is that file to rounding
    plain = _cli(common, tmp_path / "plain")
    assert _cli(common + ["--pairs", "both"], tmp_path / "both") == plain
    a = S.read_kitti_poses(str(tmp_path / "plain" / "09-pred_kitti_pose.txt"))
    b = S.read_kitti_poses(str(tmp_path / "trajectory" / "09-pred_kitti_pose.txt"))
    assert np.abs(a - b).max() <= 1e-4
