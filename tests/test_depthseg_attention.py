"""The depth-split flow attention (att_source 13: -se_flow_on_depthseg_seplayers) without a GPU: the parser, the weight
surface, the float64 restatement of tests/depthseg_attention_ref.py against hand-built answers, the condition on the test
inputs that both sides of the threshold are exercised, and the header / binding / library surface."""
import ctypes
import os
import re

import numpy as np
import pytest

from davo_amd import _lib, synth, parse_version, FLAGSHIP_VERSION, tf_checkpoint as T
from davo_amd.version import ATT_SOURCE, NUM_SEG_CLASSES, UnsupportedVariantError, weight_shapes
from oracle import davo_oracle as O

import depthseg_attention_ref as R
from helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NET = "v1-sharedNN-dilatedPoseNN"
SUB = "-se_flow_on_depthseg_seplayers"
FULL = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all-se_flow_on_depthseg_seplayers-abs_flow-fc_tanh"
SHAPES = [(36, 100, 3), (64, 96, 2), (128, 416, 1), (32, 64, 1)]


# ---- parser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [NET + SUB, FULL])
def test_the_substring_parses_alone_and_inside_the_full_string(version):
    cfg = parse_version(version)
    assert cfg.att_source == "se_flow_depthseg_sep" and ATT_SOURCE[cfg.att_source] == 13
    assert len(cfg.as_c_ints()) == 8 and cfg.as_c_ints()[5] == 13
    assert cfg.needs_depth and not cfg.tgt_attended and cfg.se_scope is None
    assert cfg.depth_thres_init == 15.0
    assert max(ATT_SOURCE.values()) == 13 and sorted(ATT_SOURCE.values()) == list(range(14))      # appended, nothing renumbered


def test_the_full_string_keeps_its_other_switches():
    cfg = parse_version(FULL)
    assert cfg.as_c_ints() == (5, 128, 1, 0, 3, 13, 1, 1)
    assert parse_version(FULL.replace(SUB, "-se_flow")).as_c_ints() == (5, 128, 1, 0, 3, 1, 1, 1)


@pytest.mark.parametrize("suffix,want", [("_20", 20.0), ("_12.5", 12.5), ("", 15.0)])
def test_the_number_behind_the_substring_sets_the_threshold_initialiser(suffix, want):
    assert parse_version(NET + "-segmask_all" + SUB + suffix + "-fc_tanh").depth_thres_init == want
    assert parse_version(NET + "-segmask_all-se_flow").depth_thres_init == 15.0


@pytest.mark.parametrize("other", ["-se_flow", "-se_depth_to_seg", "-se_depth_wo_tgt_to_seg", "-no_segmask"])
def test_the_substring_wins_over_later_branches_of_the_chain(other):
    for version in (NET + SUB + other, NET + other + SUB):
        assert parse_version(version).att_source == "se_flow_depthseg_sep", version


@pytest.mark.parametrize("version", [NET + "-se_flow_on_depthseg_sharedlayers", NET + "-se_flow_on_depthseg_sharedlayers_20",
                                     NET + "-se_flow_on_depthseg", NET + SUB + "-norm_depth", NET + SUB + "-se_insert",
                                     NET + "-se_flow_on_depthseg_sharedlayers" + SUB, NET + SUB + "_1.2.3", NET + SUB + "_."])
def test_the_neighbouring_strings_still_raise(version):
    with pytest.raises(UnsupportedVariantError):
        parse_version(version)


# (version, major, att_source, as_c_ints, posenn_se) as the parser returned them before source 13 existed
GOLDEN_CONFIGS = [
    ('v0-sharedNN-dilatedPoseNN-segmask-se_flow-abs_flow-fc_tanh', 'v0', 'se_flow', (3, 128, 1, 0, 3, 1, 1, 0), 'none'),
    ('v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all-se_flow-abs_flow-fc_tanh', 'v1', 'se_flow', (5, 128, 1, 0, 3, 1, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-cnv6_64-no_segmask', 'v1', 'ones', (5, 64, 0, 0, 0, 0, 0, 0), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_all', 'v1', 'static_all', (5, 128, 0, 0, 0, 3, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_all-se_flow-norm_flow-abs_flow_h', 'v1', 'se_flow', (5, 128, 0, 1, 1, 1, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_all-static', 'v1', 'static_src', (5, 128, 0, 0, 0, 2, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_rgb-se_flow-fc_lrelu-abs_flow_v', 'v1', 'se_flow', (5, 128, 2, 0, 2, 1, 1, 0), 'none'),
]


def test_every_golden_version_string_parses_as_before():
    listed = {g[0]: g[1:] for g in GOLDEN_CONFIGS}
    versions = {case["version"] for case in load_golden()["cases"].values()}
    assert versions == set(listed)                             # a new golden string must be listed here with its config
    for v in sorted(versions):
        cfg = parse_version(v)
        assert (cfg.major, cfg.att_source, cfg.as_c_ints(), cfg.posenn_se) == listed[v], v
        assert not cfg.needs_depth and cfg.depth_thres_init == 15.0


# ---- weights ---------------------------------------------------------------------------------------------------------
NINE = {"pose_exp_net/se_flow_near/bottleneck_fc/kernel": (2, 8), "pose_exp_net/se_flow_near/bottleneck_fc/bias": (8,),
        "pose_exp_net/se_flow_near/recover_fc/kernel": (8, 19), "pose_exp_net/se_flow_near/recover_fc/bias": (19,),
        "pose_exp_net/se_flow_far/bottleneck_fc/kernel": (2, 8), "pose_exp_net/se_flow_far/bottleneck_fc/bias": (8,),
        "pose_exp_net/se_flow_far/recover_fc/kernel": (8, 19), "pose_exp_net/se_flow_far/recover_fc/bias": (19,),
        "pose_exp_net/se_flow/depth_threshold": ()}


def test_weight_shapes_are_the_posenn_names_plus_the_nine():
    """The PoseNN's own variables are what `-no_segmask' needs (the flagship's 26 names less its four se_flow/*_fc)."""
    sh = weight_shapes(parse_version(FULL))
    posenn = weight_shapes(parse_version(FULL.replace("-segmask_all" + SUB, "-no_segmask")))
    flagship = weight_shapes(parse_version(FLAGSHIP_VERSION))
    assert len(flagship) == 26 and set(posenn) == {k for k in flagship if "/se_flow/" not in k}
    assert set(sh) == set(posenn) | set(NINE) and len(sh) == len(posenn) + 9
    for k in posenn:
        assert sh[k] == posenn[k], k
    for k, shape in NINE.items():
        assert sh[k] == shape, k
    assert not any(re.search(r"/se_flow/.*_fc/", k) for k in sh)


@pytest.mark.parametrize("suffix,init", [("", 15.0), ("_20", 20.0), ("_12.5", 12.5)])
def test_make_weights_is_reproducible_and_the_threshold_is_near_its_initialiser(suffix, init):
    version = FULL.replace(SUB, SUB + suffix)
    a, b = synth.make_weights(version), synth.make_weights(parse_version(version))
    assert set(a) == set(weight_shapes(parse_version(version)))
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == weight_shapes(parse_version(version))[k] and np.array_equal(a[k], b[k]), k
    thr = a[R.THRESHOLD]
    assert thr.shape == () and abs(float(thr) - init) < 1.0 and float(thr) != init
    # the two MLPs are drawn on streams of their own: they differ from each other and from the flagship's se_flow
    f = synth.make_weights(FLAGSHIP_VERSION)
    for part in R.PARTS:
        near, far = a["pose_exp_net/se_flow_near/" + part], a["pose_exp_net/se_flow_far/" + part]
        assert not np.array_equal(near, far) and not np.array_equal(near, f["pose_exp_net/se_flow/" + part])
    # ... and the PoseNN is the flagship's
    assert np.array_equal(a["pose_exp_net/cnv1/weights"], f["pose_exp_net/cnv1/weights"])


def test_a_tf_bundle_round_trips_the_rank_0_threshold_to_the_bit(tmp_path):
    w = synth.make_weights(FULL)
    T.write_checkpoint(str(tmp_path / "model-7"), w)
    listed = {name: shape for name, shape, _ in T.list_variables(str(tmp_path))}
    assert listed[R.THRESHOLD] == ()
    back = T.read_checkpoint(str(tmp_path), verify_crc=True)
    assert set(back) == set(w)
    for k in w:
        assert back[k].shape == w[k].shape and back[k].dtype == np.float32 and np.array_equal(back[k], w[k]), k
    assert back[R.THRESHOLD].shape == () and back[R.THRESHOLD].tobytes() == w[R.THRESHOLD].tobytes()
    only = T.load_weights(str(tmp_path))[R.THRESHOLD]
    assert only.shape == () and float(only) == float(w[R.THRESHOLD])


# ---- the restatement against hand-built answers ----------------------------------------------------------------------
def _small(B=2, H=16, W=24, seed_window=3):
    img, flow, seg = synth.make_inputs(B, H, W, first_window=seed_window)
    depth = synth.make_depth(B, H, W, first_window=seed_window)
    return img, flow, seg, depth


def _gather(table, seg_plane):
    """table [B,19], labels [B,H,W] -> [B,H,W]: the plain gather, 0 outside [0, 19)"""
    out = np.zeros(seg_plane.shape)
    for b in range(seg_plane.shape[0]):
        for c in range(NUM_SEG_CLASSES):
            out[b][seg_plane[b] == float(c)] = table[b, c]
    return out


def test_constant_depth_gives_the_near_or_the_far_gather():
    cfg = parse_version(FULL)
    img, flow, seg, depth = _small()
    w = synth.make_weights(cfg)
    thr = np.float32(w[R.THRESHOLD])
    near_t, far_t = R.class_tables(cfg, flow, w)
    assert np.abs(near_t[:, 1:] - far_t[:, 1:]).max() > 1e-3           # two different MLPs: the sides can be told apart
    assert np.array_equal(near_t[:, 0], np.ones((2, 19))) and np.array_equal(far_t[:, 0], np.ones((2, 19)))
    for value, tabs in ((float(thr) - 1.0, near_t), (float(thr) + 1.0, far_t), (float(thr), far_t), (np.nan, far_t),
                        (np.nextafter(thr, np.float32(0)), near_t), (np.inf, far_t), (-np.inf, near_t)):
        att = R.attention(cfg, flow, seg, np.full_like(depth, value), w)
        assert np.array_equal(att[0], np.ones_like(att[0]))            # the target's map is ones
        for frame in (1, 2):
            want = _gather(tabs[:, frame], seg[:, R.FRAME_PLANE[frame], :, :, 0])
            assert np.array_equal(att[frame][..., 0], want), (value, frame)


def test_a_depth_equal_to_the_threshold_in_float32_is_far_and_the_compare_is_in_float32():
    thr = np.float32(15.03)
    d = np.array([float(thr), np.nextafter(thr, np.float32(0)), float(thr) - 1e-9, np.nan], np.float64).reshape(1, 1, 1, 4, 1)
    got = R.near_mask(np.repeat(d, 3, axis=1), thr)[0, 0, 0]
    assert got.tolist() == [False, True, False, False]                 # thr - 1e-9 rounds to thr in float32: far


def test_labels_outside_the_classes_give_zero_on_both_sides():
    cfg = parse_version(FULL)
    img, flow, seg, depth = _small()
    w = synth.make_weights(cfg)
    seg = seg.copy()
    seg[:, :, :4] = 255.0
    seg[:, :, 4:8] = 19.0
    seg[:, :, 8:10] = np.nan
    for value in (1.0, 70.0, np.nan):
        att = R.attention(cfg, flow, seg, np.full_like(depth, value), w)
        for frame in (1, 2):
            assert np.array_equal(att[frame][:, :10], np.zeros_like(att[frame][:, :10])), (value, frame)
            assert att[frame][:, 10:].min() > 0.0
        assert np.array_equal(att[0], np.ones_like(att[0]))


@pytest.mark.parametrize("masking", ["-segmask_all", "-segmask_rgb"])
def test_equal_mlps_pack_like_the_flagship_whatever_the_depth(masking):
    version = NET + masking + SUB + "-abs_flow-fc_tanh"
    cfg = parse_version(version)
    img, flow, seg, depth = _small()
    w = synth.make_weights(cfg)
    w = R.with_mlps(w, far=R.mlp_of(w, "se_flow_near"))
    fw = R.flagship_weights(w, "se_flow_near")
    want = O.pack_inputs(parse_version(version.replace(SUB, "-se_flow")), img, flow, seg, fw)
    for d in (depth, depth[:, ::-1].copy(), np.full_like(depth, np.nan)):
        assert np.array_equal(R.pack(cfg, img, flow, seg, d, w), want)
    # ... and with two MLPs the depth does matter, and the target's channels never do
    w2 = synth.make_weights(cfg)
    a, b = R.pack(cfg, img, flow, seg, depth, w2), R.pack(cfg, img, flow, seg, np.full_like(depth, 1.0), w2)
    assert np.abs(a - b)[..., 5:].max() > 1e-3 and np.array_equal(a[..., :5], b[..., :5])
    assert np.array_equal(a[..., :3], want[..., :3])


def test_the_restatement_s_forward_is_the_flagship_s_for_equal_mlps():
    cfg = parse_version(FULL)
    img, flow, seg, depth = _small(B=1, H=16, W=16)
    w = synth.make_weights(cfg)
    w = R.with_mlps(w, far=R.mlp_of(w, "se_flow_near"))
    want = O.forward(R.flagship_cfg(cfg), img, flow, seg, R.flagship_weights(w, "se_flow_near"))
    assert np.array_equal(R.forward(cfg, img, flow, seg, depth, w), want)


# ---- the test inputs exercise both sides -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", SHAPES)
def test_the_synthetic_depth_lies_on_both_sides_of_the_threshold(H, W, B):
    """A condition on the inputs the GPU tests use (synth.make_depth's first windows): on every source plane of every window
    the share of depth < thr is inside 0.3..0.8, at 15.0 and at the threshold synth.make_weights draws.  Measured at 15.0 over
    the four shapes: 0.50..0.735 (the 36x100 shape's third plane pair gives the 0.735)."""
    depth = synth.make_depth(B, H, W)
    at15 = R.near_shares(depth, 15.0)
    print("%dx%d B=%d: share of depth < 15.0 per (window, source plane) %s" % (H, W, B, np.round(at15, 3).tolist()))
    assert at15.shape == (B, 2) and at15.min() >= 0.3 and at15.max() <= 0.8, at15
    drawn = R.near_shares(depth, synth.make_weights(FULL)[R.THRESHOLD])
    assert drawn.min() >= 0.3 and drawn.max() <= 0.8, drawn


# ---- surface ---------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree():
    raw = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    assert re.search(r"\b13 -se_flow_on_depthseg_seplayers\b", raw) and "att_table_far" in raw
    assert "pose_exp_net/se_flow/depth_threshold" in raw and "se_flow_near" in raw and "se_flow_far" in raw
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(davo_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_lib.build())
    for name in sorted(declared):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
    assert set(_lib.EXPORTS) <= declared
    assert ctypes.sizeof(_lib.DavoVariant) == 32                       # still eight ints
    assert ctypes.sizeof(_lib.DavoFeatureOut) == 6 * ctypes.sizeof(ctypes.c_void_p)       # davo_feature_out did not change


def test_the_feature_map_driver_exits_with_a_message_for_this_variant():
    from davo_amd import generate_feature_map as G
    with pytest.raises(SystemExit, match="se_flow_on_depthseg_seplayers"):
        G.main(["--version", FULL, "--synthetic", "3", "--output_dir", os.devnull])
