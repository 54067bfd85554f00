"""The three-frame PoseNN (`-dilatedPoseNN' without `-sharedNN', decouple_net_v0_dilation) without a GPU: the parser, the
variables, the float64 restatement of tests/three_frame_ref.py against the oracle package, the conditions the GPU cases' inputs
must meet, and the C surface.  The library against the restatement: tests/test_three_frame_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from davo_amd import _lib, synth
from davo_amd.version import FLAGSHIP_VERSION, UnsupportedVariantError, parse_version, weight_shapes
from oracle import davo_oracle as O

import feature_attention_cases as FA
import pooled_flow_ref as PF
import three_frame_cases as K
import three_frame_ref as T
from helpers import ABS_TOL, REL_TOL, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- parser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", K.VERSIONS)
def test_the_three_frame_versions_parse(version):
    cfg = parse_version(version)
    assert cfg.posenn == "triplet" and cfg.posenn_se == "none" and not cfg.needs_depth
    twin = parse_version(version.replace("-dilatedPoseNN", "-sharedNN-dilatedPoseNN"))
    assert twin.posenn == "pairs" and twin.as_c_ints() == cfg.as_c_ints()        # the eight ABI fields do not carry the topology


def test_the_other_sources_that_end_in_a_class_table_parse_too():
    for sub in ("-se_seg_wo_tgt", "-se_rgb_wo_tgt_to_seg", "-se_SegFlow_to_seg_wo_tgt", "-se_SegFlow_to_seg", "-se_SegFlow_to_seg_8_wo_tgt",
                "-se_SegFlow_to_seg_8", "-se_gp2x2_flow_nobottle", "-se_spp21_flow", "-se_spp2_flow", "-se_spp864_flow"):
        assert parse_version(K.BASE + "-segmask_all" + sub + "-fc_tanh").posenn == "triplet", sub


@pytest.mark.parametrize("version", K.REJECTED)
def test_the_neighbouring_strings_still_raise(version):
    with pytest.raises(UnsupportedVariantError):
        parse_version(version)


def test_the_rejections_name_their_reference_function_or_reason():
    for version, word in (("v1-dilatedCouplePoseNN-no_segmask", "couple_net_v0_dilation"), ("v1-couplePoseNN-no_segmask", "couple_net_v0"),
                          ("v1-no_segmask", "decouple_net_v0"), ("v1-dilatedPoseNN-se_flow", "never read"),
                          ("v1-dilatedPoseNN-no_segmask-se_insert", "se_insert"), (K.BASE + "-segmask_all-se_depth_to_seg", "depth")):
        with pytest.raises(UnsupportedVariantError, match=word):
            parse_version(version)


# (version, major, att_source, as_c_ints, posenn_se) as the parser returned them before the topology existed: the golden cases'
# strings, the flagship, and the strings the other variants' test modules are built on
PAIR_CONFIGS = [
    ('v0-sharedNN-dilatedPoseNN-segmask-se_flow-abs_flow-fc_tanh', 'v0', 'se_flow', (3, 128, 1, 0, 3, 1, 1, 0), 'none'),
    (FLAGSHIP_VERSION, 'v1', 'se_flow', (5, 128, 1, 0, 3, 1, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-cnv6_64-no_segmask', 'v1', 'ones', (5, 64, 0, 0, 0, 0, 0, 0), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_all', 'v1', 'static_all', (5, 128, 0, 0, 0, 3, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_all-se_flow-norm_flow-abs_flow_h', 'v1', 'se_flow', (5, 128, 0, 1, 1, 1, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_all-static', 'v1', 'static_src', (5, 128, 0, 0, 0, 2, 1, 1), 'none'),
    ('v1-sharedNN-dilatedPoseNN-segmask_rgb-se_flow-fc_lrelu-abs_flow_v', 'v1', 'se_flow', (5, 128, 2, 0, 2, 1, 1, 0), 'none'),
    (FA.PUBLISHED, 'v1', 'ones', (5, 128, 0, 0, 0, 0, 0, 0), 'insert'),
    (FA.PLAIN, 'v1', 'ones', (5, 128, 0, 0, 0, 0, 0, 0), 'none'),
    (PF.version("se_spp864_flow"), 'v1', 'se_spp864_flow', (5, 128, 1, 0, 3, 17, 1, 1), 'none'),
    (PF.version("se_gp2x2_flow_nobottle"), 'v1', 'se_gp2x2_flow_nobottle', (5, 128, 1, 0, 3, 14, 1, 1), 'none'),
]


def test_every_pair_network_string_parses_as_before():
    listed = {g[0]: g[1:] for g in PAIR_CONFIGS}
    assert {case["version"] for case in load_golden()["cases"].values()} <= set(listed)
    for v in sorted(listed):
        cfg = parse_version(v)
        assert (cfg.major, cfg.att_source, cfg.as_c_ints(), cfg.posenn_se) == listed[v], v
        assert cfg.posenn == "pairs", v
        sh = weight_shapes(cfg)
        assert sh["pose_exp_net/cnv1/weights"] == (7, 7, 2 * cfg.cin_per_frame, 16)
        assert sh["pose_exp_net/pose/rotation/pred/weights"] == (1, 1, 256, 3) and sh["pose_exp_net/pose/translation/pred/biases"] == (3,)


# ---- weights ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version,cin", [(K.FLAGSHIP3, 15), (K.VERSIONS[5], 9)])
def test_weight_shapes_and_synthetic_weights(version, cin):
    cfg = parse_version(version)
    sh = weight_shapes(cfg)
    twin = weight_shapes(parse_version(version.replace("-dilatedPoseNN", "-sharedNN-dilatedPoseNN")))
    assert set(sh) == set(twin)                                 # the same variables under the same names
    changed = {n for n in sh if sh[n] != twin[n]}
    assert changed == {"pose_exp_net/cnv1/weights"} | {"pose_exp_net/pose/%s/pred/%s" % (h, t) for h in T.HEADS for t in ("weights", "biases")}
    assert sh["pose_exp_net/cnv1/weights"] == (7, 7, cin, 16)
    for h in T.HEADS:
        assert sh["pose_exp_net/pose/%s/pred/weights" % h] == (1, 1, 256, 6) and sh["pose_exp_net/pose/%s/pred/biases" % h] == (6,)
    w = synth.make_weights(cfg)
    assert {n: tuple(a.shape) for n, a in w.items()} == sh and all(a.dtype == np.float32 for a in w.values())


def test_tf_bundle_round_trip(tmp_path):
    from davo_amd import tf_checkpoint as C
    cfg = parse_version(K.FLAGSHIP3)
    w = synth.make_weights(cfg)
    prefix = str(tmp_path / "model-3f")
    C.write_checkpoint(prefix, w)
    back = C.load_weights(prefix)
    assert set(back) == set(w) == set(weight_shapes(cfg))
    for n in w:
        assert back[n].shape == w[n].shape and np.array_equal(back[n], w[n]), n
    assert back["pose_exp_net/cnv1/weights"].shape == (7, 7, 15, 16) and back["pose_exp_net/pose/rotation/pred/weights"].shape == (1, 1, 256, 6)


# ---- the restatement against the oracle package ---------------------------------------------------------------------------
# Bar of the two identities: only the summation order of a float64 sum of K <= 2,304 terms differs between the two networks (cnv1's
# zero channels add exact zeros; every other layer is the same call on the same values up to that), so the difference is a few
# units of 2,304 * 2^-53 = 2.6e-13 of a layer's mass, carried through seven layers: 1e-10 of max|pose| leaves two orders of room.
IDENTITY_REL = 1e-10


@pytest.mark.parametrize("s", [0, 1])
def test_one_source_alone_is_the_pair_network(s):
    H, W, B = 36, 100, 2
    cfg3, inp, w = K.case(H, W, B)
    cfg2 = parse_version(K.FLAGSHIP3.replace("-dilatedPoseNN", "-sharedNN-dilatedPoseNN"))
    pair = synth.make_weights(cfg2)
    pair_pred = {h: (pair["pose_exp_net/pose/%s/pred/weights" % h], pair["pose_exp_net/pose/%s/pred/biases" % h]) for h in T.HEADS}
    w3, w2 = T.restricted(cfg3, cfg2, w, s, pair_pred)
    got = T.forward(cfg3, *inp, w3)[:, s]
    want = O.forward(cfg2, *inp, w2, np.float64)[:, s]
    scale = np.abs(want).max()
    assert scale > 1e-3
    assert np.abs(got - want).max() <= IDENTITY_REL * scale, (np.abs(got - want).max(), scale)
    # ... and the identity is about THIS source: the other row of the same restricted network is another pose
    assert np.abs(T.forward(cfg3, *inp, w3)[:, 1 - s] - want).max() > 1e-3 * scale


def test_the_reshape_against_a_hand_built_avg():
    rot = np.array([[1., 2., 3., 4., 5., 6.], [7., 8., 9., 10., 11., 12.]])
    trans = -rot
    p = T.reshape_poses(rot, trans)
    assert p.shape == (2, 2, 6)
    assert np.allclose(p[0, 0], 0.01 * np.array([1, 2, 3, -1, -2, -3])) and np.allclose(p[0, 1], 0.01 * np.array([4, 5, 6, -4, -5, -6]))
    assert np.allclose(p[1, 1], 0.01 * np.array([10, 11, 12, -10, -11, -12]))
    for b in range(2):
        for s in range(2):
            for head, avg in enumerate((rot, trans)):
                for k in range(3):
                    assert p[b, s, 3 * head + k] == 0.01 * avg[b, 3 * s + k]


def test_pack15_channel_order_and_the_packed_sixteen():
    H, W, B = 16, 16, 3
    cfg, (img, flow, seg), w = K.case(H, W, B)
    x = T.pack15(cfg, img, flow, seg, w)
    att = T.attention_maps(cfg, img, flow, seg, w)
    rgb = O.preprocess_image(img, np.float64)
    assert np.array_equal(x[..., 0:3], rgb[:, :, W:2 * W] * att[0]) and np.all(x[..., 3:5] == 0)
    assert np.array_equal(x[..., 5:8], rgb[:, :, :W] * att[1]) and np.array_equal(x[..., 8:10], flow[:, 0].astype(np.float64) * att[1])
    assert np.array_equal(x[..., 10:13], rgb[:, :, 2 * W:] * att[2]) and np.array_equal(x[..., 13:15], flow[:, 1].astype(np.float64) * att[2])
    assert np.all(att[0] == 1.0)                                # se_flow: the target's map is ones
    p = T.pack16(x, cfg)
    assert np.array_equal(p[..., :13], x[..., T.REAL_CHANNELS[5]]) and np.all(p[..., 13:] == 0)
    # cnv1 on the 16 packed channels with the re-indexed kernel is cnv1 on the 15
    w1, b1 = w["pose_exp_net/cnv1/weights"], w["pose_exp_net/cnv1/biases"]
    a = O.conv2d_same(x, w1.astype(np.float64), b1.astype(np.float64), 2, 1)
    b = O.conv2d_same(p, T.cnv1_weights16(w1.astype(np.float64), cfg), b1.astype(np.float64), 2, 1)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


# ---- conditions on the inputs of every GPU case ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", K.SHAPES, ids=K.IDS)
def test_every_channel_and_both_rows_show_in_the_poses(H, W, B):
    """A library that dropped, swapped or zeroed one of the 13 real input channels, or returned one source's pose in both rows,
    must miss the parity bar by far: zeroing cnv1's weights on any one channel moves the pose by more than 100 x the bar."""
    cfg, inp, w = K.case(H, W, B)
    x = T.pack15(cfg, *inp, w)
    want = K.reference(H, W, B)
    scale = np.abs(want).max()
    bar = min(ABS_TOL, REL_TOL * scale)
    assert np.abs(want[:, 0] - want[:, 1]).max() > 100 * bar
    seen = inp[2][0].reshape(3, -1)
    assert all(set(range(19)) | {255} <= set(np.unique(seen[p]).astype(int)) for p in range(3))
    for ch in T.REAL_CHANNELS[cfg.cin_per_frame]:
        wz = dict(w)
        k1 = np.array(w["pose_exp_net/cnv1/weights"])
        k1[:, :, ch] = 0
        wz["pose_exp_net/cnv1/weights"] = k1
        moved = np.abs(T.forward(cfg, *inp, wz, x=x) - want).max()
        assert moved > 100 * bar, (ch, moved, bar)


# ---- C surface --------------------------------------------------------------------------------------------------------
def test_header_binding_and_exported_symbol():
    src = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    assert re.search(r"\bint\s+davo_set_posenn_topology\s*\(\s*davo_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", src)
    assert re.search(r"DAVO_POSENN_PAIRS\s*=\s*0\s*,\s*DAVO_POSENN_TRIPLET\s*=\s*1", src)
    assert "davo_set_posenn_topology" in _lib.EXPORTS and (_lib.POSENN_PAIRS, _lib.POSENN_TRIPLET) == (0, 1)
    L = ctypes.CDLL(_lib.build())
    assert hasattr(L, "davo_set_posenn_topology")
    assert "patch_cnv1_t" in src


def test_the_cli_refuses_one_pair_runs_of_a_three_frame_version(capsys):
    from davo_amd import run_kitti_pose
    with pytest.raises(SystemExit) as exc:
        run_kitti_pose.main(["--test_seq", "9", "--output_dir", "unused", "--synthetic", "5", "--version", K.FLAGSHIP3, "--pairs", "trajectory"])
    assert exc.value.code == 2
    assert "three-frame" in capsys.readouterr().err
