"""The class-table attention sources (att_source 4..10) on the CPU: version parsing, the float64 restatement the GPU tests
check against, the CLI loader's label planes, and TF bundles with the new scopes."""
import numpy as np
import pytest

from davo_amd import synth
from davo_amd.version import parse_version, weight_shapes, UnsupportedVariantError, NUM_SEG_CLASSES

import class_table_ref as R

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
# substring -> (att_source, C value, tgt_attended, scope, bottleneck kernel shape)
SOURCES = {
    "-se_seg_wo_tgt": ("se_seg_wo_tgt", 4, False, "se_seg", (19, 19)),
    "-se_rgb_wo_tgt_to_seg": ("se_rgb_wo_tgt_to_seg", 5, False, "se_rgb", (3, 8)),
    "-se_rgb_to_seg": ("se_rgb_to_seg", 6, True, "se_rgb", (3, 8)),
    "-se_SegFlow_to_seg_wo_tgt": ("se_SegFlow_to_seg_wo_tgt", 7, False, "se_segflow", (21, 19)),
    "-se_SegFlow_to_seg": ("se_SegFlow_to_seg", 8, True, "se_segflow", (21, 19)),
    "-se_SegFlow_to_seg_8_wo_tgt": ("se_SegFlow_to_seg_8_wo_tgt", 9, False, "se_segflow", (21, 8)),
    "-se_SegFlow_to_seg_8": ("se_SegFlow_to_seg_8", 10, True, "se_segflow", (21, 8)),
}


def _check(cfg, sub, act):
    name, value, tgt, scope, k1 = SOURCES[sub]
    assert cfg.att_source == name and cfg.tgt_attended is tgt and cfg.se_scope == scope
    assert cfg.as_c_ints() == (5, 128, {"relu": 0, "tanh": 1}[act], 0, 0, value, 1, 1)
    sh = weight_shapes(cfg)
    p = "pose_exp_net/%s/" % scope
    se = {k: v for k, v in sh.items() if "/se_" in k}
    assert se == {p + "bottleneck_fc/kernel": k1, p + "bottleneck_fc/bias": (k1[1],),
                  p + "recover_fc/kernel": (k1[1], NUM_SEG_CLASSES), p + "recover_fc/bias": (NUM_SEG_CLASSES,)}
    assert not any("seg_channel_weight" in k for k in sh)
    assert len(sh) == 22 + 4


@pytest.mark.parametrize("sub", sorted(SOURCES))
def test_each_substring_alone(sub):
    _check(parse_version(BASE + sub), sub, "relu")
    _check(parse_version(BASE + sub + "-fc_tanh"), sub, "tanh")


@pytest.mark.parametrize("sub", ["-se_seg_wo_tgt", "-se_rgb_wo_tgt_to_seg"])
def test_published_strings(sub):
    """doc/arch-variants.md:12,14: DAVO (segmentation source) and DAVO (rgb source)."""
    v = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all%s-fc_tanh" % sub
    _check(parse_version(v), sub, "tanh")


def test_v0_and_unmasked_forms():
    c = parse_version("v0-sharedNN-dilatedPoseNN-segmask-se_rgb_to_seg")
    assert (c.cin_per_frame, c.mask_rgb, c.mask_info, c.att_source, c.tgt_attended) == (3, True, False, "se_rgb_to_seg", True)
    assert weight_shapes(c)["pose_exp_net/cnv1/weights"] == (7, 7, 6, 16)
    c = parse_version("v1-sharedNN-dilatedPoseNN-segmask_rgb-se_seg_wo_tgt-norm_flow")
    assert (c.mask_rgb, c.mask_info, c.norm_flow) == (True, False, True)
    c = parse_version("v1-sharedNN-dilatedPoseNN-se_SegFlow_to_seg")
    assert (c.mask_rgb, c.mask_info) == (False, False)


@pytest.mark.parametrize("sub", ["-se_seg", "-se_rgb_wo_tgt", "-se_rgb", "-se_mixSegFlow", "-se_gp2x2_seg", "-se_spp21_mixSegFlow"])
def test_other_sources_still_rejected(sub):
    with pytest.raises(UnsupportedVariantError):
        parse_version(BASE + sub + "-fc_tanh")


def test_existing_tgt_attended_and_scope():
    assert parse_version(BASE + "-static").tgt_attended is False
    assert parse_version(BASE).tgt_attended is True                      # static_all
    c = parse_version(BASE + "-se_flow-abs_flow-fc_tanh")
    assert c.tgt_attended is False and c.se_scope == "se_flow"
    assert parse_version(BASE.replace("segmask_all", "no_segmask")).se_scope is None


# ---- the float64 restatement against hand-built answers ------------------------------------------------------------------
def test_histogram_known_answer():
    seg = np.zeros((1, 4, 8, 1), np.float32)
    flat = seg.reshape(-1)
    flat[:] = [0, 0, 0, 1, 1, 18, 18.9, 255,
               np.nan, -0.5, -1.0, 19.0, 5.5, 5, np.inf, -np.inf,
               3, 3, 3, 3, 3, 3, 3, 3,
               7, 7, 7, 7, 7, 7, 7, 2]
    want = np.zeros(NUM_SEG_CLASSES)
    want[0] = 4          # three zeros and -0.5 (truncated)
    want[1] = 2
    want[18] = 2
    want[5] = 2
    want[3] = 8
    want[7] = 7
    want[2] = 1
    got = R.label_histogram(seg)
    assert np.array_equal(got[0], want / 32.0)                           # 255, NaN, -1, 19, +-inf: zero rows, still in the 32


def test_rgb_descriptor_of_a_constant_colour_strip():
    B, H, W = 2, 4, 8
    img = np.empty((B, H, 3 * W, 3), np.uint8)
    cols = {0: (10, 20, 30), 1: (255, 0, 128), 2: (0, 0, 0)}             # strip slots src0 | tgt | src1
    for k, c in cols.items():
        img[:, :, k * W:(k + 1) * W] = c
    flow = np.zeros((B, 4, H, W, 2), np.float32)
    seg = np.zeros((B, 3, H, W, 1), np.float32)
    d = R.descriptors(parse_version(BASE + "-se_rgb_to_seg"), img, flow, seg)
    for frame, slot in enumerate((1, 0, 2)):
        want = np.array(cols[slot], np.float64) / 255.0 * 2.0 - 1.0
        assert np.allclose(d[:, frame], want, rtol=0, atol=1e-15)


def test_segflow_descriptor_and_tables():
    cfg = parse_version(BASE + "-se_SegFlow_to_seg-norm_flow-abs_flow-fc_tanh")
    img, flow, seg = synth.make_inputs(2, 16, 24)
    d = R.descriptors(cfg, img, flow, seg)
    assert d.shape == (2, 3, 21)
    t0 = abs((0.0 - 0.32140523) / 15.384229)
    assert np.allclose(d[:, 0, 19:], t0, rtol=0, atol=1e-15)            # the target's zeros_like flow, transformed
    want = np.abs((flow[:, 1].astype(np.float64) - 0.32140523) / 15.384229).mean(axis=(1, 2))
    assert np.allclose(d[:, 2, 19:], want, rtol=1e-12)
    assert np.allclose(d[:, :, :19].sum(-1), 1.0 - (seg[:, (1, 0, 2)] == 255).mean(axis=(2, 3, 4)))
    w = synth.make_weights(cfg)
    tab = R.class_tables(cfg, img, flow, seg, w)
    assert tab.shape == (2, 3, 19) and np.all((tab > 0) & (tab < 1))
    wo = parse_version(BASE + "-se_SegFlow_to_seg_wo_tgt-norm_flow-abs_flow-fc_tanh")
    tab_wo = R.class_tables(wo, img, flow, seg, w)
    assert np.array_equal(tab_wo[:, 0], np.ones((2, 19))) and np.array_equal(tab_wo[:, 1:], tab[:, 1:])


def test_zero_kernels_give_the_static_packing():
    """The GPU equivalence tests rest on this: zero kernels and recover_fc/bias = the static weight vector turn the class
    table into the static one, so -se_seg_wo_tgt packs like -static and -se_rgb_to_seg like static_all (-segmask_all)."""
    from oracle import davo_oracle as O
    img, flow, seg = synth.make_inputs(1, 16, 24)
    for sub, static in (("-se_seg_wo_tgt", BASE + "-static"), ("-se_rgb_to_seg", BASE)):
        cfg, scfg = parse_version(BASE + sub), parse_version(static)
        ws = synth.make_weights(scfg)
        w = equivalent_weights(cfg, ws)
        assert np.allclose(R.pack(cfg, img, flow, seg, w), O.pack_inputs(scfg, img, flow, seg, ws), rtol=0, atol=1e-12)


def equivalent_weights(cfg, static_weights):
    w = {k: v for k, v in static_weights.items() if "seg_channel_weight" not in k}
    p = "pose_exp_net/%s/" % cfg.se_scope
    for name, shape in weight_shapes(cfg).items():
        if name.startswith(p):
            w[name] = np.zeros(shape, np.float32)
    w[p + "recover_fc/bias"] = static_weights["pose_exp_net/pose_exp_net/seg_channel_weight/weight"].copy()
    return w


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def test_cli_loader_reads_the_target_label_plane_exactly_when_it_is_attended():
    from davo_amd.run_kitti_pose import loader_seg_planes
    for sub, (_, _, tgt, _, _) in SOURCES.items():
        assert loader_seg_planes(parse_version(BASE + sub)) == ((0, 1, 2) if tgt else None), sub
    assert loader_seg_planes(parse_version(BASE)) == (0, 1, 2)
    for v in (BASE + "-static", BASE + "-se_flow-abs_flow-fc_tanh", BASE.replace("segmask_all", "no_segmask")):
        assert loader_seg_planes(parse_version(v)) is None


@pytest.mark.parametrize("sub", ["-se_seg_wo_tgt", "-se_rgb_to_seg", "-se_SegFlow_to_seg_8"])
def test_tf_bundle_round_trips_the_new_scopes(tmp_path, sub):
    from davo_amd import tf_checkpoint as T
    cfg = parse_version(BASE + sub + "-fc_tanh")
    w = synth.make_weights(cfg)
    T.write_checkpoint(str(tmp_path / "model-1"), w, num_shards=2)
    got = T.load_weights(str(tmp_path))
    assert set(got) == set(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k
    listed = {name: shape for name, shape, _ in T.list_variables(str(tmp_path / "model-1"))}
    for k in w:
        if "/se_" in k:
            assert listed[k] == w[k].shape, k
