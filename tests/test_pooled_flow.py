"""The pooled flow-attention variants (att_source 14..17) without a GPU: the parser, the weight tables, the float64
restatement of tests/pooled_flow_ref.py against hand-built geometry, the library's pool plan (davo_pool_plan) against the
restatement, and - on every input tests/test_pooled_flow_gpu.py uses - the preconditions and the two bars of the GPU tests."""
import numpy as np
import pytest

from davo_amd import synth, parse_version, tf_checkpoint as T
from davo_amd.pool import pool_plan
from davo_amd.version import ATT_SOURCE, FLAGSHIP_VERSION, POOLED_ATT_SOURCE, UnsupportedVariantError, att_source_id, weight_shapes

import layer_check as LC
import pooled_flow_cases as K
import pooled_flow_ref as R

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
STRINGS = {"-se_gp2x2_flow_nobottle": "se_gp2x2_flow_nobottle", "-se_spp21_flow": "se_spp21_flow",
           "-se_spp2_flow": "se_spp2_flow", "-se_spp864_flow": "se_spp864_flow"}
PLAN_SHAPES = [(128, 416), (36, 100), (20, 100), (96, 32), (64, 64), (256, 832)]


# ---- parser -----------------------------------------------------------------------------------------------------------------
def test_the_four_strings_parse():
    for i, (sub, name) in enumerate(STRINGS.items()):
        cfg = parse_version(BASE + sub + "-abs_flow-fc_tanh")
        assert cfg.att_source == name and att_source_id(name) == POOLED_ATT_SOURCE[name] == 14 + i and cfg.as_c_ints()[5] == 14 + i
        assert cfg.se_scope == "se_flow" and not cfg.tgt_attended and not cfg.needs_depth
        assert cfg.abs_mode == "all" and cfg.se_act == "tanh" and cfg.mask_rgb and cfg.mask_info
    assert parse_version(BASE + "-se_spp864_flow-norm_flow-abs_flow_h").abs_mode == "h"


def test_the_elif_order_is_the_references():
    # `-se_flow' is tested before all of them (davo.py:1175), `_nobottle' before the bare gp2x2 string (:1181, 1187)
    for sub in STRINGS:
        assert parse_version(BASE + sub + "-se_flow").att_source == "se_flow"
    assert parse_version(BASE + "-se_gp2x2_flow_nobottle").att_source == "se_gp2x2_flow_nobottle"
    # gp2x2 stands before the spp strings, spp21 before spp2 before spp864
    assert parse_version(BASE + "-se_spp864_flow-se_gp2x2_flow_nobottle").att_source == "se_gp2x2_flow_nobottle"
    assert parse_version(BASE + "-se_spp864_flow-se_spp2_flow").att_source == "se_spp2_flow"
    assert parse_version(BASE + "-se_spp2_flow-se_spp21_flow").att_source == "se_spp21_flow"
    # a class-table source later in the chain loses to a pooled one
    assert parse_version(BASE + "-se_seg_wo_tgt-se_spp2_flow").att_source == "se_spp2_flow"


@pytest.mark.parametrize("sub", ["-se_gp2x2_flow", "-se_spp_flow", "-se_gp2x2_seg", "-se_spp21_seg", "-se_spp_seg_21", "-se_spp2_seg",
                                 "-se_spp_seg", "-se_spp864_seg", "-se_mixSegFlow", "-se_spp21_mixSegFlow",
                                 "-se_gp2x2_flow-se_spp864_flow", "-se_spp_flow-se_spp864_flow"])
def test_the_pinned_and_the_seg_pooling_strings_still_raise(sub):
    with pytest.raises(UnsupportedVariantError):
        parse_version(BASE + sub + "-abs_flow-fc_tanh")
    with pytest.raises(UnsupportedVariantError):
        parse_version(BASE + "-se_insert" + "-se_spp2_flow")


# ---- weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", list(STRINGS))
def test_weight_shapes_synth_weights_and_a_tf_bundle(sub, tmp_path):
    cfg = parse_version(BASE + sub + "-abs_flow-fc_tanh")
    D, nh = R.WIDTHS[cfg.att_source]
    sh = weight_shapes(cfg)
    p = "pose_exp_net/se_flow/"
    assert sh[p + "bottleneck_fc/kernel"] == (D, nh) and sh[p + "bottleneck_fc/bias"] == (nh,)
    assert sh[p + "recover_fc/kernel"] == (nh, 19) and sh[p + "recover_fc/bias"] == (19,)
    assert len(sh) == len(weight_shapes(parse_version(FLAGSHIP_VERSION))) and not any("se_flow_" in k or "seg_channel" in k for k in sh)
    assert D == 2 * len(R.cells(128, 416, cfg.att_source)) == 2 * len(R.cells(36, 100, cfg.att_source))      # D depends on the variant alone
    w = synth.make_weights(cfg)
    assert {k: v.shape for k, v in w.items()} == sh and all(v.dtype == np.float32 for v in w.values())
    T.write_checkpoint(str(tmp_path / "model-3"), w)
    back = T.read_checkpoint(str(tmp_path), verify_crc=True)
    assert set(back) == set(w)
    for k in w:
        assert back[k].shape == w[k].shape and np.array_equal(back[k], w[k]), k
    assert {n: s for n, s, _ in T.list_variables(str(tmp_path))}[p + "bottleneck_fc/kernel"] == (D, nh)


# ---- hand-built geometry ----------------------------------------------------------------------------------------------------
def test_geometry_at_128x416():
    c = R.cells(128, 416, "se_spp864_flow")
    assert len(c) == 64 + 36 + 16
    l8, l6, l4 = c[:64], c[64:100], c[100:]
    assert l8[0][1:] == ((0, 16), (0, 16), 256) and l8[1][2] == (52, 68) and l8[63][1:] == ((112, 128), (364, 380), 256)
    assert l6[0][1:] == ((0, 22), (0, 22), 484) and l6[1][2] == (70, 92) and l6[5][2] == (350, 372)
    assert l6[35][1:] == ((110, 128), (350, 372), 484)             # padded map 132x420: four of the 22 rows are tf.pad's zeros, in the divisor
    assert l4[0][1:] == ((0, 32), (0, 32), 1024) and l4[1][2] == (104, 136) and l4[15][1:] == ((96, 128), (312, 344), 1024)
    c21 = R.cells(128, 416, "se_spp21_flow")
    assert len(c21) == 5 and c21[4][1:] == ((0, 128), (0, 128), 128 * 128)      # the level-1 cell is columns [0, 128) only
    c2 = R.cells(128, 416, "se_spp2_flow")
    assert [x[2] for x in c2] == [(0, 64), (208, 272), (0, 64), (208, 272)] and [x[1] for x in c2] == [(0, 64), (0, 64), (64, 128), (64, 128)]
    assert all(x[3] == 64 * 64 for x in c2) and c21[:4] == c2
    g = R.cells(128, 416, "se_gp2x2_flow_nobottle")
    assert [x[1:] for x in g] == [((0, 64), (0, 208), 13312), ((0, 64), (208, 416), 13312), ((64, 128), (0, 208), 13312), ((64, 128), (208, 416), 13312)]
    # most of a landscape frame lies outside every window
    assert R.outside_mask(128, 416, "se_spp2_flow").mean() > 0.6 and R.outside_mask(128, 416, "se_spp864_flow").mean() > 0.3
    assert not R.outside_mask(128, 416, "se_gp2x2_flow_nobottle").any()


def test_geometry_at_36x100_and_20x100_and_a_portrait():
    l8 = R.level_cells(36, 100, 8)
    assert l8[0][1:] == ((0, 5), (0, 5), 25) and l8[1][2] == (13, 18)                    # hs 5, ws 13
    assert all(c[1] == (35, 36) and c[3] == 25 for c in l8[56:])                          # the last cell row holds one real row
    l8 = R.level_cells(20, 100, 8)
    assert l8[0][1:] == ((0, 3), (0, 3), 9) and l8[48][1] == (18, 20)                     # hs 3; row 6 holds two real rows
    assert all(c[1:] == ((0, 0), (0, 0), 9) for c in l8[56:])                             # row 7 = rows [21, 24): wholly in padding
    for transform in ("-abs_flow", "-norm_flow", "-norm_flow-abs_flow"):
        cfg = parse_version(R.version("se_spp864_flow", transform=transform))
        flow = K.inputs(2, 20, 100)[1]
        for dtype in (np.float64, np.float32):
            d = R.descriptor(cfg, flow, dtype)
            assert np.array_equal(d[:, :, 2 * 56:2 * 64], np.zeros((2, 2, 16), dtype)) and np.abs(d[:, :, :2 * 56]).min() > 0
        assert np.array_equal(R.literal_descriptor(R.transformed(cfg, flow)[1, 0], cfg.att_source)[2 * 56:2 * 64], np.zeros(16))
    # portrait 96x32, level 2: hs 48, ws 16, SAME column padding 32 = 16 | 16; divisor 48 x 32 (the map's own columns)
    l2 = R.level_cells(96, 32, 2)
    assert l2[0][1:] == ((0, 48), (0, 32), 48 * 32) and l2[1][1:] == ((0, 48), (0, 32), 48 * 32)
    assert l2[2][1:] == ((48, 96), (0, 32), 48 * 32) and l2[3][1:] == ((48, 96), (0, 32), 48 * 32)
    l4 = R.level_cells(96, 32, 4)                                                         # hs 24, ws 8, left 8: cell j covers [8 j - 8, 8 j + 16)
    assert [c[2] for c in l4[:4]] == [(0, 16), (0, 24), (8, 32), (16, 32)] and [c[3] for c in l4[:4]] == [24 * 16, 24 * 24, 24 * 24, 24 * 16]


@pytest.mark.parametrize("H,W", PLAN_SHAPES)
@pytest.mark.parametrize("src", K.SOURCES)
def test_the_cells_are_the_references_own_steps(src, H, W):
    """tf.pad + avg_pool SAME + reshape, stated literally, gives the descriptor the cell list gives."""
    if H * W > 128 * 416:
        pytest.skip("the literal pooling is slow there; the cell list is checked against the plan at that size")
    rng = np.random.RandomState(H * 1000 + W)
    t = rng.standard_normal((H, W, 2))
    want = R.literal_descriptor(t, src)
    cs = R.cells(H, W, src)
    got = np.concatenate([t[y[0]:y[1], x[0]:x[1]].sum(axis=(0, 1)) / div for _, y, x, div in cs])
    assert want.shape == got.shape == (R.WIDTHS[src][0],) and np.abs(want - got).max() < 1e-12


# ---- the library's plan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", PLAN_SHAPES)
@pytest.mark.parametrize("src", K.SOURCES)
def test_davo_pool_plan_is_the_restatements_cells(src, H, W):
    rects, inv = pool_plan(H, W, src)
    want_r, want_i = R.plan_arrays(H, W, src)
    assert rects.shape == want_r.shape == (R.WIDTHS[src][0] // 2, 4) and np.array_equal(rects, want_r)
    assert np.array_equal(inv.view(np.uint32), want_i.view(np.uint32))
    assert (rects[:, 0] >= 0).all() and (rects[:, 1] <= H).all() and (rects[:, 2] >= 0).all() and (rects[:, 3] <= W).all()


def test_davo_pool_plan_reports_no_cells_for_sources_that_do_not_pool():
    assert sorted(ATT_SOURCE.values()) == list(range(14)) and sorted(POOLED_ATT_SOURCE.values()) == [14, 15, 16, 17]
    for name, a in ATT_SOURCE.items():
        if a < 14:
            rects, inv = pool_plan(128, 416, name)
            assert rects.shape == (0, 4) and inv.shape == (0,), name
    assert pool_plan(128, 416, parse_version(FLAGSHIP_VERSION).att_source)[0].shape == (0, 4)
    for bad in ((0, 416, 14), (128, 0, 14), (128, 416, -1), (128, 416, 18)):
        with pytest.raises(ValueError):
            pool_plan(*bad)


def test_the_frame_layout_plans_them_as_se_flow():
    """davo_frames_plan_fmt: the same planes and the same bytes as -se_flow, whatever the selection and the formats (the older
    davo_frames_plan keeps the range 0..13 it was published with; davo_amd.frames_plan picks the form)."""
    from davo_amd import frames_plan
    for src in K.SOURCES:
        for pairs in ("both", "src0", "src1"):
            for labels, flow in (("f32", "f32"), ("u8", "f16")):
                assert frames_plan(128, 416, 5, pairs, src, labels, flow) == frames_plan(128, 416, 5, pairs, "se_flow", labels, flow)
        assert frames_plan(36, 100, 3, "both", att_source_id(src)) == frames_plan(36, 100, 3, "both", "se_flow")
    with pytest.raises(ValueError):
        frames_plan(36, 100, 3, "both", 18)


def test_spp2_and_gp2x2_have_the_same_cells_at_64x64():
    a, b = pool_plan(64, 64, "se_spp2_flow"), pool_plan(64, 64, "se_gp2x2_flow_nobottle")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    assert [c[1:] for c in R.cells(64, 64, "se_spp2_flow")] == [c[1:] for c in R.cells(64, 64, "se_gp2x2_flow_nobottle")]
    assert not np.array_equal(pool_plan(128, 416, "se_spp2_flow")[0], pool_plan(128, 416, "se_gp2x2_flow_nobottle")[0])


# ---- every input of the GPU tests -------------------------------------------------------------------------------------------
def test_the_raw_synthetic_flow_would_not_do():
    """mean |flow| near 12.5 saturates the bottleneck: the reason the cases use pooled_flow_ref.make_flow."""
    raw = synth.make_inputs(1, 36, 100)[1]
    assert 11.5 < np.abs(raw).mean() < 13.5
    assert 0.5 < np.abs(K.inputs(3, 36, 100)[1]).mean() < 2.0


@pytest.mark.parametrize("case", K.layer_cases(), ids=K.case_id)
def test_preconditions_and_bars_hold_on_the_gpu_tests_inputs(case):
    """Before any device result: the table tells where the flow sits (pooled_flow_ref.check_preconditions), and the restatement
    in float32 with numpy's pairwise sums meets both GPU bars on these inputs - `se_desc' within 2^-20 x sum|t(flow)| x inv_div
    per entry, the table rows within layer_check.TABLE_TOL - with the margins printed.  Margins measured here: the table bar keeps
    9x or more everywhere; the `se_desc' bar 4.2x or more at every case but se_spp864_flow at 64x64, where it is 3.55x - there the
    bar is widened to 4x the float32 restatement's error (pooled_flow_cases.DESC_BAR_FACTOR: 1.13), and only there."""
    src, masking, act, transform, H, W, B = case
    cfg, w = K.config(case)
    flow = K.inputs(B, H, W)[1]
    figures = R.check_preconditions(cfg, flow, w, LC.TABLE_TOL, need_outside=K.has_outside(src, H, W))
    d64, d32 = R.descriptor(cfg, flow), R.descriptor(cfg, flow, np.float32)
    bar = R.descriptor_bar(cfg, flow)
    err = np.abs(d32.astype(np.float64) - d64)
    live = bar > 0
    assert np.array_equal(err[~live], np.zeros((~live).sum()))                  # empty cells: exactly 0
    desc_margin = float((bar[live] / np.maximum(err[live], 1e-300)).min())
    factor = K.desc_bar_factor(src, H, W)
    assert factor == 1.0 or (desc_margin < 4.0 and factor <= 1.02 * 4.0 / desc_margin), (factor, desc_margin)      # widened only where it must be, to 4x
    desc_margin *= factor
    t64 = R.tables_from_descriptor(cfg, d64, w)
    t32 = R.tables_from_descriptor(cfg, d32, w, np.float32)
    tab_err = float(np.abs(t32.astype(np.float64) - t64)[:, 1:].max())
    tab_margin = LC.TABLE_TOL / max(tab_err, 1e-300)
    print("%s: preconditions %s; float32 restatement: se_desc margin %.1fx, table err %.3g (margin %.1fx)" % (
        K.case_id(case), figures, desc_margin, tab_err, tab_margin))
    assert desc_margin >= 4.0 and tab_margin >= 4.0, (desc_margin, tab_margin)


@pytest.mark.parametrize("src", K.ENTRY_SOURCES + ["se_spp2_flow", "se_spp21_flow"])
def test_preconditions_hold_on_the_entry_point_inputs(src):
    H, W, B = K.ENTRY_SHAPE
    cfg, w = K.config((src, "-segmask_all", "-fc_tanh", "-abs_flow"))
    for first in (0, 7):
        R.check_preconditions(cfg, K.inputs(B, H, W, first)[1], w, LC.TABLE_TOL)
    from davo_amd import flow_to_f16
    R.check_preconditions(cfg, flow_to_f16(K.inputs(B, H, W)[1]).astype(np.float32), w, LC.TABLE_TOL)
