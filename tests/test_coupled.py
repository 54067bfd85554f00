"""The coupled shared PoseNN (`-sharedNN-dilatedCouplePoseNN', couple_sharednet_v0_dilation; davo_set_posenn_heads) without a GPU:
the parser, the variables, the float64 restatement of tests/coupled_ref.py against the oracle package by the duplicated-head
identity, the conditions the GPU cases' inputs must meet, the plan table and the C surface.  The library against the restatement:
tests/test_coupled_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest

from davo_amd import _lib, synth
from davo_amd.version import UnsupportedVariantError, parse_version, weight_shapes
from oracle import davo_oracle as O

import coupled_cases as K
import coupled_ref as C
from helpers import ABS_TOL, REL_TOL
from test_abi import built      # noqa: F401  (the module's fixture: builds the library where it is missing)
from test_three_frame import IDENTITY_REL, PAIR_CONFIGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_VARS = {"pose_exp_net/pose/cnv6/weights", "pose_exp_net/pose/cnv6/biases", "pose_exp_net/pose/cnv7/weights",
             "pose_exp_net/pose/cnv7/biases", "pose_exp_net/pose/pred/weights", "pose_exp_net/pose/pred/biases"}


# ---- parser ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", K.VERSIONS)
def test_the_coupled_versions_parse(version):
    cfg = parse_version(version)
    assert cfg.heads == "coupled" and cfg.posenn == "pairs" and cfg.posenn_se == "none"
    twin = parse_version(version.replace("-dilatedCouplePoseNN", "-dilatedPoseNN"))
    assert twin.heads == "decoupled" and twin.as_c_ints() == cfg.as_c_ints()     # the eight ABI fields do not carry the heads
    assert (twin.att_source, twin.mask_rgb, twin.mask_info, twin.major) == (cfg.att_source, cfg.mask_rgb, cfg.mask_info, cfg.major)


def test_the_depth_split_and_the_other_pooled_sources_parse_too():
    for sub in ("-se_flow_on_depthseg_seplayers_12.5", "-se_depth_wo_tgt_to_seg", "-se_gp2x2_flow_nobottle", "-se_spp2_flow", "-se_spp864_flow",
                "-se_seg_wo_tgt", "-se_SegFlow_to_seg_8"):
        cfg = parse_version(K.BASE + "-segmask_all" + sub + "-fc_tanh")
        assert cfg.heads == "coupled" and cfg.posenn == "pairs", sub


@pytest.mark.parametrize("width", K.WIDTHS)
def test_each_width_parses(width):
    cfg = parse_version(K.version(width))
    assert cfg.heads == "coupled" and cfg.cnv6_out == width
    assert parse_version(K.FLAGSHIP_C.replace("-cnv6_128", "")).cnv6_out == 128          # the default


@pytest.mark.parametrize("version,word", K.REJECTED)
def test_the_rejected_neighbours_raise_with_their_reason(version, word):
    with pytest.raises(NameError, match=word) as exc:
        parse_version(version)
    if "-sharedNN-couplePoseNN" not in version:                  # the reference's own NameError keeps its type and message
        assert isinstance(exc.value, UnsupportedVariantError)
    for sub in ("-se_skipadd", "-se_replace"):
        with pytest.raises(UnsupportedVariantError):
            parse_version(K.BASE + "-no_segmask" + sub)


def test_every_pair_network_string_is_still_decoupled():
    for version, major, att_source, c_ints, posenn_se in PAIR_CONFIGS:
        cfg = parse_version(version)
        assert cfg.heads == "decoupled" and cfg.posenn == "pairs", version
        assert (cfg.major, cfg.att_source, cfg.as_c_ints(), cfg.posenn_se) == (major, att_source, c_ints, posenn_se), version
        assert not HEAD_VARS & set(weight_shapes(cfg))


# ---- variables ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", K.WIDTHS)
def test_weight_shapes_and_synthetic_weights(width):
    cfg = parse_version(K.version(width))
    sh = weight_shapes(cfg)
    twin = weight_shapes(parse_version(K.version(width).replace("-dilatedCouplePoseNN", "-dilatedPoseNN")))
    assert set(sh) - set(twin) == HEAD_VARS and not any("/rotation/" in n or "/translation/" in n for n in sh)
    assert {n: sh[n] for n in set(sh) & set(twin)} == {n: twin[n] for n in set(sh) & set(twin)}      # the trunk and the SE scope
    p = "pose_exp_net/pose/"
    assert sh[p + "cnv6/weights"] == (3, 3, 256, width) and sh[p + "cnv6/biases"] == (width,)
    assert sh[p + "cnv7/weights"] == (3, 3, width, 256) and sh[p + "cnv7/biases"] == (256,)
    assert sh[p + "pred/weights"] == (1, 1, 256, 6) and sh[p + "pred/biases"] == (6,)
    w = synth.make_weights(cfg)
    assert {n: tuple(a.shape) for n, a in w.items()} == sh and all(a.dtype == np.float32 for a in w.values())


def test_a_variant_without_an_se_scope_has_sixteen_variables():
    assert len(weight_shapes(parse_version(K.BASE + "-no_segmask"))) == 16
    assert len(weight_shapes(parse_version(K.FLAGSHIP_C))) == 20


def test_tf_bundle_round_trip(tmp_path):
    from davo_amd import tf_checkpoint as T
    cfg = parse_version(K.FLAGSHIP_C)
    w = synth.make_weights(cfg)
    prefix = str(tmp_path / "model-coupled")
    T.write_checkpoint(prefix, w)
    back = T.load_weights(prefix)
    assert set(back) == set(w) == set(weight_shapes(cfg))
    for n in w:
        assert back[n].shape == w[n].shape and np.array_equal(back[n], w[n]), n
    assert back["pose_exp_net/pose/pred/weights"].shape == (1, 1, 256, 6) and back["pose_exp_net/pose/cnv7/weights"].shape == (3, 3, 128, 256)


# ---- the restatement against the oracle package: the duplicated-head identity -----------------------------------------------
# tests/test_three_frame.py's bar of its one-source identities: the two networks differ in the order of float64 sums of K <= 2,304
# terms (here: pred's 256 terms split over two heads, everything else the same call on the same values)
@pytest.mark.parametrize("version", [K.FLAGSHIP_C, K.version(32), K.BASE + "-segmask_all-se_rgb_to_seg-fc_tanh"])
def test_duplicated_heads_are_the_coupled_network(version):
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B, version)
    dversion, dw = C.duplicated(cfg, w)
    dcfg = parse_version(dversion)
    assert dcfg.heads == "decoupled" and {n: tuple(np.shape(a)) for n, a in dw.items()} == weight_shapes(dcfg)
    got = C.forward(cfg, *inp, w)
    x = C.pack(dcfg, *inp, dw)
    want = O.posenet(x.reshape((2 * B,) + x.shape[2:]), {n: np.asarray(a, np.float64) for n, a in dw.items()}).reshape(B, 2, 6)
    if dcfg.att_source in ("ones", "se_flow", "static_src", "static_all"):
        assert np.array_equal(want, O.forward(dcfg, *inp, dw, np.float64))       # the oracle's own forward, where it has the source
    scale = np.abs(want).max()
    assert scale > 1e-3
    assert np.abs(got - want).max() <= IDENTITY_REL * scale, (np.abs(got - want).max(), scale)


# ---- conditions on the inputs of every GPU case, on the restatement alone ----------------------------------------------------
@pytest.mark.parametrize("H,W,B", K.SHAPES, ids=K.IDS)
def test_preconditions_of_the_gpu_cases(H, W, B):
    """A library that dropped a pred column, read half of cnv6 in cnv7 (as a group would), swapped the rotation and translation
    columns or ran the decoupled network must miss the parity bar by far."""
    cfg, inp, w = K.case(H, W, B)
    keep = {}
    want = C.forward(cfg, *inp, w, keep=keep)
    assert np.array_equal(want, K.reference(H, W, B))
    scale = np.abs(want).max()
    bar = min(ABS_TOL, REL_TOL * scale)
    seen = inp[2][0].reshape(3, -1)
    assert all(set(range(19)) | {255} <= set(np.unique(seen[p]).astype(int)) for p in range(3))
    cnv5 = keep["cnv5"]
    # each of the six pred columns moves its pose component
    for k in range(6):
        wz = dict(w)
        pw = np.array(w["pose_exp_net/pose/pred/weights"])
        pw[..., k] = 0
        wz["pose_exp_net/pose/pred/weights"] = pw
        moved = np.abs(C.pose_from_cnv7(keep["cnv7"], wz).reshape(B, 2, 6) - want)
        assert moved[..., k].max() > 100 * bar and np.delete(moved, k, axis=-1).max() == 0, (k, moved.max(), bar)
    # zeroing the upper half of cnv6's channels changes the poses: a cnv7 that read only the lower half would show
    wz = dict(w)
    k7 = np.array(w["pose_exp_net/pose/cnv7/weights"])
    k7[:, :, cfg.cnv6_out // 2:] = 0
    wz["pose_exp_net/pose/cnv7/weights"] = k7
    assert np.abs(C.head(cnv5, wz).reshape(B, 2, 6) - want).max() > 100 * bar
    # the columns 0..2 and 3..5 are not interchangeable
    assert np.abs(want[..., [3, 4, 5, 0, 1, 2]] - want).max() > 100 * bar
    # ... and the decoupled network on the same-shaped synthetic weights is another network
    dcfg = parse_version(cfg.version.replace("-dilatedCouplePoseNN", "-dilatedPoseNN"))
    other = O.forward(dcfg, *inp, synth.make_weights(dcfg), np.float64)
    assert np.abs(other - want).max() > 100 * bar
    # the two rows of a window are different poses
    assert np.abs(want[:, 0] - want[:, 1]).max() > 100 * bar


# ---- the plan table --------------------------------------------------------------------------------------------------------
def _planners(path):
    L = ctypes.CDLL(path)
    ip = ctypes.POINTER(ctypes.c_int)
    L.davo_plan_layer.argtypes = [ctypes.c_int] * 3 + [ip] * 3
    L.davo_plan_layer_f32.argtypes = [ctypes.c_int] * 4 + [ip] * 3

    def h3(M, N):
        rows, bm, bn = (ctypes.c_int * 2)(), (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
        n = L.davo_plan_layer(M, N, 1, rows, bm, bn)
        assert n in (1, 2), (M, N, n)
        return tuple(K.TILE_ID[(bm[i], bn[i])] for i in range(n))

    def f32(M, N):
        m0, mt, bn = (ctypes.c_int * 2)(), (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
        n = L.davo_plan_layer_f32(-(-M // 128), N, 1, 256, m0, mt, bn)
        assert n in (1, 2), (M, N, n)
        return tuple(bn[i] for i in range(n))
    return h3, f32


def _uncovered(plan, table, differs=None):
    out = []
    for width in K.WIDTHS:
        listed = {c[1:] for c in table[width]}
        for B in K.PLAN_BATCHES:
            g6, g7 = K.gemms(width, B)
            tiles = (plan(*g6), plan(*g7))
            if differs and width == 256 and B in differs:
                assert tiles[0] == differs[B], (B, tiles)
                continue
            if tiles not in listed:
                listed.add(tiles)
                out.append((width, B) + tiles)
    return out


def test_every_f16x3_plan_has_a_gpu_case(built):      # noqa: F811
    h3, _ = _planners(built)
    missing = _uncovered(h3, K.PLAN_CASES, K.PLANNER_DIFFERS_256)
    assert not missing, "(cnv6, cnv7) plans without a case in tests/coupled_cases.py (width, first B, cnv6, cnv7): %s" % missing
    for width in K.WIDTHS:                              # ... and every listed case is the planner's at its batch size
        for B, t6, t7 in K.PLAN_CASES[width]:
            g6, g7 = K.gemms(width, B)
            if not (width == 256 and B in K.PLANNER_DIFFERS_256):
                assert (h3(*g6), h3(*g7)) == (t6, t7), (width, B)


def test_every_f32_plan_has_a_gpu_case(built):      # noqa: F811
    _, f32 = _planners(built)
    missing = _uncovered(f32, K.F32_CASES)
    assert not missing, "float32 (cnv6, cnv7) plans without a case in tests/coupled_cases.py (width, first B, cnv6, cnv7): %s" % missing
    for width in K.WIDTHS:
        for B, t6, t7 in K.F32_CASES[width]:
            g6, g7 = K.gemms(width, B)
            assert (f32(*g6), f32(*g7)) == (t6, t7), (width, B)


# ---- C surface -----------------------------------------------------------------------------------------------------------
def test_header_binding_and_exported_symbol(built):      # noqa: F811
    src = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    assert re.search(r"\bint\s+davo_set_posenn_heads\s*\(\s*davo_ctx\s*\*\s*\w*\s*,\s*int\s+\w+\s*\)\s*;", src)
    assert re.search(r"DAVO_POSENN_HEADS_DECOUPLED\s*=\s*0\s*,\s*DAVO_POSENN_HEADS_COUPLED\s*=\s*1", src)
    comment = src[src.index("The PoseNN's heads"):src.index("int davo_set_posenn_heads")]
    for word in ("nets/posenn.py:133-187", "pose_exp_net/pose/{cnv6,cnv7,pred}/{weights,biases}", "0.01 * mean", "fuse_pose"):
        assert word in comment, word
    assert "davo_set_posenn_heads" in _lib.EXPORTS and (_lib.POSENN_HEADS_DECOUPLED, _lib.POSENN_HEADS_COUPLED) == (0, 1)
    L = ctypes.CDLL(built)
    assert hasattr(L, "davo_set_posenn_heads")
    L.davo_set_posenn_heads.argtypes = [ctypes.c_void_p, ctypes.c_int]
    assert L.davo_set_posenn_heads(None, 1) == -1                # DAVO_ERR_INVALID: a null context, checked before anything else
