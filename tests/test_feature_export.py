"""The feature export's surface without a GPU: the header declares it and the binding carries it, DAVO has the opt-in, and
the float64 restatement the GPU tests compare against (tests/feature_export_ref.py) has the properties it is trusted for."""
import ctypes
import os
import re

import numpy as np
import pytest

from davo_amd import DAVO, Engine, FLAGSHIP_VERSION, _lib, parse_version
from davo_amd.davo import seg_one_hot

import feature_export_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "davo_hip.h")).read(), flags=re.S)


def test_header_declares_the_entry_points_and_the_binding_carries_them():
    src = _header()
    assert re.search(r"int\s+davo_set_feature_export\s*\(\s*davo_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", src)
    assert re.search(r"int\s+davo_forward_features\s*\(", src)
    m = re.search(r"typedef\s+struct\s*\{(.*?)\}\s*davo_feature_out\s*;", src, flags=re.S)
    assert m, "davo_feature_out is not declared"
    fields = re.findall(r"float\s*\*\s*(\w+)\s*;", m.group(1))
    assert fields == ["att_19", "attention", "masked_image", "image", "feat_rot", "feat_trans"]
    assert [n for n, _ in _lib.DavoFeatureOut._fields_] == fields               # field order is ABI
    assert ctypes.sizeof(_lib.DavoFeatureOut) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert {"davo_set_feature_export", "davo_forward_features"} <= set(_lib.EXPORTS)
    assert "launch_feature" in _lib.UNITS
    assert tuple(Engine.FEATURE_OUTPUTS) == tuple(fields)


def test_davo_has_the_opt_in_and_the_mode_stays_closed_without_it():
    d = DAVO(version=FLAGSHIP_VERSION)
    assert callable(d.enable_feature_mode)
    with pytest.raises(NotImplementedError, match="enable_feature_mode"):
        d.inference(None, mode='feature')
    with pytest.raises(NotImplementedError):
        d.inference(None, mode='depth')
    assert d.enable_feature_mode() is d                  # before setup_inference: remembered, nothing to allocate yet
    with pytest.raises(NotImplementedError):
        d.inference(None, mode='depth')                  # any other unknown mode keeps raising


# ---- the restatement's own properties -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps():
    rng = np.random.default_rng(5)
    return [rng.standard_normal((2, h, w, 3)) for h, w in ((4, 4), (9, 25), (16, 24), (1, 1))]


def test_resize_lattice_identity(maps):
    for x in maps:
        assert np.array_equal(FR.resize_x4(x)[:, ::4, ::4], x)


def test_resize_clamped_border(maps):
    for x in maps:
        y = FR.resize_x4(x)
        r, c = 4 * (x.shape[1] - 1), 4 * (x.shape[2] - 1)
        assert np.array_equal(y[:, r:], np.repeat(y[:, r:r + 1], 4, axis=1))
        assert np.array_equal(y[:, :, c:], np.repeat(y[:, :, c:c + 1], 4, axis=2))


def test_resize_equals_the_separable_form(maps):
    for x in maps:
        a, b = FR.resize_x4(x), FR.resize_x4_separable(x)
        assert a.shape == (x.shape[0], 4 * x.shape[1], 4 * x.shape[2], x.shape[3])
        assert np.abs(a - b).max() <= 8 * np.finfo(np.float64).eps * np.abs(x).max()
    m = FR.resize_matrix(9)
    assert np.allclose(m.sum(axis=1), 1.0) and (m >= 0).all() and (np.count_nonzero(m, axis=1) <= 2).all()
    assert np.array_equal(m[4:8, 1], [1.0, 0.75, 0.5, 0.25]) and np.array_equal(m[4:8, 2], [0.0, 0.25, 0.5, 0.75])


def test_resize_error_scale_is_the_largest_corner(maps):
    x = maps[1]
    assert (np.abs(FR.resize_x4(x)) <= FR.corner_max(x) * (1 + 1e-15)).all()      # a convex combination of the corners


def test_features_take_the_second_pair_and_split_the_heads():
    rng = np.random.default_rng(6)
    cnv6 = rng.standard_normal((6, 4, 5, 64))
    rot, trans = FR.features(cnv6, 32)
    assert rot.shape == trans.shape == (3, 16, 20, 32)
    assert np.array_equal(rot[:, ::4, ::4], cnv6[1::2, :, :, :32]) and np.array_equal(trans[:, ::4, ::4], cnv6[1::2, :, :, 32:])


FAMILIES = [
    # (version, frames gathered from the forward's table)
    (FLAGSHIP_VERSION, [1, 2]),                                               # -se_flow: the target is overridden with ones
    (BASE + "-no_segmask", []),
    (BASE + "-segmask_all-static", [1, 2]),
    (BASE + "-segmask_all", [0, 1, 2]),                                       # static_all
    (BASE + "-segmask_all-se_rgb_wo_tgt_to_seg-fc_tanh", [1, 2]),
    (BASE + "-segmask_all-se_rgb_to_seg-fc_tanh", [0, 1, 2]),
    (BASE + "-segmask_all-se_depth_wo_tgt_to_seg-fc_tanh", [1, 2]),
    (BASE + "-segmask_all-se_depth_to_seg-fc_tanh", [0, 1, 2]),
]


@pytest.mark.parametrize("version,rows", FAMILIES)
def test_att_19_rule_per_variant_family(version, rows):
    cfg = parse_version(version)
    rng = np.random.default_rng(7)
    tables = rng.uniform(0.05, 0.95, (2, 3, 19)).astype(np.float32)           # whatever d_tab holds on overridden rows
    a19 = FR.att_19(cfg, tables)
    assert a19.shape == (3, 2, 19) and a19.dtype == np.float32
    for f in range(3):
        assert FR.looked_up(cfg, f) == (f in rows)
        assert np.array_equal(a19[f], tables[:, f] if f in rows else np.ones((2, 19), np.float32))
    seg = rng.integers(0, 19, (2, 3, 8, 8, 1)).astype(np.float32)
    seg[0, :, 0, 0] = 255.0                                                  # an ignore pixel in every frame
    att = FR.attention(cfg, a19, seg)
    for f in range(3):
        plane = seg[:, FR.FILE_PLANE[f], :, :, 0]
        if f in rows:
            assert att[f][0, 0, 0] == 0.0
            assert np.array_equal(att[f][1], a19[f][1][plane[1].astype(int)])
        else:
            assert np.array_equal(att[f], np.ones_like(att[f]))              # ignore pixels included
    imgs = FR.images(rng.integers(0, 256, (2, 8, 24, 3), dtype=np.uint8))
    masked = FR.masked_images(cfg, imgs, att)
    assert np.array_equal(masked, imgs * att[..., None] if cfg.mask_rgb else imgs)


def test_images_follow_the_strip_order():
    img = np.zeros((1, 4, 12, 3), np.uint8)
    img[:, :, 0:4], img[:, :, 4:8], img[:, :, 8:12] = 0, 255, 51            # src0 | tgt | src1
    x = FR.images(img)
    assert x.shape == (3, 1, 4, 4, 3)
    assert np.all(x[0] == 1.0) and np.all(x[1] == -1.0) and np.allclose(x[2], -0.6, atol=1e-15)


def test_seg_19_on_the_edge_labels():
    labels = np.array([0, 18, 19, 255, -1, 18.9, np.nan, np.inf, -0.5], np.float32)
    seg = np.broadcast_to(labels[None, None, None, :, None], (1, 3, 1, labels.size, 1)).copy()
    want = np.zeros((labels.size, 19), np.float32)
    want[0, 0] = want[1, 18] = want[5, 18] = want[8, 0] = 1.0               # truncation: 18.9 -> 18, -0.5 -> 0; the rest: zero rows
    for got in FR.seg_19(seg):
        assert got.shape == (1, 1, labels.size, 19) and got.dtype == np.float32
        assert np.array_equal(got[0, 0], want)
    lib = seg_one_hot(seg)                                                     # what DAVO.inference returns is the same rule
    assert lib.shape == (1, 3, 1, labels.size, 19) and lib.dtype == np.float32
    assert all(np.array_equal(lib[0, p, 0], want) for p in range(3))
