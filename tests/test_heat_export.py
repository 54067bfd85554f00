"""The heat export's surface without a GPU: the header declares it, the binding carries it and the library exports it; the two
identities it rests on (sum o resize = resize o sum; max of the resized map = max of the stored map) hold for the restatement of
tests/heat_export_ref.py; the bar the GPU test holds the device to is met by the reference's own order; the driver's file names,
table lines and index images are the reference's."""
import ctypes
import os
import re

import numpy as np
import pytest

from davo_amd import DAVO, Engine, FLAGSHIP_VERSION, _lib, parse_version
from davo_amd import generate_feature_map as G
from davo_amd.davo import host_maps

import feature_export_ref as FR
import heat_export_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "davo_hip.h")).read(), flags=re.S)


# ---- header <-> binding <-> exported symbols ----------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_new_names():
    src = _header()
    assert re.search(r"int\s+davo_set_heat_export\s*\(\s*davo_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", src)
    m = re.search(r"int\s+davo_forward_heat\s*\((.*?)\)\s*;", src, flags=re.S)
    assert m, "davo_forward_heat is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 9 and params[0].startswith("davo_ctx") and params[1].startswith("int")
    assert params[7].startswith("const davo_feature_out*") and params[8].startswith("const davo_heat_out*")
    s = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*davo_heat_out\s*;", src)
    assert s, "davo_heat_out is not declared"
    fields = re.findall(r"float\s*\*\s*(\w+)\s*;", s.group(1))
    assert fields == ["rot_sum", "trans_sum", "rot_max", "trans_max"]
    assert [n for n, _ in _lib.DavoHeatOut._fields_] == fields                  # field order is ABI
    assert ctypes.sizeof(_lib.DavoHeatOut) == 4 * ctypes.sizeof(ctypes.c_void_p)
    f = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*davo_feature_out\s*;", src)
    assert len(re.findall(r"float\s*\*\s*(\w+)\s*;", f.group(1))) == 6             # davo_feature_out keeps its six members
    assert {"davo_set_heat_export", "davo_forward_heat"} <= set(_lib.EXPORTS)
    L = ctypes.CDLL(_lib.build())
    for name in ("davo_set_heat_export", "davo_forward_heat"):
        assert hasattr(L, name), name
    bound = _lib.lib()
    assert len(bound.davo_forward_heat.argtypes) == 9 and len(bound.davo_set_heat_export.argtypes) == 2
    assert Engine.HEAT_OUTPUTS == ("heat_rot", "heat_trans", "max_rot", "max_trans")
    assert Engine.FEATURE_OUTPUTS == ("att_19", "attention", "masked_image", "image", "feat_rot", "feat_trans")
    raw = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    assert "generate_feature_map.py:204-265" in raw


def test_enable_feature_mode_takes_full_or_heat():
    d = DAVO(version=FLAGSHIP_VERSION)
    with pytest.raises(ValueError, match="bogus"):
        d.enable_feature_mode(features='bogus')
    with pytest.raises(NotImplementedError, match="enable_feature_mode"):        # a refused choice opens nothing
        d.inference(None, mode='feature')
    assert d.enable_feature_mode(features='heat') is d and d.enable_feature_mode(features='full') is d
    assert d.enable_feature_mode() is d


# ---- identity 1: sum o resize = resize o sum (float64) ----------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (1, 5), (4, 4), (5, 1), (4, 8), (8, 4), (9, 25)])
def test_sum_then_resize_is_resize_then_sum(h, w):
    rng = np.random.default_rng(100 * h + w)
    for C in (32, 256):
        x = rng.random((2, h, w, C)) * rng.choice([1e-3, 1.0, 1e3], size=(2, h, w, 1))
        then_sum = FR.resize_x4(x).sum(axis=-1)
        sum_then = FR.resize_x4(x.sum(axis=-1)[..., None])[..., 0]
        assert then_sum.shape == (2, 4 * h, 4 * w)
        assert np.abs(then_sum - sum_then).max() <= 1e-12 * np.abs(then_sum).max()
        assert np.abs(FR.resize_x4(x).mean(axis=-1) * C - sum_then).max() <= 1e-12 * np.abs(then_sum).max()


# ---- identity 2: max(resized) == max(stored), float32, TF's order, to the bit -----------------------------------------
def _adversarial_quadruples():
    f = np.float32
    tiny, big = f(np.finfo(np.float32).tiny), f(np.finfo(np.float32).max)
    den = f(1e-45)                                                     # the smallest denormal
    vals = [f(0), den, f(3) * den, tiny, np.nextafter(tiny, f(0)), f(1), np.nextafter(f(1), f(2)), np.nextafter(f(1), f(0)),
            f(0.1), f(1e-20), f(65504), f(1e30), big, np.nextafter(big, f(0))]
    quads = []
    for a in vals:
        quads.append((a, a, a, a))                                     # equal corners
        for b in vals:
            quads += [(a, b, b, b), (b, a, b, b), (b, b, a, b), (b, b, b, a), (a, b, a, b), (a, a, b, b), (a, b, b, a)]
            quads += [(f(0), a, b, a), (a, f(0), a, b), (a, b, f(0), b), (b, a, b, f(0))]      # one corner 0
        up = np.nextafter(a, big)
        quads += [(a, up, a, up), (up, a, up, a), (a, a, up, up), (up, up, a, a), (a, up, up, a)]   # adjacent floats
    return np.array(quads, np.float32)


def test_the_resized_maximum_is_the_stored_maximum_to_the_bit():
    rng = np.random.default_rng(11)
    rand = (rng.random((100000, 4), dtype=np.float32) * np.exp2(rng.integers(-30, 30, size=(100000, 1))).astype(np.float32))
    rand[::7, rng.integers(0, 4)] = 0.0
    for quads in (rand, _adversarial_quadruples()):
        with np.errstate(over="ignore", under="ignore"):
            out = HR.lerp_corners_f32(*quads.T)                        # [n,4,4]
        corner_max = quads.max(axis=1)
        assert np.array_equal(out[:, 0, 0].view(np.uint32), quads[:, 0].view(np.uint32))        # the lattice value, unchanged
        finite = np.isfinite(out).all(axis=(1, 2))                     # (max - 0 is finite; only max-float differences overflow)
        assert finite.mean() > 0.9
        assert (out[finite].max(axis=(1, 2)) <= corner_max[finite]).all()
        assert (out[finite].min(axis=(1, 2)) >= quads[finite].min(axis=1)).all()
    # and so for whole blocks, clamped borders included: 1x1, 1x5, 4x4, odd extents
    for h, w in ((1, 1), (1, 5), (4, 4), (3, 7)):
        x = rng.random((2, h, w, 8), dtype=np.float32) * np.float32(37.5)
        x[rng.random(x.shape) < 0.4] = 0.0                             # post-ReLU: many zeros
        got = HR.resize_x4_f32(x).max(axis=(1, 2, 3))
        assert np.array_equal(got.view(np.uint32), x.max(axis=(1, 2, 3)).view(np.uint32))


# ---- the GPU test's bar is one the reference's order meets ------------------------------------------------------------
@pytest.mark.parametrize("c6", [32, 64, 128, 256])
@pytest.mark.parametrize("h,w", [(4, 4), (4, 8), (8, 4)])
def test_the_reference_order_meets_the_bar_with_a_float32_pairwise_sum(c6, h, w):
    """The device stand-in - float32 pairwise channel sum of the stored block, then TF's float32 lerp of that plane - against
    the float64 reduction of the resized maps, at the GPU test's shapes: within 2^-20 of the largest corner sum on every
    output, none left out."""
    rng = np.random.default_rng(c6 + h)
    B = 3
    cnv6 = (rng.random((2 * B, h, w, 2 * c6), dtype=np.float32) * np.float32(20.0))
    cnv6[rng.random(cnv6.shape) < 0.5] = 0.0
    ref = HR.heat(cnv6, c6)
    for name, stored in HR.stored_heads(cnv6, c6).items():
        standin = HR.resize_x4_f32(HR.pairwise_sum_f32(stored)[..., None])[..., 0]
        bar = HR.BAR_REL * HR.corner_sum_max(stored)
        err = np.abs(standin.astype(np.float64) - ref[name][0])
        assert err.shape == (B, 4 * h, 4 * w) and (err <= bar).all(), (name, float((err / np.maximum(bar, 1e-300)).max()))
        assert np.array_equal(standin[:, ::4, ::4], HR.pairwise_sum_f32(stored))
        assert np.array_equal(ref[name][2], stored.max(axis=(1, 2, 3)).astype(np.float64))
        assert np.abs(ref[name][1] * c6 - ref[name][0]).max() <= 1e-12 * ref[name][0].max()


# ---- index images -----------------------------------------------------------------------------------------------------
def test_index_images_are_the_references_expression():
    rng = np.random.default_rng(3)
    resized = rng.random((8, 12, 32), dtype=np.float32) * np.float32(9.0)
    resized[rng.random(resized.shape) < 0.3] = 0.0
    avg_ref, sum_ref = HR.reference_images(resized)
    total = resized.sum(axis=-1)
    mean = total * np.float32(1.0 / 32)
    feats = {"rot_sum": total[None], "rot_avg": mean[None], "rot_max": np.array([resized.max()], np.float32),
             "trans_sum": np.zeros((1, 8, 12), np.float32), "trans_avg": np.zeros((1, 8, 12), np.float32), "trans_max": np.zeros(1, np.float32)}
    images = G.window_images(feats, 0)
    assert set(images) == {("rot", "avg"), ("rot", "sum"), ("trans", "avg"), ("trans", "sum")}
    assert images["rot", "sum"][1].dtype == np.uint8 and np.array_equal(images["rot", "sum"][1], sum_ref)
    assert sum_ref.max() == 255
    # the mean: numpy's float32 mean and sum * (1 / C) differ by rounding, so an index may differ by one where it sits on a step
    d = np.abs(images["rot", "avg"][1].astype(int) - avg_ref.astype(int))
    assert d.max() <= 1 and (d > 0).mean() < 0.01
    assert np.array_equal(G.index_image(mean, resized.max()), HR.index_image(mean, resized.max()))
    # maximum 0: all zeros, not the reference's division by zero
    for fn in (G.index_image, HR.index_image):
        z = fn(np.zeros((4, 4), np.float32), 0.0)
        assert z.dtype == np.uint8 and z.shape == (4, 4) and not z.any()
    assert not images["trans", "avg"][1].any() and not images["trans", "sum"][1].any()
    assert np.array_equal(G.index_image(np.float32([0, 1, 2, 4]), 4.0), np.uint8([0, 63, 127, 255]))      # truncation, not rounding


# ---- the driver's names and lines -------------------------------------------------------------------------------------
def test_driver_file_names_and_table_lines():
    assert G.feature_file(0, "rot", "avg") == "000001-rot_feature-avg.png"
    assert G.feature_file(4538, "trans", "sum") == "004539-trans_feature-sum.png"
    assert G.feature_file(2, "rot", "sum", "npy") == "000003-rot_feature-sum.npy"
    with pytest.raises(ValueError):
        G.feature_file(0, "pose", "avg")
    with pytest.raises(ValueError):
        G.feature_file(0, "rot", "max")
    assert G.table_title() == "id,road,sidewalk,building,wall,fence,pole,traffic light,traffic sign,vegetation,terrain,sky,person," \
                              "rider,car,truck,bus,train,motorcycle,bicycle\n"
    row = np.linspace(0.0, 1.0, 19).astype(np.float32)
    line = G.table_line(6, row)
    assert line == "%06d,%s\n" % (7, ",".join([str(att) for att in row]))      # generate_feature_map.py:191
    assert line.startswith("000007,0.0,") and line.endswith(",1.0\n") and line.count(",") == 19
    assert G.table_line(0, np.ones((1, 1, 19), np.float32)[0, 0]) == "000001," + ",".join(["1.0"] * 19) + "\n"
    with pytest.raises(ValueError):
        G.table_line(0, np.ones(18, np.float32))
    a = G.build_parser().parse_args(["--output_dir", "o"])
    assert (a.batch_size, a.img_height, a.img_width, a.seq_length, a.test_seq) == (1, 128, 416, 3, 9)
    assert a.concat_img_dir is None and a.ckpt_file is None and a.synthetic is None and not a.npy
    assert "cv2" in G.__doc__


# ---- the maps of the heat mode, rebuilt on the host -------------------------------------------------------------------
@pytest.mark.parametrize("version", [FLAGSHIP_VERSION, BASE + "-no_segmask", BASE + "-segmask_all", BASE + "-segmask_all-static"])
def test_host_maps_are_the_restatements_maps(version):
    from davo_amd import synth
    cfg = parse_version(version)
    B, H, W = 2, 8, 12
    img, flow, seg = synth.make_inputs(B, H, W)
    seg[0, :, :2, :5] = np.nan
    seg[-1, :, 4:6, 1:3] = -0.75
    seg[-1, :, 6:8] = 19.0
    tables = np.random.default_rng(1).random((B, 3, 19), dtype=np.float32)
    m = host_maps(cfg, img, seg, tables)
    assert all(a.dtype == np.float32 for a in m.values())
    assert np.array_equal(m["att_19"], FR.att_19(cfg, tables))
    assert np.array_equal(m["attention"], FR.attention(cfg, m["att_19"], seg))
    assert np.abs(m["image"] - FR.images(img)).max() <= 2.0 ** -22
    assert np.array_equal(m["masked_image"], m["image"] * m["attention"][..., None] if cfg.mask_rgb else m["image"])
