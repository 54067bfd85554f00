"""The heat export on the GPU (include/davo_hip.h: davo_set_heat_export / davo_forward_heat; DAVO.enable_feature_mode(
features='heat'); davo_amd/generate_feature_map.py) against the float64 restatement of tests/heat_export_ref.py, which reduces
in the reference's order: resize every channel, then sum / max.

The maxima are compared to the bit with the per-window, per-head maximum of davo_debug_read("cnv6") after the same call; the
lattice heat[b, 4i, 4j] to the bit with the device's own channel sums (davo_debug_read("heat_sum")) of a second call, which is
also bit for bit the first; every output of the planes within 2^-20 of its largest corner sum (heat_export_ref.BAR_REL: 12 + 3
float32 roundings, a bar the reference's order meets itself: tests/test_heat_export.py).
Shapes: 16x16 (cnv6 is 4x4: every output row and column is border or next to it), 16x32 and 32x16 (a transposed stride shows),
B = 1, and B = 3 through a one-window workspace, so that pieces are exercised; 20x28 (5x7) where a window's pixels are no whole
number of waves, the one other path of the reduction kernel."""
import ctypes
import functools

import numpy as np
import pytest

from davo_amd import DAVO, DavoError, Engine, FLAGSHIP_VERSION, parse_version, synth
from davo_amd import generate_feature_map as G

from helpers import hip_free_bytes
from test_feature_export_gpu import BASE, PRECISIONS, _engine, _features, _forward, _inputs, _rescaled, _weights

import heat_export_ref as HR

pytestmark = pytest.mark.gpu

HEAT = Engine.HEAT_OUTPUTS
HEADS = (("rot", "heat_rot", "max_rot"), ("trans", "heat_trans", "max_trans"))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _heat_engine(cfg, H, W, max_batch, weights, precision, one_window=False, full=False):
    """an engine with the heat export on; one_window: a workspace for one window (switched on under host_chunk 1) that serves
    an unsplit batch in pieces"""
    e = _engine(cfg, H, W, max_batch, weights, precision, export=full)
    if one_window:
        e.set_option("host_chunk", 1)
    e.set_heat_export(True)
    if one_window:
        e.set_option("host_chunk", 0)
    return e


def _check_against_cnv6(e, cfg, r, B, H, W, what):
    """r's heat outputs against the cnv6 the engine holds now: maxima to the bit, planes within the bar on every output,
    the lattice bit for bit the fixed pairwise float32 tree of the stored values; -> the worst error in units of the bar"""
    c6 = cfg.cnv6_out
    cnv6 = e.debug_read("cnv6", (2 * B, H // 4, W // 4, 2 * c6))
    ref = HR.heat(cnv6, c6)
    worst = 0.0
    for (name, plane, top), stored in zip(HEADS, HR.stored_heads(cnv6, c6).values()):
        assert r[plane].shape == (B, H, W) and r[plane].dtype == np.float32 and r[top].shape == (B,) and r[top].dtype == np.float32
        assert _same_bits(r[top], stored.max(axis=(1, 2, 3))), "%s %s: not the stored maximum to the bit" % (what, top)
        assert np.array_equal(r[top].astype(np.float64), ref[name][2]), (what, top)
        bar = HR.BAR_REL * HR.corner_sum_max(stored)
        err = np.abs(r[plane].astype(np.float64) - ref[name][0])
        assert err.shape == (B, H, W)                                   # every output is compared
        ratio = float((err / np.maximum(bar, 1e-300)).max()) if err.max() > 0 else 0.0
        print("%s %s: worst |err| / (2^-20 max corner sum) = %.3g" % (what, plane, ratio))
        assert (err <= bar).all(), "%s %s: |err| is %.3g of the bar" % (what, plane, ratio)
        assert _same_bits(r[plane][:, ::4, ::4], HR.pairwise_sum_f32(stored)), "%s %s: the lattice is not the fixed tree's sum" % (what, plane)
        worst = max(worst, ratio)
    assert np.abs(cnv6).max() > 0, what
    return worst


# ---- maxima, lattice, whole planes: every width, both storage forms ---------------------------------------------------
#        cnv6_out, H, W, B, one-window workspace
CASES = [(32, 16, 16, 1, False), (32, 16, 32, 3, True), (64, 32, 16, 1, False), (64, 16, 16, 3, True),
         (128, 16, 32, 1, False), (128, 32, 16, 3, True), (256, 16, 16, 1, False), (256, 16, 32, 3, True), (256, 32, 16, 3, False),
         (64, 20, 28, 3, False)]          # cnv6 5x7: 35 pixels a window, so a wave of the reduction straddles two windows
CASE_IDS = ["cnv6_%d-%dx%d-B%d%s" % (c[:4] + ("-pieces" if c[4] else "",)) for c in CASES]


@functools.lru_cache(maxsize=None)
def _run(case, precision):
    """two calls of one engine and what the device holds after them, computed once per case and left unchanged"""
    c6, H, W, B, one_window = case
    cfg = parse_version(FLAGSHIP_VERSION.replace("-cnv6_128", "-cnv6_%d" % c6))
    inputs = _inputs(cfg, B, H, W)
    e = _heat_engine(cfg, H, W, B, _weights(cfg, inputs), precision, one_window)
    first = _features(e, inputs, want=HEAT)
    second = _features(e, inputs, want=HEAT)
    n = 1 if one_window else B                                          # windows of the piece exported last
    out = dict(cfg=cfg, first=first, second=second, cnv6=e.debug_read("cnv6", (2 * B, H // 4, W // 4, 2 * c6)),
               heat_sum=e.debug_read("heat_sum", (2, n, H // 4, W // 4)), n=n)
    with pytest.raises(ValueError, match="heat_sum"):
        e.debug_read("heat_sum", (2, n + 1, H // 4, W // 4))
    only = _features(e, inputs, want=("max_trans",))                     # one member alone: the same bits
    assert set(only) == {"pose", "max_trans"} and _same_bits(only["max_trans"], first["max_trans"])
    only = _features(e, inputs, want=("heat_rot",))
    assert set(only) == {"pose", "heat_rot"} and _same_bits(only["heat_rot"], first["heat_rot"])
    e.close()
    for a in list(first.values()) + list(second.values()) + [out["cnv6"], out["heat_sum"]]:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_maxima_are_the_stored_maxima_to_the_bit(case, precision):
    c6, H, W, B, _ = case
    got = _run(case, precision)
    assert set(got["second"]) == {"pose"} | set(HEAT)
    for (name, _, top), stored in zip(HEADS, HR.stored_heads(got["cnv6"], c6).values()):
        want = stored.max(axis=(1, 2, 3))
        assert got["second"][top].shape == (B,) and got["second"][top].dtype == np.float32
        assert _same_bits(got["second"][top], want), (name, got["second"][top], want)
        assert (want > 0).all()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_lattice_is_the_devices_own_channel_sum_and_calls_repeat(case, precision):
    c6, H, W, B, _ = case
    got = _run(case, precision)
    for k in got["first"]:
        assert _same_bits(got["first"][k], got["second"][k]), k                  # bitwise reproducible
    n = got["n"]
    for h, (name, plane, _) in enumerate(HEADS):
        lattice = got["second"][plane][:, ::4, ::4]
        assert lattice.shape == (B, H // 4, W // 4)
        assert _same_bits(lattice[B - n:], got["heat_sum"][h]), name               # the piece the workspace holds
        # ... and every window's is the fixed tree of the stored values: (c0 + c1) + (c2 + c3), then pairwise
        assert _same_bits(lattice, HR.pairwise_sum_f32(HR.stored_heads(got["cnv6"], c6)[name])), name


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_whole_planes_against_the_reference_order(case, precision):
    c6, H, W, B, _ = case
    got = _run(case, precision)
    ref = HR.heat(got["cnv6"], c6)
    for name, plane, _ in HEADS:
        stored = HR.stored_heads(got["cnv6"], c6)[name]
        bar = HR.BAR_REL * HR.corner_sum_max(stored)
        err = np.abs(got["second"][plane].astype(np.float64) - ref[name][0])
        assert err.shape == bar.shape == (B, H, W)                                 # no output is left out
        ratio = float((err / np.maximum(bar, 1e-300)).max()) if err.max() > 0 else 0.0
        print("%s %s %s: worst |err| / (2^-20 max corner sum) = %.3g" % (CASE_IDS[CASES.index(case)], precision, plane, ratio))
        assert (err <= bar).all(), "%s: |err| is %.3g of the bar" % (plane, ratio)
        assert ref[name][0].max() > 0


# ---- against the full export ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_heat_is_the_reduction_of_the_full_maps_of_the_same_call(precision):
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W, c6 = 3, 16, 32, cfg.cnv6_out
    inputs = _inputs(cfg, B, H, W)
    e = _heat_engine(cfg, H, W, B, _weights(cfg, inputs), precision, full=True)
    r = _features(e, inputs, want=("feat_rot", "feat_trans") + HEAT)
    assert set(r) == {"pose", "feat_rot", "feat_trans"} | set(HEAT)
    for feat, plane, top in (("feat_rot", "heat_rot", "max_rot"), ("feat_trans", "heat_trans", "max_trans")):
        full = r[feat]
        bar = HR.BAR_REL * HR.corner_sum_max(full[:, ::4, ::4])                    # the lattice of the full map is the stored cnv6
        err = np.abs(r[plane].astype(np.float64) - full.sum(-1, dtype=np.float64))
        assert err.shape == (B, H, W) and (err <= bar).all(), (plane, float((err / np.maximum(bar, 1e-300)).max()))
        assert _same_bits(r[top], full.max(axis=(1, 2, 3))), top
    # the full members through the new entry point are davo_forward_features' to the bit
    old = _features(e, inputs, want=("feat_rot", "att_19"))
    new = _features(e, inputs, want=("feat_rot", "att_19", "max_rot"))
    assert _same_bits(old["feat_rot"], new["feat_rot"]) and _same_bits(old["att_19"], new["att_19"]) and _same_bits(old["feat_rot"], r["feat_rot"])
    e.close()


# ---- poses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_poses_are_davo_forwards_to_the_bit_before_and_after(precision):
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 16, 32
    inputs = _inputs(cfg, B, H, W)
    e = _heat_engine(cfg, H, W, B, _weights(cfg, inputs), precision)
    before = _forward(e, inputs)
    r = _features(e, inputs, want=HEAT)
    assert _same_bits(r["pose"], before)
    assert _same_bits(_forward(e, inputs), before)
    # NULL structs through the raw entry point: a plain forward
    vp = ctypes.c_void_p
    pose = np.empty((B, 2, 6), np.float32)
    assert e._L.davo_forward_heat(e._ctx, B, *[a.ctypes.data_as(vp) for a in inputs[:3]], None, pose.ctypes.data_as(vp), None, None) == 0
    assert _same_bits(pose, before)
    e.close()


def test_sub_batches_deliver_every_window():
    """host_chunk 1: B = 3 runs as three sub-batches of one window, each exported before the next one runs; every window is
    to the bit what a call on that window alone returns."""
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 32, 16
    inputs = _inputs(cfg, B, H, W)
    e = _heat_engine(cfg, H, W, B, _weights(cfg, inputs), "f16x3")
    e.set_option("host_chunk", 1)
    got = _features(e, inputs, want=HEAT)
    assert _same_bits(got["pose"], _forward(e, inputs))
    for b in range(B):
        alone = _features(e, tuple(a[b:b + 1] for a in inputs), want=HEAT)
        for k in got:
            assert _same_bits(got[k][b:b + 1], alone[k]), (b, k)
    _check_against_cnv6(e, cfg, alone, 1, H, W, "the last window alone")
    e.close()


# ---- variants ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,version", [("se_insert", BASE + "-no_segmask-se_insert"),
                                          ("se_depth_to_seg", BASE + "-segmask_all-se_depth_to_seg-fc_tanh")])
def test_variants(name, version):
    cfg = parse_version(version)
    B, H, W = 3, 16, 32
    inputs = _inputs(cfg, B, H, W)
    assert (len(inputs) == 4) == (name == "se_depth_to_seg")                    # the depth source runs with its planes
    e = _heat_engine(cfg, H, W, B, _weights(cfg, inputs), "f16x3")
    r = _features(e, inputs, want=HEAT)
    assert _same_bits(r["pose"], _forward(e, inputs))
    _check_against_cnv6(e, cfg, r, B, H, W, name)
    e.close()


def test_the_direct_implementation_exports_too():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 1, 16, 16
    inputs = _inputs(cfg, B, H, W)
    e = _heat_engine(cfg, H, W, B, _weights(cfg, inputs), "f32")
    e.set_impl("direct")
    r = _features(e, inputs, want=HEAT)
    assert _same_bits(r["pose"], _forward(e, inputs))
    _check_against_cnv6(e, cfg, r, B, H, W, "impl 1")
    e.close()


# ---- re-issue ---------------------------------------------------------------------------------------------------------
def test_a_reissued_batch_is_exported_from_the_reissue():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    inputs = _inputs(cfg, B, H, W)
    e = _heat_engine(cfg, H, W, B, _rescaled(_weights(cfg, inputs), 16), "f16x3")
    r = _features(e, inputs, want=HEAT)
    st = e.range_stats()
    assert st["reissued"] == 1 and st["recalibrations"] == 1 and st["f32_batches"] == 0, (st, e.range_report())
    _check_against_cnv6(e, cfg, r, B, H, W, "re-issued")                        # the post-call cnv6 is the re-issue's
    again = _features(e, inputs, want=HEAT)                                      # the new scales hold
    assert e.range_stats() == st
    for k in r:
        assert _same_bits(again[k], r[k]), k
    e.close()


# ---- error codes ------------------------------------------------------------------------------------------------------
def test_error_codes():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 1, 16, 16
    inputs = _inputs(cfg, B, H, W)
    e = _engine(cfg, H, W, B, _weights(cfg, inputs), "f16x3", export=False)
    vp = ctypes.c_void_p
    pose = np.empty((B, 2, 6), np.float32)
    raw = [a.ctypes.data_as(vp) for a in inputs[:3]]
    top = np.empty(B, np.float32)
    from davo_amd import _lib
    heat = _lib.DavoHeatOut(None, None, top.ctypes.data, None)

    def call(out, h):
        rc = e._L.davo_forward_heat(e._ctx, B, *raw, None, pose.ctypes.data_as(vp), out, h)
        return rc, e._L.davo_last_error(e._ctx).decode()
    # a heat member with the switch off
    rc, msg = call(None, ctypes.byref(heat))
    assert rc == -3 and "davo_set_heat_export" in msg
    with pytest.raises(DavoError, match="davo_set_heat_export"):
        _features(e, inputs, want=("max_rot",))
    e.set_feature_export(True)                                                  # the other switch does not open it
    rc, msg = call(None, ctypes.byref(heat))
    assert rc == -3 and "davo_set_heat_export" in msg
    e.set_feature_export(False)
    # a full member with only the heat switch on
    e.set_heat_export(True)
    feat = np.empty((B, H, W, cfg.cnv6_out), np.float32)
    rc, msg = call(ctypes.byref(_lib.DavoFeatureOut(None, None, None, None, feat.ctypes.data, None)), ctypes.byref(heat))
    assert rc == -3 and "davo_set_feature_export" in msg
    a19 = np.empty((3, B, 19), np.float32)
    rc, msg = call(ctypes.byref(_lib.DavoFeatureOut(a19.ctypes.data, None, None, None, None, None)), None)
    assert rc == -3 and "davo_set_feature_export" in msg
    with pytest.raises(DavoError, match="davo_set_feature_export"):
        _features(e, inputs, want=("feat_rot", "max_rot"))
    rc, msg = call(None, ctypes.byref(heat))                                    # heat alone: fine
    assert rc == 0, msg
    # the pair selection
    e.set_pairs("src1")
    rc, msg = call(None, ctypes.byref(heat))
    assert rc == -1 and "DAVO_PAIRS_BOTH" in msg
    with pytest.raises(ValueError, match="DAVO_PAIRS_BOTH"):
        _features(e, inputs, want=HEAT)
    e.set_pairs("both")
    with pytest.raises(ValueError, match="unknown feature output"):
        _features(e, inputs, want=("heat_rot", "flows"))
    e.set_heat_export(False)
    rc, msg = call(None, ctypes.byref(heat))
    assert rc == -3 and "davo_set_heat_export" in msg
    e.close()


# ---- memory -----------------------------------------------------------------------------------------------------------
def test_the_workspace_is_small_costs_nothing_while_off_and_goes_with_the_context():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 8, 128, 416                                   # the flagship shape; eight windows put the block above any allocation granule
    inputs = _inputs(cfg, 1, H, W)
    weights = _weights(cfg, inputs)
    e = _engine(cfg, H, W, B, weights, "f16x3", export=False)
    _forward(e, inputs)
    never = hip_free_bytes()                                 # the switch is off: nothing of the export is there
    e.set_heat_export(True)
    heat_bytes = never - hip_free_bytes()
    r = _features(e, inputs, want=HEAT)
    assert hip_free_bytes() == never - heat_bytes            # a call allocates nothing more
    assert r["heat_rot"].shape == (1, H, W) and (r["max_rot"] > 0).all()
    e.set_heat_export(False)
    assert hip_free_bytes() == never
    e.set_feature_export(True)
    full_bytes = never - hip_free_bytes()
    e.set_feature_export(False)
    assert hip_free_bytes() == never
    formula = 8 * 2 * (H // 4 * (W // 4) + H * W + 1) * 4
    print("heat workspace %d bytes (formula %d), full export workspace %d bytes: 1/%.0f" % (heat_bytes, formula, full_bytes, full_bytes / max(heat_bytes, 1)))
    assert full_bytes > 0 and 0 <= heat_bytes < full_bytes / 50
    _forward(e, inputs)
    assert hip_free_bytes() == never
    e.close()
    free = []
    small = _inputs(cfg, 3, 16, 32)
    for _ in range(4):
        e = _heat_engine(cfg, 16, 32, 3, weights, "f16x3")
        _features(e, small, want=HEAT)
        e.close()                                            # the switch still on: davo_destroy frees the block
        free.append(hip_free_bytes())
    assert free[3] == free[0], free


# ---- the reference's call surface -------------------------------------------------------------------------------------
def _check_heat_dict(out, B, H, W):
    assert set(out) == {"pose", "masks", "features", "images", "seg_19"}
    assert set(out["features"]) == {"rot_sum", "trans_sum", "rot_avg", "trans_avg", "rot_max", "trans_max"}
    assert out["pose"].shape == (B, 2, 6)
    for k, a in out["features"].items():
        assert a.dtype == np.float32 and a.shape == ((B,) if k.endswith("_max") else (B, H, W)), k
    assert set(out["masks"]) == {"attention", "image", "att_19"}
    for key, shape in (("attention", (B, H, W, 1)), ("image", (B, H, W, 3)), ("att_19", (B, 1, 1, 19))):
        assert len(out["masks"][key]) == 3 and all(a.shape == shape and a.dtype == np.float32 for a in out["masks"][key]), key
    assert len(out["images"]) == 3 and all(a.shape == (B, H, W, 3) for a in out["images"])
    assert len(out["seg_19"]) == 3 and all(a.shape == (B, H, W, 19) for a in out["seg_19"])


def test_davo_inference_feature_mode_heat():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W, c6 = 3, 16, 32, cfg.cnv6_out
    img, flow, seg = _inputs(cfg, B, H, W)
    weights = synth.make_weights(cfg)
    d = DAVO(version=FLAGSHIP_VERSION)
    d.load_weights(weights)
    d.setup_inference(H, W, "davo", 3, B, img, input_flow=flow, input_seglabel=seg)
    pose = d.inference(None, mode='pose')['pose']
    d.enable_feature_mode(features='heat')                     # after setup_inference
    out = d.inference(None, mode='feature')
    _check_heat_dict(out, B, H, W)
    f = out["features"]
    assert _same_bits(out["pose"], pose) and _same_bits(d.inference(None, mode='pose')['pose'], pose)
    for head in ("rot", "trans"):
        assert np.array_equal(f[head + "_avg"] * np.float32(c6), f[head + "_sum"])            # exactly: the width is a power of two
        assert (f[head + "_max"] > 0).all() and (f[head + "_avg"].max(axis=(1, 2)) <= f[head + "_max"]).all()
    # only the heat switch is on: the full export's workspace was never allocated, its members stay closed
    with pytest.raises(DavoError, match="davo_set_feature_export"):
        d.engine.forward_features(img, flow, seg, want=("feat_rot",))
    d.engine.close()

    # full mode on the same class is what it was; the heat dict is its reduction, its maps are its maps to the bit
    full = DAVO(version=FLAGSHIP_VERSION).enable_feature_mode()
    full.load_weights(weights)
    full.setup_inference(H, W, "davo", 3, B, img, input_flow=flow, input_seglabel=seg)
    ref = full.inference(None, mode='feature')
    assert set(ref["features"]) == {"rot", "trans"} and ref["features"]["rot"].shape == (B, H, W, c6)
    assert _same_bits(ref["pose"], pose)
    for k in range(3):
        assert _same_bits(out["masks"]["att_19"][k], ref["masks"]["att_19"][k]), k
        assert _same_bits(out["masks"]["attention"][k], ref["masks"]["attention"][k]), k
        assert _same_bits(out["masks"]["image"][k], ref["masks"]["image"][k]), k
        assert _same_bits(out["images"][k], ref["images"][k]), k
        assert np.array_equal(out["seg_19"][k], ref["seg_19"][k]), k
    for head in ("rot", "trans"):
        assert _same_bits(f[head + "_max"], ref["features"][head].max(axis=(1, 2, 3)))
        bar = HR.BAR_REL * HR.corner_sum_max(ref["features"][head][:, ::4, ::4])
        assert (np.abs(f[head + "_sum"].astype(np.float64) - ref["features"][head].sum(-1, dtype=np.float64)) <= bar).all()
    full.engine.close()

    # the iterator form, enabled before setup_inference: every batch once, in order
    def batches():
        for i in range(B):
            yield img[i:i + 1], flow[i:i + 1], seg[i:i + 1]
    s = DAVO(version=FLAGSHIP_VERSION).enable_feature_mode(features='heat')
    s.load_weights(weights)
    s.setup_inference(H, W, "davo", 3, 1, batches())
    for i in range(B):
        got = s.inference(None, mode='feature')
        _check_heat_dict(got, 1, H, W)
        assert _same_bits(got["images"][1][0], out["images"][1][i]), i
        assert _same_bits(got["masks"]["attention"][2][0], out["masks"]["attention"][2][i]), i
        scale = float(f["rot_sum"][i].max())
        assert np.abs(got["features"]["rot_sum"][0] - f["rot_sum"][i]).max() <= 1e-4 * scale, i       # across batch sizes: to rounding
    with pytest.raises(StopIteration):
        s.inference(None, mode='feature')
    s.engine.close()

    # a batch davo_forward splits (2 x host_chunk windows): issued as its sub-batches, every window delivered
    big = DAVO(version=FLAGSHIP_VERSION).enable_feature_mode(features='heat')
    big.load_weights(weights)
    big.setup_inference(H, W, "davo", 3, B, img, input_flow=flow, input_seglabel=seg)
    big.engine.set_option("host_chunk", 1)
    split = big.inference(None, mode='feature')
    _check_heat_dict(split, B, H, W)
    assert _same_bits(split["pose"], big.inference(None, mode='pose')['pose'])
    for k in range(3):
        assert _same_bits(split["masks"]["att_19"][k], out["masks"]["att_19"][k]) and _same_bits(split["images"][k], out["images"][k]), k
    big.engine.close()


# ---- the driver end to end --------------------------------------------------------------------------------------------
def test_the_driver_end_to_end(tmp_path):
    from PIL import Image
    H, W, n_frames = 16, 32, 5
    out_dir = tmp_path / "out"
    G.main(["--synthetic", str(n_frames), "--img_height", str(H), "--img_width", str(W), "--output_dir", str(out_dir),
            "--test_seq", "9", "--batch_size", "2", "--npy"])
    n_windows = n_frames - 2
    assert sorted(p.name for p in out_dir.iterdir()) == ["09-featuremaps", "09-pred_kitti_pose.txt", "09-tgtsrc0.txt", "09-tgtsrc1.txt"]
    names = sorted(p.name for p in (out_dir / "09-featuremaps").iterdir())
    want = sorted(G.feature_file(w, head, kind, ext) for w in range(n_windows) for head in G.HEADS for kind in G.KINDS for ext in ("png", "npy"))
    assert names == want and len(names) == n_windows * 8 and "000001-rot_feature-avg.png" in names
    assert len(open(out_dir / "09-pred_kitti_pose.txt").read().splitlines()) == n_frames
    # the same windows through the class: tables and one image of every kind
    d = DAVO(version=FLAGSHIP_VERSION).enable_feature_mode(features='heat')
    d.load_weights(synth.make_weights(FLAGSHIP_VERSION))
    d.setup_inference(H, W, "davo", 3, 2)
    pred = d.inference(None, mode='feature', inputs=synth.make_inputs(2, H, W, first_window=0))
    d.engine.close()
    for k, name in ((1, "09-tgtsrc0.txt"), (2, "09-tgtsrc1.txt")):
        lines = open(out_dir / name).read().splitlines(True)
        assert len(lines) == 1 + n_windows and lines[0] == G.table_title()
        for w in range(2):
            assert lines[1 + w] == G.table_line(w, pred["masks"]["att_19"][k][w, 0, 0]), (name, w)
    f = pred["features"]
    w = 1
    for head in G.HEADS:
        png = np.asarray(Image.open(out_dir / "09-featuremaps" / G.feature_file(w, head, "avg")))
        assert png.dtype == np.uint8 and png.shape == (H, W)
        assert np.array_equal(png, HR.index_image(f[head + "_avg"][w], f[head + "_max"][w]))
        png = np.asarray(Image.open(out_dir / "09-featuremaps" / G.feature_file(w, head, "sum")))
        assert np.array_equal(png, HR.index_image(f[head + "_sum"][w], f[head + "_sum"][w].max())) and png.max() == 255
        assert _same_bits(np.load(out_dir / "09-featuremaps" / G.feature_file(w, head, "sum", "npy")), f[head + "_sum"][w])
