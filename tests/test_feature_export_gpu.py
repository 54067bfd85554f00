"""The feature export on the GPU (include/davo_hip.h: davo_set_feature_export / davo_forward_features; DAVO.inference(sess,
mode='feature')) against the float64 restatement of tests/feature_export_ref.py.

The resize is compared with the float64 lerp of the tensor davo_debug_read("cnv6") returns after the same call: every element
within 2^-20 of its largest corner (nine float32 roundings of quantities at most twice that; the weights k/4 are exact) and
bit-equal to the debug read on the lattice.  The maps are compared to the bit with gathers of the exported att_19 rows, the rows
with the forward's own table (davo_debug_read("att_table")), the tables with the float64 references at layer_check's bar, the
masked images in float32 mode with the packed tensor's rgb channels to the bit, the plain images within 2^-22 of float64.
Shapes: 16x16 (cnv6 is 4x4: three of four output rows and columns touch the clamp), 36x100 (9x25: odd extents, no multiple of
any tile), 64x96; B = 1 and 3."""
import ctypes

import numpy as np
import pytest

from davo_amd import DAVO, DavoError, Engine, FLAGSHIP_VERSION, parse_version, synth

from helpers import hip_free_bytes

import depth_source_ref as D
import feature_export_ref as FR
import layer_check as LC

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "f32"]
BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"
RESIZE_REL = 2.0 ** -20
IMAGE_TOL = 2.0 ** -22


def _inputs(cfg, B, H, W, first_window=3):
    img, flow, seg = synth.make_inputs(B, H, W, first_window=first_window)
    seg[0, :, :2, :5] = np.nan                  # labels that are no class, in every frame: no table row
    seg[-1, :, 4:6, 1:3] = -0.75                # truncates to class 0
    seg[-1, :, 6:8] = 19.0
    return (img, flow, seg) + ((synth.make_depth(B, H, W, first_window=first_window),) if cfg.needs_depth else ())


def _weights(cfg, inputs):
    w = synth.make_weights(cfg)
    return D.sensitive_weights(cfg, w, inputs[3]) if cfg.needs_depth else w


def _engine(cfg, H, W, max_batch, weights, precision, export=True):
    e = Engine(cfg, H, W, max_batch)
    e.load_weights(weights)
    e.set_precision(precision)
    if export:
        e.set_feature_export(True)
    return e


def _features(e, inputs, **kw):
    return e.forward_features(*inputs[:3], depth=inputs[3] if len(inputs) > 3 else None, **kw)


def _forward(e, inputs):
    return e.forward(*inputs[:3], depth=inputs[3] if len(inputs) > 3 else None)


def _check_resize(e, cfg, r, B, H, W, what):
    """r's features against the float64 lerp of the cnv6 the engine holds now; -> the worst error in units of the bar."""
    c6 = cfg.cnv6_out
    cnv6 = e.debug_read("cnv6", (2 * B, H // 4, W // 4, 2 * c6))
    worst = 0.0
    for name, want, stored in zip(("feat_rot", "feat_trans"), FR.features(cnv6, c6), (cnv6[1::2, ..., :c6], cnv6[1::2, ..., c6:])):
        got = r[name]
        assert got.shape == (B, H, W, c6) and got.dtype == np.float32, (what, name, got.shape)
        assert np.array_equal(got[:, ::4, ::4], stored), "%s %s: the lattice is not the debug read to the bit" % (what, name)
        bar = RESIZE_REL * FR.corner_max(stored)
        err = np.abs(got.astype(np.float64) - want)
        ratio = float((err / np.maximum(bar, 1e-300)).max()) if err.max() > 0 else 0.0
        print("%s %s: worst |err| / (2^-20 max corner) = %.3g" % (what, name, ratio))
        assert (err <= bar).all(), "%s %s: |err| is %.3g of the bar" % (what, name, ratio)
        worst = max(worst, ratio)
    assert np.abs(cnv6).max() > 0, what
    return worst


# ---- the resize -----------------------------------------------------------------------------------------------------
RESIZE_CASES = [(128, 16, 16, 1), (128, 36, 100, 3), (128, 64, 96, 3), (32, 36, 100, 1), (32, 16, 16, 3), (64, 36, 100, 1),
                (64, 16, 16, 3), (256, 16, 32, 1), (256, 16, 32, 3)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("c6,H,W,B", RESIZE_CASES, ids=["cnv6_%d-%dx%d-B%d" % c for c in RESIZE_CASES])
def test_resize_against_float64_and_the_lattice(c6, H, W, B, precision):
    cfg = parse_version(FLAGSHIP_VERSION.replace("-cnv6_128", "-cnv6_%d" % c6))
    inputs = _inputs(cfg, B, H, W)
    e = _engine(cfg, H, W, B, _weights(cfg, inputs), precision)
    r = _features(e, inputs, want=("feat_rot", "feat_trans"))
    assert set(r) == {"pose", "feat_rot", "feat_trans"}
    _check_resize(e, cfg, r, B, H, W, "cnv6_%d %dx%d B=%d %s" % (c6, H, W, B, precision))
    only = _features(e, inputs, want=("feat_trans",))            # one head alone: the same bits
    assert set(only) == {"pose", "feat_trans"} and np.array_equal(only["feat_trans"], r["feat_trans"])
    e.close()


# ---- the maps ---------------------------------------------------------------------------------------------------------
VARIANTS = [
    ("flagship", FLAGSHIP_VERSION),
    ("no_segmask", BASE + "-no_segmask"),
    ("static", BASE + "-segmask_all-static"),
    ("static_all", BASE + "-segmask_all"),
    ("se_rgb_to_seg", BASE + "-segmask_all-se_rgb_to_seg-fc_tanh"),
    ("se_depth_wo_tgt_to_seg", BASE + "-segmask_all-se_depth_wo_tgt_to_seg-fc_tanh"),
    ("v0", "v0-sharedNN-dilatedPoseNN-segmask-se_flow-abs_flow-fc_tanh"),
    ("se_insert", BASE + "-no_segmask-se_insert"),
]


def _ref_tables(cfg, inputs, weights):
    if cfg.needs_depth:
        return D.class_tables(cfg, inputs[3], weights), [0, 1, 2] if cfg.tgt_attended else [1, 2]
    return LC.ref_tables(cfg, *inputs[:3], weights)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,version", VARIANTS, ids=[v[0] for v in VARIANTS])
def test_maps_per_variant(name, version, precision):
    cfg = parse_version(version)
    B, H, W = 3, 36, 100
    inputs = _inputs(cfg, B, H, W)
    seg = inputs[2]
    weights = _weights(cfg, inputs)
    e = _engine(cfg, H, W, B, weights, precision)
    r = _features(e, inputs)
    what = "%s %s" % (name, precision)
    a19, att = r["att_19"], r["attention"]
    assert a19.shape == (3, B, 19) and att.shape == (3, B, H, W) and a19.dtype == att.dtype == np.float32
    # att_19: the forward's own rows where it looked a table up, ones where the reference overrides the map
    table = e.debug_read("att_table", (B, 3, 19))
    assert np.array_equal(a19, FR.att_19(cfg, table)), what
    want_tab, rows = _ref_tables(cfg, inputs, weights)
    assert rows == [f for f in range(3) if FR.looked_up(cfg, f)], (what, rows)
    LC.check_table(np.transpose(a19, (1, 0, 2)), want_tab, rows, what)
    # attention: the gather of att_19 through int(seg), to the bit
    assert np.array_equal(att, FR.attention(cfg, a19, seg)), what
    for f in range(3):
        plane = seg[:, FR.FILE_PLANE[f], :, :, 0]
        ignore = ~(np.isfinite(plane) & (plane > -1) & (plane < 19))
        assert ignore.any()
        if f in rows:
            assert (att[f][ignore] == 0.0).all(), (what, f)
        else:
            assert (att[f] == 1.0).all() and (a19[f] == 1.0).all(), (what, f)
    # image: within 2^-22 of float64
    err = np.abs(r["image"].astype(np.float64) - FR.images(inputs[0])).max()
    print("%s image: max|err| %.3g (bar %.3g)" % (what, err, IMAGE_TOL))
    assert err <= IMAGE_TOL, what
    # masked image: float32 mode stores the packed tensor as float32 - the same expression, the same bits
    masked = r["masked_image"]
    assert masked.shape == (3, B, H, W, 3)
    if not cfg.mask_rgb:
        assert np.array_equal(masked, r["image"]), what
    if precision == "f32":
        packed = e.debug_read("packed", (2 * B, H, W, 8))
        assert np.array_equal(masked[0], packed[0::2, ..., 0:3]), what + " tgt"
        assert np.array_equal(masked[1], packed[0::2, ..., 3:6]), what + " src0"
        assert np.array_equal(masked[2], packed[1::2, ..., 3:6]), what + " src1"
    else:
        want = FR.masked_images(cfg, FR.images(inputs[0]), att.astype(np.float64))
        assert np.abs(masked.astype(np.float64) - want).max() <= 2 * IMAGE_TOL, what
    _check_resize(e, cfg, r, B, H, W, what)
    e.close()


# ---- poses, sub-batches, recovery -------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_poses_are_davo_forwards_to_the_bit_and_the_pose_path_is_untouched(precision):
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 64, 96
    inputs = _inputs(cfg, B, H, W)
    e = _engine(cfg, H, W, B, _weights(cfg, inputs), precision)
    before = _forward(e, inputs)
    r = _features(e, inputs)
    assert np.array_equal(r["pose"], before)
    assert np.array_equal(_forward(e, inputs), before)            # a mode='pose' call after a feature call
    plain = _features(e, inputs, want=())                         # all-NULL out: a plain forward
    assert set(plain) == {"pose"} and np.array_equal(plain["pose"], before)
    e.close()


def test_the_direct_implementation_exports_too():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 1, 16, 16
    inputs = _inputs(cfg, B, H, W)
    e = _engine(cfg, H, W, B, _weights(cfg, inputs), "f32")
    e.set_impl("direct")
    r = _features(e, inputs)
    assert np.array_equal(r["pose"], _forward(e, inputs))
    _check_resize(e, cfg, r, B, H, W, "impl 1")
    assert np.array_equal(r["attention"], FR.attention(cfg, r["att_19"], inputs[2]))
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_sub_batches_deliver_every_window(precision):
    """B = 3 with host_chunk 2 equals host_chunk 0 to the bit in every output.  (davo_forward splits a batch from 2 x host_chunk
    windows on, so that call is one step.)  host_chunk 1 runs three sub-batches of one window: every window is delivered, each
    to the bit what a call on that window alone returns - across batch sizes the convolutions agree to rounding only, split-K
    moves with the batch (tests/test_hip_parity.py::test_batching_is_per_sample_and_deterministic).  A workspace sized for one
    window serves an unsplit batch in pieces, to the bit."""
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    inputs = _inputs(cfg, B, H, W)
    e = _engine(cfg, H, W, B, _weights(cfg, inputs), precision)
    e.set_option("host_chunk", 0)
    whole = _features(e, inputs)
    e.set_option("host_chunk", 2)
    got = _features(e, inputs)
    for k in whole:
        assert np.array_equal(got[k], whole[k]), (2, k)
    e.set_option("host_chunk", 1)
    got = _features(e, inputs)
    assert np.array_equal(got["pose"], _forward(e, inputs))
    for b in range(B):
        alone = _features(e, tuple(a[b:b + 1] for a in inputs))
        for k in whole:
            mine = got[k][b:b + 1] if k in ("pose", "feat_rot", "feat_trans") else got[k][:, b:b + 1]
            assert np.array_equal(mine, alone[k]), (1, b, k)
    for k in ("att_19", "attention", "masked_image", "image"):          # nothing of these depends on the batch size
        assert np.array_equal(got[k], whole[k]), (1, k)
    e.close()
    e = _engine(cfg, H, W, B, _weights(cfg, inputs), precision, export=False)
    e.set_option("host_chunk", 1)
    e.set_feature_export(True)                                           # room for one window
    e.set_option("host_chunk", 0)
    got = _features(e, inputs)
    for k in whole:
        assert np.array_equal(got[k], whole[k]), ("pieces", k)
    e.close()


def _rescaled(weights, shift):
    """tests/test_hip_parity.py's guard recipe: cnv3's activations x 2^shift, undone in cnv4 - the same network, outside the
    fp16-pair range of the default scales."""
    k = np.float32(2.0 ** shift)
    w2 = dict(weights)
    w2["pose_exp_net/cnv3/weights"] = weights["pose_exp_net/cnv3/weights"] * k
    w2["pose_exp_net/cnv3/biases"] = weights["pose_exp_net/cnv3/biases"] * k
    w2["pose_exp_net/cnv4/weights"] = weights["pose_exp_net/cnv4/weights"] / k
    return w2


@pytest.mark.parametrize("chunk", [0, 1])
def test_a_reissued_batch_is_exported_from_the_reissue(chunk):
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    inputs = _inputs(cfg, B, H, W)
    e = _engine(cfg, H, W, B, _rescaled(_weights(cfg, inputs), 16), "f16x3")
    e.set_option("host_chunk", chunk)
    r = _features(e, inputs)
    st = e.range_stats()
    assert st["reissued"] == 1 and st["recalibrations"] == 1 and st["f32_batches"] == 0, (st, e.range_report())
    _check_resize(e, cfg, r, B, H, W, "re-issued, host_chunk %d" % chunk)      # the post-call cnv6 is the re-issue's
    assert np.array_equal(r["att_19"], FR.att_19(cfg, e.debug_read("att_table", (B, 3, 19))))
    assert np.array_equal(r["attention"], FR.attention(cfg, r["att_19"], inputs[2]))
    again = _features(e, inputs)                                               # the new scales hold
    assert e.range_stats() == st
    if chunk == 0:                                                             # (sub-batches of one window: equal to rounding only)
        for k in r:
            assert np.array_equal(again[k], r[k]), k
    e.close()


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_errors():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 1, 16, 16
    inputs = _inputs(cfg, B, H, W)
    weights = _weights(cfg, inputs)
    e = _engine(cfg, H, W, B, weights, "f16x3", export=False)
    with pytest.raises(DavoError, match="davo_set_feature_export"):           # DAVO_ERR_NOT_READY
        _features(e, inputs)
    pose = np.empty((B, 2, 6), np.float32)
    raw = [a.ctypes.data_as(ctypes.c_void_p) for a in inputs[:3]]
    assert e._L.davo_forward_features(e._ctx, B, *raw, None, pose.ctypes.data_as(ctypes.c_void_p), None) == -3
    with pytest.raises(DavoError, match="davo_set_feature_export"):
        _features(e, inputs, want=())
    e.set_feature_export(True)
    e.set_pairs("src1")
    with pytest.raises(ValueError, match="DAVO_PAIRS_BOTH"):                  # DAVO_ERR_INVALID
        _features(e, inputs)
    e.set_pairs("both")
    with pytest.raises(ValueError, match="unknown feature output"):
        _features(e, inputs, want=("flows",))
    assert set(_features(e, inputs, want=("att_19",))) == {"pose", "att_19"}
    e.set_feature_export(False)
    with pytest.raises(DavoError, match="davo_set_feature_export"):
        _features(e, inputs)
    e.close()
    # a depth source without its planes: davo_forward_depth's error
    dcfg = parse_version(BASE + "-segmask_all-se_depth_to_seg-fc_tanh")
    dinputs = _inputs(dcfg, B, H, W)
    e = _engine(dcfg, H, W, B, _weights(dcfg, dinputs), "f16x3")
    vp = ctypes.c_void_p
    pose = np.empty((B, 2, 6), np.float32)
    args = [a.ctypes.data_as(vp) for a in dinputs[:3]]
    rc_f = e._L.davo_forward_depth(e._ctx, B, *args, None, pose.ctypes.data_as(vp))
    msg_f = e._L.davo_last_error(e._ctx).decode()
    rc_x = e._L.davo_forward_features(e._ctx, B, *args, None, pose.ctypes.data_as(vp), None)
    assert rc_x == rc_f == -1 and e._L.davo_last_error(e._ctx).decode() == msg_f and "null depth" in msg_f
    with pytest.raises(ValueError, match="depth"):
        e.forward_features(*dinputs[:3])
    assert np.array_equal(_features(e, dinputs)["pose"], _forward(e, dinputs))
    e.close()


# ---- memory -----------------------------------------------------------------------------------------------------------
def test_the_workspace_goes_with_the_context_and_costs_nothing_while_off():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 64, 96
    inputs = _inputs(cfg, B, H, W)
    weights = _weights(cfg, inputs)
    free = []
    for _ in range(10):
        e = _engine(cfg, H, W, B, weights, "f16x3")
        _features(e, inputs)
        e.close()
        free.append(hip_free_bytes())
    assert free[9] == free[0], free
    # never enabled: what a context allocates is what it allocates after enable + disable
    e = _engine(cfg, H, W, B, weights, "f16x3", export=False)
    _forward(e, inputs)
    never = hip_free_bytes()
    e.set_feature_export(True)
    assert hip_free_bytes() < never                       # 2 x 3 x 64 x 96 x 128 x 4 B of features alone
    e.set_feature_export(False)
    assert hip_free_bytes() == never
    _forward(e, inputs)
    assert hip_free_bytes() == never
    e.close()


# ---- the reference's call surface -------------------------------------------------------------------------------------
def _check_feature_dict(out, B, H, W, c6):
    assert set(out) == {"pose", "masks", "features", "images", "seg_19"}
    assert set(out["masks"]) == {"attention", "image", "att_19"} and set(out["features"]) == {"rot", "trans"}
    assert out["pose"].shape == (B, 2, 6) and out["pose"].dtype == np.float32
    for key, shape in (("attention", (B, H, W, 1)), ("image", (B, H, W, 3)), ("att_19", (B, 1, 1, 19))):
        assert isinstance(out["masks"][key], list) and len(out["masks"][key]) == 3
        assert all(a.shape == shape and a.dtype == np.float32 for a in out["masks"][key]), key
    for key in ("rot", "trans"):
        assert out["features"][key].shape == (B, H, W, c6) and out["features"][key].dtype == np.float32
    assert len(out["images"]) == 3 and all(a.shape == (B, H, W, 3) and a.dtype == np.float32 for a in out["images"])
    assert len(out["seg_19"]) == 3 and all(a.shape == (B, H, W, 19) and a.dtype == np.float32 for a in out["seg_19"])


def test_davo_inference_feature_mode():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    img, flow, seg = _inputs(cfg, B, H, W)
    weights = synth.make_weights(cfg)
    d = DAVO(version=FLAGSHIP_VERSION)
    d.load_weights(weights)
    d.setup_inference(H, W, "davo", 3, B, img, input_flow=flow, input_seglabel=seg)
    with pytest.raises(NotImplementedError, match="enable_feature_mode"):
        d.inference(None, mode='feature')
    pose = d.inference(None, mode='pose')['pose']
    d.enable_feature_mode()                                    # after setup_inference
    out = d.inference(None, mode='feature')
    _check_feature_dict(out, B, H, W, cfg.cnv6_out)
    assert np.array_equal(out["pose"], pose)
    assert np.array_equal(d.inference(None, mode='pose')['pose'], pose)
    for f in range(3):
        a19, att = out["masks"]["att_19"][f], out["masks"]["attention"][f]
        plane = seg[:, FR.FILE_PLANE[f], :, :, 0]
        idx, ok = FR.class_index(plane)
        assert np.array_equal(att[..., 0][ok], np.take_along_axis(a19[:, 0, 0], idx.reshape(B, -1), 1).reshape(B, H, W)[ok])
        assert np.array_equal(out["seg_19"][f], FR.seg_19(seg)[f])
    with pytest.raises(NotImplementedError):
        d.inference(None, mode='depth')
    d.engine.close()

    # the iterator form, enabled before setup_inference: every batch once, in order, also behind a pose call's look-ahead
    def batches():
        for i in range(B):
            yield img[i:i + 1], flow[i:i + 1], seg[i:i + 1]
    s = DAVO(version=FLAGSHIP_VERSION).enable_feature_mode()
    s.load_weights(weights)
    s.setup_inference(H, W, "davo", 3, 1, batches())
    for i in range(B):
        got = s.inference(None, mode='feature')
        _check_feature_dict(got, 1, H, W, cfg.cnv6_out)
        # window i's: its frames and maps to the bit (they do not depend on the batch size), its poses to rounding
        assert np.array_equal(got["images"][1][0], out["images"][1][i]), i
        assert np.array_equal(got["masks"]["attention"][2][0], out["masks"]["attention"][2][i]), i
        assert np.abs(got["pose"][0] - pose[i]).max() <= 1e-5 * np.abs(pose).max(), i
    with pytest.raises(StopIteration):
        s.inference(None, mode='feature')
    s.engine.close()
