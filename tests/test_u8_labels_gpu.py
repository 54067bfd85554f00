"""Byte label maps on the GPU (include/davo_hip.h: davo_set_label_format).

Every comparison is between a float32-label engine on label maps S and a byte-label engine on labels_to_u8(S), with the same
weights and the same other inputs, and every comparison is to the bit: the byte is the float's class for every pixel
(tests/test_u8_labels.py), so the two engines must compute the same numbers everywhere.  The float engine's own comparison
against float64 exists already (tests/test_plan_layers_gpu.py and the variants' own files): bit-equality to it is the whole
proof.  S is synth.make_inputs' label maps with NaN, -0.5, 18.9, 19.0, 200.0, 255.0 and +inf written in.

Shapes: 36x100 (odd map extents, no multiple of any tile) and 64x96 with more than one window, and once 128x416 at batch 1 for
cnv1's production tile; B = 9 at 36x100 crosses davo_forward's sub-batch of 8 and takes davo_submit's two-plane label copy."""
import numpy as np
import pytest

from davo_amd import DAVO, Engine, FLAGSHIP_VERSION, labels_to_u8, parse_version, synth
from davo_amd.version import ATT_SOURCE

from helpers import hip_free_bytes

pytestmark = pytest.mark.gpu

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"
VARIANTS = [                                                 # one per family
    ("flagship", FLAGSHIP_VERSION),
    ("static_all", BASE + "-segmask_all"),
    ("se_seg_wo_tgt", BASE + "-segmask_all-se_seg_wo_tgt-fc_tanh"),
    ("se_SegFlow_to_seg_8", BASE + "-segmask_all-se_SegFlow_to_seg_8-abs_flow-fc_tanh"),
    ("se_rgb_to_seg", BASE + "-segmask_all-se_rgb_to_seg-fc_tanh"),
    ("se_depth_to_seg", BASE + "-segmask_all-se_depth_to_seg-fc_tanh"),
    ("depthseg_seplayers", BASE + "-segmask_all-se_flow_on_depthseg_seplayers-abs_flow-fc_tanh"),
    ("no_segmask_se_insert", BASE + "-no_segmask-se_insert"),
    ("v0_segmask", "v0-sharedNN-dilatedPoseNN-segmask-se_flow-abs_flow-fc_tanh"),
]
IDS = [v[0] for v in VARIANTS]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _inputs(cfg, B, H, W, first_window=3):
    """-> (img, flow, S, labels_to_u8(S), depth or None)"""
    img, flow, seg = synth.make_inputs(B, H, W, first_window=first_window)
    seg[0, :, :2, :5] = np.nan                               # labels that are no class, in every frame
    seg[-1, :, 4:6, 1:3] = -0.5                              # truncates to class 0
    seg[-1, :, 6:8, :7] = 18.9                               # class 18
    seg[0, :, 8:10] = 19.0
    seg[-1, :, 10:12, 3:] = 200.0
    seg[0, :, 12:13] = 255.0
    seg[-1, :, 13:15, ::3] = np.inf
    depth = synth.make_depth(B, H, W, first_window=first_window) if cfg.needs_depth else None
    return img, flow, seg, labels_to_u8(seg), depth


def _engines(cfg, H, W, max_batch, weights=None):
    """-> (the float32-label engine, the byte-label engine), same weights"""
    weights = synth.make_weights(cfg) if weights is None else weights
    pair = (Engine(cfg, H, W, max_batch), Engine(cfg, H, W, max_batch, labels="u8"))
    for e in pair:
        e.load_weights(weights)
    assert pair[0]._L.davo_get_label_format(pair[0]._ctx) == 0 and pair[1]._L.davo_get_label_format(pair[1]._ctx) == 1
    return pair


def _unread_planes(cfg, pairs):
    """label planes (file order src0, tgt, src1) that a batch of this variant under this pair selection does not read"""
    if ATT_SOURCE[cfg.att_source] == 0:
        return [0, 1, 2]
    read = {"src0": {0}, "src1": {2}, "both": {0, 2}}[pairs] | ({1} if cfg.tgt_attended else set())
    return [p for p in (0, 1, 2) if p not in read]


def _other_ids(seg8, planes):
    """seg8 with other valid class ids in `planes`"""
    out = seg8.copy()
    for p in planes:
        out[:, p] = (seg8[:, p].astype(np.int32) * 5 + 7) % 19
        assert (out[:, p] != seg8[:, p]).any()
    return out


# ---- layer tensors ----------------------------------------------------------------------------------------------------
def _layer_tensors(e, cfg, img, flow, seg, depth, impl):
    B, H, W = img.shape[0], img.shape[1], img.shape[2] // 3
    out = {"pose": e.forward(img, flow, seg, depth)}
    if ATT_SOURCE[cfg.att_source] != 0:                      # (-no_segmask computes no table)
        out["att_table"] = e.debug_read("att_table", (B, 3, 19))
    if cfg.att_source == "se_flow_depthseg_sep":
        out["att_table_far"] = e.debug_read("att_table_far", (B, 3, 19))
    out["packed"] = e.debug_read("packed", (2 * B, H, W, 10 if impl else 8))
    return out


SETTINGS = {"f16x3": [{}, {"fuse_pack": 0}, {"fuse_pack": 1}, {"fold_tails": 0}, {"fold_tails": 1}],
            "f32": [{}, {"impl": 1}, {"fold_tails": 0}, {"fold_tails": 1}]}          # impl 1: the LD = 10 packer


def _compare_layers(cfg, B, H, W, settings=SETTINGS):
    img, flow, seg, seg8, depth = _inputs(cfg, B, H, W)
    ef, eb = _engines(cfg, H, W, B)
    assert np.isfinite(seg).sum() < seg.size and (seg8 == 255).any() and (seg8 == 18).any()
    for precision, options in settings.items():
        for opts in options:
            if opts.get("impl") and cfg.version.startswith("v0"):
                continue                                     # the direct-convolution cross-check takes the 10-channel (v1) input only
            got = []
            for e, s in ((ef, seg), (eb, seg8)):
                e.set_precision(precision)
                e.set_impl(opts.get("impl", 0))
                e.set_option("fuse_pack", opts.get("fuse_pack", -1))
                e.set_option("fold_tails", opts.get("fold_tails", -1))
                got.append(_layer_tensors(e, cfg, img, flow, s, depth, opts.get("impl", 0)))
            for k in got[0]:
                assert _same(got[0][k], got[1][k]), "%s %dx%d B=%d %s %s: %s differs" % (cfg.version, H, W, B, precision, opts, k)
            assert np.abs(got[0]["pose"]).max() > 0 and np.isfinite(got[0]["packed"]).all()
    ef.close()
    eb.close()


@pytest.mark.parametrize("name,version", VARIANTS, ids=IDS)
def test_layer_tensors_are_the_float_engines_to_the_bit(name, version):
    cfg = parse_version(version)
    _compare_layers(cfg, 3, 36, 100)
    _compare_layers(cfg, 2, 64, 96)


def test_layer_tensors_on_the_production_tile():
    _compare_layers(parse_version(FLAGSHIP_VERSION), 1, 128, 416, {"f16x3": [{"fuse_pack": 0}, {"fuse_pack": 1}], "f32": [{}]})


# ---- every entry point ------------------------------------------------------------------------------------------------
def _device_forward(e, B, img, flow, seg, depth):
    arrays = [img, flow, seg] + ([depth] if depth is not None else [])
    bufs = [e.alloc(a.nbytes).upload(a) for a in arrays]
    d_pose = e.alloc(B * 12 * 4)
    try:
        e.forward_device(B, bufs[0], bufs[1], bufs[2], d_pose, depth=bufs[3] if depth is not None else None)
        e.synchronize()
        return d_pose.download((B, 2, 6))
    finally:
        for b in bufs + [d_pose]:
            b.free()


def _streamed(e, img, flow, seg, depth, n=5):
    """n submits of the batch from scratch arrays that are overwritten as soon as each davo_submit returns (hold = 0)"""
    scratch = [np.empty_like(a) for a in (img, flow, seg)] + ([np.empty_like(depth)] if depth is not None else [])
    outs = [np.full((img.shape[0], 2, 6), np.nan, np.float32) for _ in range(n)]
    for out in outs:
        for dst, src in zip(scratch, (img, flow, seg, depth)):
            dst[...] = src
        e.submit(scratch[0], scratch[1], scratch[2], out, hold=0, depth=scratch[3] if depth is not None else None)
        scratch[0][...] = 77
        scratch[1][...] = 1e6
        scratch[2][...] = 3
        if depth is not None:
            scratch[3][...] = 0.25
    e.wait(0)
    e.synchronize()
    return outs


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("name,version", VARIANTS, ids=IDS)
def test_every_entry_point(name, version, B):
    cfg = parse_version(version)
    H, W = 36, 100
    img, flow, seg, seg8, depth = _inputs(cfg, B, H, W)
    ef, eb = _engines(cfg, H, W, 9)
    for e in (ef, eb):
        e.set_inflight(4)
    for pairs in ("src0", "src1", "both"):
        unread = _unread_planes(cfg, pairs)
        alt = _other_ids(seg8, unread)                       # the planes nobody reads hold other classes than the float array's
        for e in (ef, eb):
            e.set_pairs(pairs)
        what = "%s B=%d %s" % (name, B, pairs)
        want = ef.forward(img, flow, seg, depth)
        assert np.abs(want).max() > 0
        assert _same(eb.forward(img, flow, alt, depth), want), what + ": davo_forward"
        dev = _device_forward(ef, B, img, flow, seg, depth)
        assert _same(_device_forward(eb, B, img, flow, alt, depth), dev), what + ": davo_forward_device"
        sf, sb = _streamed(ef, img, flow, seg, depth), _streamed(eb, img, flow, alt, depth)
        for a, b in zip(sf, sb):
            assert np.isfinite(a).all() and _same(a, b), what + ": davo_submit"
        if len(unread) < 3:                                  # ... and the planes that ARE read matter
            moved = _other_ids(seg8, [p for p in (0, 2) if p not in unread][:1])
            assert not _same(eb.forward(img, flow, moved, depth), want), what + ": a label plane the batch reads changed nothing"
    # calibration runs both pairs of the batch it is handed, whatever the selection
    alt = _other_ids(seg8, _unread_planes(cfg, "both"))
    assert ef.calibrate(img, flow, seg, depth) == eb.calibrate(img, flow, alt, depth)
    for e in (ef, eb):
        e.set_pairs("both")
    assert _same(ef.forward(img, flow, seg, depth), eb.forward(img, flow, alt, depth)), "%s B=%d after davo_calibrate" % (name, B)
    assert ef.range_stats() == eb.range_stats()
    ef.close()
    eb.close()


# ---- range recovery ---------------------------------------------------------------------------------------------------
def _rescaled(weights, shift):
    """tests/test_hip_parity.py's guard recipe: cnv3's activations x 2^shift, undone in cnv4 - the same network, outside the
    fp16-pair range of the default scales."""
    k = np.float32(2.0 ** shift)
    w2 = dict(weights)
    w2["pose_exp_net/cnv3/weights"] = weights["pose_exp_net/cnv3/weights"] * k
    w2["pose_exp_net/cnv3/biases"] = weights["pose_exp_net/cnv3/biases"] * k
    w2["pose_exp_net/cnv4/weights"] = weights["pose_exp_net/cnv4/weights"] / k
    return w2


@pytest.mark.parametrize("streamed", [False, True], ids=["davo_forward", "davo_submit"])
def test_a_batch_that_trips_the_range_guard_is_reissued_from_the_bytes(streamed):
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    img, flow, seg, seg8, _ = _inputs(cfg, B, H, W)
    ef, eb = _engines(cfg, H, W, B, _rescaled(synth.make_weights(cfg), 16))
    if streamed:
        for e in (ef, eb):
            e.set_inflight(2)
        got_f, got_b = _streamed(ef, img, flow, seg, None, n=3), _streamed(eb, img, flow, seg8, None, n=3)      # re-issued from the library's own copy
    else:
        got_f, got_b = [ef.forward(img, flow, seg)], [eb.forward(img, flow, seg8)]
    for a, b in zip(got_f, got_b):
        assert np.isfinite(a).all() and np.abs(a).max() > 0 and _same(a, b)
    st = ef.range_stats()
    assert st["reissued"] >= 1 and st["recalibrations"] >= 1, (st, ef.range_report())
    assert eb.range_stats() == st, (eb.range_stats(), eb.range_report())
    ef.close()
    eb.close()


# ---- exports ----------------------------------------------------------------------------------------------------------
EXPORT_VARIANTS = [VARIANTS[0], VARIANTS[4]]                 # the flagship and a class-table variant that attends the target


@pytest.mark.parametrize("name,version", EXPORT_VARIANTS, ids=[v[0] for v in EXPORT_VARIANTS])
def test_exports(name, version):
    cfg = parse_version(version)
    B, H, W = 3, 36, 100
    img, flow, seg, seg8, depth = _inputs(cfg, B, H, W)
    want_all = Engine.FEATURE_OUTPUTS + Engine.HEAT_OUTPUTS
    for one_window in (False, True):
        ef, eb = _engines(cfg, H, W, B)
        got = []
        for e, s in ((ef, seg), (eb, seg8)):
            if one_window:                                   # room for one window: the batch goes out in pieces
                e.set_option("host_chunk", 1)
            e.set_feature_export(True)
            e.set_heat_export(True)
            if one_window:
                e.set_option("host_chunk", 0)
            r = [e.forward_features(img, flow, s, depth, want=want_all)]
            e.set_option("host_chunk", 1)                    # sub-batches of one window
            r.append(e.forward_features(img, flow, s, depth, want=("att_19", "attention", "masked_image")))
            got.append(r)
        for rf, rb in zip(*got):
            assert set(rf) == set(rb)
            for k in rf:
                assert _same(rf[k], rb[k]), "%s one_window=%s: %s differs" % (name, one_window, k)
        assert set(got[0][0]) == {"pose"} | set(want_all)
        att = got[0][0]["attention"]
        assert (att == 0).any() and (att != 0).any()         # labels that are no class zero the map in both
        ef.close()
        eb.close()


@pytest.mark.parametrize("features", ["full", "heat"])
def test_the_reference_call_surface_takes_bytes(features):
    B, H, W = 2, 36, 100
    cfg = parse_version(FLAGSHIP_VERSION)
    img, flow, seg, seg8, _ = _inputs(cfg, B, H, W)
    weights = synth.make_weights(cfg)
    outs = []
    for labels, s in (("f32", seg), ("u8", seg8), ("u8", seg8[..., 0])):      # bytes as [B,3,H,W,1] and as [B,3,H,W]
        d = DAVO(FLAGSHIP_VERSION).enable_feature_mode(features=features)
        if labels == "u8":
            assert d.use_u8_labels() is d
        d.setup_inference(H, W, "davo", 3, B, input_img_uint8=img, input_flow=flow, input_seglabel=s)
        d.load_weights(weights)
        assert d.engine.labels == labels
        out = d.inference(mode="feature")
        assert _same(d.inference(mode="pose")["pose"], out["pose"])
        assert _same(d.inference(mode="pose", inputs=(img, flow, s))["pose"], out["pose"])
        it = DAVO(FLAGSHIP_VERSION)
        if labels == "u8":
            it.use_u8_labels()
        it.setup_inference(H, W, "davo", 3, B, input_img_uint8=iter([(img, flow, s)] * 2))
        it.load_weights(weights)
        assert _same(it.inference()["pose"], it.inference()["pose"])
        it.engine.close()
        outs.append(out)
        d.engine.close()

    def flat(x, prefix=""):
        if isinstance(x, dict):
            return {k2: v2 for k, v in x.items() for k2, v2 in flat(v, prefix + k + ".").items()}
        if isinstance(x, list):
            return {k2: v2 for i, v in enumerate(x) for k2, v2 in flat(v, prefix + "%d." % i).items()}
        return {prefix: x}
    want = flat(outs[0])
    assert any(k.startswith("seg_19") for k in want) and want["seg_19.1."].shape == (B, H, W, 19)
    for out in outs[1:]:
        got = flat(out)
        assert set(got) == set(want)
        for k in want:
            assert _same(got[k], want[k]), k


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_errors():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 1, 16, 16
    img, flow, seg, seg8, _ = _inputs(cfg, B, H, W)
    ef, eb = _engines(cfg, H, W, B)
    L = ef._L
    assert L.davo_set_label_format(ef._ctx, 2) == -1 and b"DAVO_LABELS" in L.davo_last_error(ef._ctx)
    assert L.davo_set_label_format(ef._ctx, -1) == -1
    assert L.davo_set_label_format(ef._ctx, 1) == 0 and L.davo_get_label_format(ef._ctx) == 1       # before any input: either way
    assert L.davo_set_label_format(ef._ctx, 0) == 0 and L.davo_get_label_format(ef._ctx) == 0
    ef.forward(img, flow, seg)
    assert L.davo_set_label_format(ef._ctx, 1) == -1 and b"before the first call that takes inputs" in L.davo_last_error(ef._ctx)
    assert L.davo_get_label_format(ef._ctx) == 0
    with pytest.raises(ValueError, match="before the first call"):
        ef.set_label_format("u8")
    assert ef.labels == "f32"
    eb.forward(img, flow, seg8)
    with pytest.raises(ValueError, match="before the first call"):
        eb.set_label_format("f32")
    with pytest.raises(ValueError, match="labels"):
        Engine(cfg, H, W, B, labels="bytes")
    # nothing converts silently, in either direction, at any entry point
    out = np.empty((B, 2, 6), np.float32)
    for e, wrong in ((eb, seg), (ef, seg8), (eb, seg8.astype(np.int32))):
        with pytest.raises(ValueError, match="label"):
            e.forward(img, flow, wrong)
        with pytest.raises(ValueError, match="label"):
            e.submit(img, flow, wrong, out)
        with pytest.raises(ValueError, match="label"):
            e.calibrate(img, flow, wrong)
        with pytest.raises(ValueError, match="label"):
            e.forward_features(img, flow, wrong)
        d_seg = e.alloc(wrong.nbytes).upload(wrong)
        with pytest.raises(ValueError, match="label"):
            e.forward_device(B, d_seg, d_seg, d_seg, d_seg)
        d_seg.free()
    assert ef.pending() == 0 and eb.pending() == 0
    ef.close()
    eb.close()


# ---- memory -----------------------------------------------------------------------------------------------------------
def _stream_some(e, img, flow, seg, slots):
    e.set_inflight(slots)
    outs = [np.empty((img.shape[0], 2, 6), np.float32) for _ in range(slots + 1)]
    for out in outs:
        e.submit(img, flow, seg, out, hold=8)
    e.wait(0)
    e.synchronize()
    return outs


def test_device_memory():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W, slots = 4, 128, 416, 4
    img, flow, seg, seg8, _ = _inputs(cfg, B, H, W)
    weights = synth.make_weights(cfg)
    free = []
    for _ in range(3):
        e = Engine(cfg, H, W, B, labels="u8")
        e.load_weights(weights)
        _stream_some(e, img, flow, seg8, slots)
        e.close()
        free.append(hip_free_bytes())
    assert free[2] == free[1] == free[0], free               # create / stream / close: back to the baseline
    held = {}
    for labels, s in (("f32", seg), ("u8", seg8)):
        e = Engine(cfg, H, W, B, labels=labels)
        e.load_weights(weights)
        _stream_some(e, img, flow, s, slots)
        held[labels] = free[0] - hip_free_bytes()
        e.close()
    assert hip_free_bytes() == free[0]
    saved = held["f32"] - held["u8"]
    # plane_bytes: a window's label maps are 3 H W x 4 bytes as floats and 3 H W as bytes, 9 H W saved per window of max_batch, in
    # every streaming slot's staging set and in each of the range guard's eight snapshots (built for the first ticketed davo_submit):
    # 9 x 128 x 416 x 4 x 12 = 23,003,136 B here.  The allocator hands memory out in 2 MiB granules and serves small buffers from
    # pools (measured on an MI355X: 702,545,920 B against 660,602,880 B held, 41,943,040 B = twenty granules saved), so the exact
    # figure is printed, not asserted; what is asserted is the bound: at least half of 3 H W x 3 bytes per window and slot.
    exact = 9 * H * W * B * (slots + 8)
    print("device memory held: float labels %d B, byte labels %d B, saved %d B (plane_bytes says %d B)" % (held["f32"], held["u8"], saved, exact))
    assert held["u8"] < held["f32"]
    assert saved >= (3 * H * W * 3 * B * slots) // 2


# ---- the driver -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", ["both", "trajectory"])
def test_the_driver_writes_the_same_files(pairs, tmp_path):
    """run_kitti_pose.main is what `python -m davo_amd.run_kitti_pose' runs; called in this process, like the multi-sequence tests
    do, so that the three launches cost no three interpreter and HIP start-ups."""
    from davo_amd import loader as L, run_kitti_pose as R
    H, W, frames = 36, 100, {3: 7, 4: 6}
    dumps = {"f32": str(tmp_path / "f32"), "u8": str(tmp_path / "u8")}
    for labels, d in dumps.items():
        for seq, n in frames.items():
            L.write_synthetic_dump(d, seq, n, H, W, seed=40 + seq, labels=labels)
    ckpt = str(tmp_path / "w.npz")
    np.savez(ckpt, **synth.make_weights(FLAGSHIP_VERSION))
    files = []
    for dump, labels in (("f32", "f32"), ("f32", "u8"), ("u8", "u8")):
        out = tmp_path / ("out_%s_%s" % (dump, labels))
        args = ["--test_seq", "3,4", "--concat_img_dir", dumps[dump], "--ckpt_file", ckpt, "--output_dir", str(out), "--img_height", str(H),
                "--img_width", str(W), "--batch_size", "2", "--loader_procs", "2", "--pairs", pairs, "--labels", labels]
        try:
            R.main(args)
        except Exception:
            # reported as text: the driver's frames hold views of the loader's shared batch buffers, unmapped by now, and a
            # traceback that prints its frames' arguments would read them
            import traceback
            pytest.fail("run_kitti_pose %s failed:\n%s" % (" ".join(args), traceback.format_exc()), pytrace=False)
        files.append([open(str(out / ("%.2d-pred_kitti_pose.txt" % seq)), "rb").read() for seq in frames])
    assert all(len(f) > 0 for f in files[0])
    assert files[1] == files[0], "float dump, --labels u8"
    assert files[2] == files[0], "byte dump, --labels u8"
