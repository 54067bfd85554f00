"""The depth-source class tables (att_source 11, 12: -se_depth_wo_tgt_to_seg, -se_depth_to_seg) on the GPU, against the
float64 restatement of tests/depth_source_ref.py.  Bars: the project's own - att_table 2e-6 absolute and the packed bar of
tests/layer_check.py, every conv layer under layer_check's bars (a) and (b), poses at tests/helpers.py's parity bar
(1e-4 absolute and relative).  The SE bottleneck kernel is scaled down per batch (depth_source_ref.sensitive_weights) so that
the tables depend on depth; each test that rests on that asserts it on the CPU reference before looking at a GPU result."""
import ctypes

import numpy as np
import pytest

from davo_amd import DAVO, Engine, synth, parse_version, FLAGSHIP_VERSION
from davo_amd.version import NUM_SEG_CLASSES, weight_shapes

import depth_source_ref as D
import layer_check as LC
from helpers import assert_pose_close, ABS_TOL, REL_TOL, hip_free_bytes

pytestmark = pytest.mark.gpu

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
PUBLISHED = BASE + "-se_depth_wo_tgt_to_seg-fc_tanh"
SUBS = ["-se_depth_wo_tgt_to_seg", "-se_depth_to_seg"]
ACTS = ["-fc_tanh", ""]
PRECISIONS = ["f16x3", "f32"]
# excitation folded into the squeeze launch (B <= 2) and as a launch of its own (B = 4, 32), and a small odd shape
SHAPES = [(128, 416, 1), (128, 416, 2), (128, 416, 4), (128, 416, 32), (36, 100, 3)]


def _engine(cfg, H, W, B, weights, precision):
    e = Engine(cfg, H, W, B)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


def _inputs(B, H, W, first_window=0):
    img, flow, seg = synth.make_inputs(B, H, W, first_window=first_window)
    seg[0, 0, :3, :5] = np.nan                  # labels outside the 19 classes: no table row
    seg[-1, 2, :2] = 19.0
    return img, flow, seg, synth.make_depth(B, H, W, first_window=first_window)


def _rows(cfg):
    return [0, 1, 2] if cfg.tgt_attended else [1, 2]


def _assert_depth_matters(cfg, depth, weights, factor=100):
    """condition on the inputs, on the float64 reference: another depth field moves the tables by > factor x TABLE_TOL"""
    a, b = D.class_tables(cfg, depth, weights), D.class_tables(cfg, D.other_depth(depth), weights)
    diff = np.abs(a - b)[:, _rows(cfg)].max()
    assert diff > factor * LC.TABLE_TOL, diff


_CASES = {}


def _case(sub, act, H, W, B, conv):
    """(cfg, inputs, weights, float64 tables, reference poses), shared by the two precisions"""
    key = (sub, act, H, W, B)
    if key not in _CASES:
        cfg = parse_version(BASE + sub + act)
        inputs = _inputs(B, H, W, first_window=5)
        w = D.sensitive_weights(cfg, synth.make_weights(cfg), inputs[3])
        _assert_depth_matters(cfg, inputs[3], w)
        _CASES.clear()                                         # one case at a time: B = 32 at 128x416 is 100 MB of inputs
        _CASES[key] = (cfg, inputs, w, D.class_tables(cfg, inputs[3], w), D.forward(cfg, *inputs, w, conv=conv))
    return _CASES[key]


def _forward(e, inputs):
    """layer_check.forward with depth: one step whatever the batch, and the batch was not re-issued"""
    if inputs[0].shape[0] > 8:
        e.set_option("host_chunk", 0)
    before = e.range_stats()
    got = e.forward(*inputs[:3], depth=inputs[3])
    after = e.range_stats()
    assert after["f32_batches"] == before["f32_batches"] and after["reissued"] == before["reissued"], (before, after, e.range_report())
    return got


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,B", SHAPES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("sub", SUBS)
def test_layer_by_layer(c_oracle, sub, act, H, W, B, precision):
    """The walk of layer_check.check_forward written out for four inputs: att_table, packed, every conv layer against a
    float64 convolution of the GPU's own input to it (on the first and the last pair image), and the poses."""
    cfg, inputs, w, want_tab, want_pose = _case(sub, act, H, W, B, c_oracle.conv2d_same)
    what = "%s%s %dx%d B=%d %s" % (sub, act, H, W, B, precision)
    e = _engine(cfg, H, W, B, w, precision)
    e.set_option("fuse_pose", 0)                               # cnv7 is stored: the last layer is checked like the others
    poses = _forward(e, inputs)
    folded = "se_excite" not in _profiled_kernels(e, inputs)
    assert folded == (B <= 2), what
    poses2 = _forward(e, inputs)
    assert np.array_equal(poses, poses2)
    NB = 2 * B
    err = LC.check_table(e.debug_read("att_table", (B, 3, NUM_SEG_CLASSES)), want_tab, _rows(cfg), what)
    print("%s: att_table max|err| %.3g (bar %.1g)" % (what, err, LC.TABLE_TOL))
    if not cfg.tgt_attended:
        assert np.array_equal(e.debug_read("att_table", (B, 3, NUM_SEG_CLASSES))[:, 0], np.ones((B, NUM_SEG_CLASSES), np.float32))
    sh = LC.shapes(cfg, H, W)
    want_p = D.pack(cfg, *inputs, w).reshape(NB, H, W, 10)[..., LC.PACK8]
    acts = {"packed": e.debug_read("packed", (NB,) + sh["packed"])}
    LC.check_packed(acts["packed"], want_p, what)
    images = sorted({0, NB - 1})
    acts["packed"] = acts["packed"][images]
    shifts = e.activation_range()[1] if precision == "f16x3" else {}
    for name, prev, stride, rate, groups in LC.layers(cfg, w):
        floor = LC.STORE_FLOOR * 2.0 ** -shifts.get(name, 0) if precision == "f16x3" else 0.0
        acts[name] = e.debug_read(name, (NB,) + sh[name])[images]
        LC.check_layer(name, acts[name], acts[prev], groups, stride, rate, LC.TAU[precision][name], what, floor)
        del acts[prev]
    LC.check_pose(np.asarray(poses, np.float64).reshape(NB, 6)[images], LC.pose_from_cnv7(acts["cnv7"], w), what + " pose head")
    perr = assert_pose_close(poses, want_pose, what)
    print("%s: pose max|err| %.3g" % (what, perr))
    e.set_option("fuse_pose", 1)                               # the default plan (fused pose head where the map allows)
    assert_pose_close(_forward(e, inputs), want_pose, what + " fuse_pose 1")
    e.close()


def _profiled_kernels(e, inputs):
    e.profile(1)
    e.profile_reset()
    e.forward(*inputs[:3], depth=inputs[3])
    names = {k for k, (n, _) in e.profile_entries().items() if n > 0}
    e.profile(0)
    assert "se_depth_squeeze" in names and "se_class_squeeze" not in names and "se_squeeze_partial" not in names, names
    return names


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("sub", SUBS)
def test_entry_points_agree_to_the_bit(sub, precision):
    """davo_forward_depth, davo_forward_device_depth and davo_submit_depth on the same batch; DAVO's class surface with
    arrays, with inputs= and with an iterator of 4-tuples."""
    cfg = parse_version(BASE + sub + "-fc_tanh")
    B, H, W = 3, 64, 96
    inputs = _inputs(B, H, W)
    w = D.sensitive_weights(cfg, synth.make_weights(cfg), inputs[3])
    e = _engine(cfg, H, W, B, w, precision)
    host = e.forward(*inputs[:3], depth=inputs[3])
    bufs = [e.alloc(a.nbytes).upload(a) for a in inputs] + [e.alloc(B * 2 * 6 * 4)]
    e.forward_device(B, bufs[0], bufs[1], bufs[2], bufs[4], depth=bufs[3])
    e.synchronize()
    assert np.array_equal(bufs[4].download((B, 2, 6)), host)
    ms = e.forward_device(B, bufs[0], bufs[1], bufs[2], bufs[4], timed=True, depth=bufs[3])
    assert ms > 0 and np.array_equal(bufs[4].download((B, 2, 6)), host)
    for b in bufs:
        b.free()
    out = np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*inputs[:3], out, depth=inputs[3])
    e.wait()
    assert np.array_equal(out, host)
    shifts = e.calibrate(*inputs[:3], depth=inputs[3])
    assert set(shifts) == set(e.LAYERS)
    with pytest.raises(ValueError, match="depth"):
        e.forward(*inputs[:3])
    with pytest.raises(ValueError, match="depth shape"):
        e.forward(*inputs[:3], depth=inputs[3][:, :2])
    e.close()
    system = DAVO(version=cfg.version)
    system.setup_inference(H, W, "davo", 3, B, inputs[0], input_flow=inputs[1], input_seglabel=inputs[2], input_depth=inputs[3])
    system.load_weights(w)
    system.engine.set_precision(precision)
    system.calibrate(inputs)
    a = system.inference(None, mode="pose")["pose"]
    b = system.inference(None, mode="pose", inputs=inputs)["pose"]
    assert np.array_equal(a, b)
    assert_pose_close(a, host, "DAVO.inference")               # (scales calibrated: float32 rounding apart from `host')
    with pytest.raises(ValueError, match="depth"):
        system.inference(None, mode="pose", inputs=inputs[:3])
    it = DAVO(version=cfg.version)
    it.setup_inference(H, W, "davo", 3, B, iter([inputs, inputs]))
    it.load_weights(w)
    it.engine.set_precision(precision)
    p0, p1 = it.inference()["pose"], it.inference()["pose"]
    assert np.array_equal(p0, p1) and np.array_equal(p0, host)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B", [32, 1])
def test_repeated_forwards_are_bit_identical_and_the_table_ignores_fold_tails(B, precision):
    cfg = parse_version(BASE + "-se_depth_to_seg-fc_tanh")
    H, W = 128, 416
    inputs = _inputs(B, H, W)
    w = D.sensitive_weights(cfg, synth.make_weights(cfg), inputs[3])
    _assert_depth_matters(cfg, inputs[3], w)
    e = _engine(cfg, H, W, B, w, precision)
    first = _forward(e, inputs)
    tab = e.debug_read("att_table", (B, 3, NUM_SEG_CLASSES))
    for _ in range(20):
        assert np.array_equal(_forward(e, inputs), first)
        assert np.array_equal(e.debug_read("att_table", (B, 3, NUM_SEG_CLASSES)), tab)
    for fold in (0, 2, -1):
        e.set_option("fold_tails", fold)
        assert np.array_equal(_forward(e, inputs), first), fold
        assert np.array_equal(e.debug_read("att_table", (B, 3, NUM_SEG_CLASSES)), tab), fold
    e.close()


def _rescaled(weights, shift):
    """the same network with cnv3's activations 2^shift larger (ReLU is homogeneous): trips the f16x3 range guard"""
    w = dict(weights)
    s = np.float32(2.0 ** shift)
    w["pose_exp_net/cnv3/weights"] = weights["pose_exp_net/cnv3/weights"] * s
    w["pose_exp_net/cnv3/biases"] = weights["pose_exp_net/cnv3/biases"] * s
    w["pose_exp_net/cnv4/weights"] = weights["pose_exp_net/cnv4/weights"] / s
    return w


@pytest.mark.parametrize("sub", SUBS)
def test_recovery_reissues_a_batch_on_its_own_depth(c_oracle, sub):
    """A checkpoint whose cnv3 activations leave the fp16-pair range on the first batch.  Batch A is submitted with hold = 0,
    its depth array overwritten at once with another field and handed to batch B: A is re-issued at its verdict from the
    context's copy of its inputs - the depth planes among them.  The same through davo_forward_device_depth, where the upload
    of the other field is ordered behind the batch on the context's stream (no timing involved)."""
    cfg = parse_version(BASE + sub + "-fc_tanh")
    B, H, W = 2, 64, 96
    A = _inputs(B, H, W, first_window=0)
    Bt = _inputs(B, H, W, first_window=7)
    depth_b = D.other_depth(A[3])
    w = D.sensitive_weights(cfg, synth.make_weights(cfg), A[3])
    conv = c_oracle.conv2d_same
    want_a = D.forward(cfg, *A, w, conv=conv)
    wrong_a = D.forward(cfg, *A[:3], depth_b, w, conv=conv)
    want_b = D.forward(cfg, *Bt[:3], depth_b, w, conv=conv)
    bar = max(ABS_TOL, REL_TOL * np.abs(want_a).max())
    assert np.abs(wrong_a - want_a).max() > 10 * bar, (np.abs(wrong_a - want_a).max(), bar)       # before any GPU result
    e = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    depth_buf = A[3].copy()
    out_a, out_b = np.full((B, 2, 6), np.nan, np.float32), np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*A[:3], out_a, hold=0, depth=depth_buf)
    depth_buf[...] = depth_b                                    # consumed: the caller recycles the depth buffer at once
    e.submit(*Bt[:3], out_b, hold=0, depth=depth_buf)           # ... and the slot's staging set takes B's planes behind A's kernels
    e.wait(0)
    assert e.range_stats()["reissued"] >= 1, e.range_stats()
    assert_pose_close(out_a, want_a, "batch A, re-issued")
    assert_pose_close(out_b, want_b, "batch B")
    # the device entry point: the caller's device buffers are recycled behind the batch on the stream
    e2 = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    d = [e2.alloc(a.nbytes).upload(a) for a in A] + [e2.alloc(B * 2 * 6 * 4)]
    e2.forward_device(B, d[0], d[1], d[2], d[4], depth=d[3])
    d[3].upload(depth_b)                                        # ordered behind the batch on the context's stream
    e2.synchronize()
    assert e2.range_stats()["reissued"] >= 1
    assert_pose_close(d[4].download((B, 2, 6)), want_a, "davo_forward_device_depth, re-issued")
    for b in d:
        b.free()
    e.close()
    e2.close()


def _equivalent_weights(cfg, static_weights):
    w = {k: v for k, v in static_weights.items() if "seg_channel_weight" not in k}
    for name, shape in weight_shapes(cfg).items():
        if name.startswith("pose_exp_net/se_depth/"):
            w[name] = np.zeros(shape, np.float32)
    w["pose_exp_net/se_depth/recover_fc/bias"] = static_weights["pose_exp_net/pose_exp_net/seg_channel_weight/weight"].copy()
    return w


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("sub,static", [("-se_depth_wo_tgt_to_seg", "-static"), ("-se_depth_to_seg", "")])
def test_zero_kernels_reproduce_the_static_attention_to_the_bit(sub, static, precision):
    """Zero SE kernels and recover_fc/bias = the static weight vector: the same mask_pack input and the same launches as
    -segmask_all-static / -segmask_all.  B = 2 (excitation folded) and B = 5 (a launch of its own), host and submit paths."""
    cfg, scfg = parse_version(BASE + sub + "-fc_tanh"), parse_version(BASE + static)
    ws = synth.make_weights(scfg)
    w = _equivalent_weights(cfg, ws)
    img, flow, seg, depth = _inputs(5, 64, 96)
    es, ec = _engine(scfg, 64, 96, 5, ws, precision), _engine(cfg, 64, 96, 5, w, precision)
    for B in (2, 5):
        a, b = es.forward(img[:B], flow[:B], seg[:B]), ec.forward(img[:B], flow[:B], seg[:B], depth=depth[:B])
        assert np.array_equal(a, b), (B, np.abs(a - b).max())
        oa, ob = np.empty((B, 2, 6), np.float32), np.empty((B, 2, 6), np.float32)
        es.submit(img[:B], flow[:B], seg[:B], oa)
        ec.submit(img[:B], flow[:B], seg[:B], ob, depth=depth[:B])
        es.wait()
        ec.wait()
        assert np.array_equal(oa, a) and np.array_equal(ob, a)
    es.close()
    ec.close()


def test_three_input_entry_points_refuse_a_depth_context_and_depth_forms_serve_the_flagship():
    vp = ctypes.c_void_p
    B, H, W = 2, 64, 96
    img, flow, seg, depth = _inputs(B, H, W)
    cfg = parse_version(PUBLISHED)
    e = _engine(cfg, H, W, B, synth.make_weights(cfg), "f16x3")
    out = np.empty((B, 2, 6), np.float32)
    ptr = lambda a: a.ctypes.data_as(vp)       # noqa: E731
    bufs = [e.alloc(a.nbytes).upload(a) for a in (img, flow, seg)] + [e.alloc(out.nbytes)]
    calls = {"davo_forward": lambda: e._L.davo_forward(e._ctx, B, ptr(img), ptr(flow), ptr(seg), ptr(out)),
             "davo_submit": lambda: e._L.davo_submit(e._ctx, B, ptr(img), ptr(flow), ptr(seg), ptr(out), 0),
             "davo_forward_device": lambda: e._L.davo_forward_device(e._ctx, B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, None),
             "davo_calibrate": lambda: e._L.davo_calibrate(e._ctx, B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None)}
    for name, call in calls.items():
        rc = call()
        assert rc == -1, (name, rc)                            # DAVO_ERR_INVALID
        with pytest.raises(ValueError, match=name + "_depth"):
            e._check(rc)
    assert e.pending() == 0
    rc = e._L.davo_forward_depth(e._ctx, B, ptr(img), ptr(flow), ptr(seg), None, ptr(out))
    with pytest.raises(ValueError, match="null depth"):
        e._check(rc)
    for b in bufs:
        b.free()
    e.close()
    # the flagship through the `_depth' forms, depth NULL and non-NULL: ignored, same bits as the three-input forms
    fcfg = parse_version(FLAGSHIP_VERSION)
    f = _engine(fcfg, H, W, B, synth.make_weights(fcfg), "f16x3")
    want = f.forward(img, flow, seg)
    for dp in (None, ptr(depth)):
        got = np.full((B, 2, 6), np.nan, np.float32)
        f._check(f._L.davo_forward_depth(f._ctx, B, ptr(img), ptr(flow), ptr(seg), dp, ptr(got)))
        assert np.array_equal(got, want)
        got[...] = np.nan
        f._check(f._L.davo_submit_depth(f._ctx, B, ptr(img), ptr(flow), ptr(seg), dp, ptr(got), 0))
        f.wait()
        assert np.array_equal(got, want)
    bufs = [f.alloc(a.nbytes).upload(a) for a in (img, flow, seg)] + [f.alloc(out.nbytes)]
    f._check(f._L.davo_forward_device_depth(f._ctx, B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, bufs[3].ptr, None))
    f.synchronize()
    assert np.array_equal(bufs[3].download((B, 2, 6)), want)
    shifts = (ctypes.c_int * 6)()
    f._check(f._L.davo_calibrate_depth(f._ctx, B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None, shifts))
    assert np.array_equal(f.forward(img, flow, seg, depth=depth), f.forward(img, flow, seg))      # Python: ignored as well
    for b in bufs:
        b.free()
    f.close()


def test_create_and_close_leaves_no_device_memory_behind():
    """Ten depth engines that each stream two batches and recover the first: staging sets, the snapshot ring (depth planes
    included), the records' host mirror - everything goes with the context."""
    cfg = parse_version(BASE + "-se_depth_to_seg-fc_tanh")
    B, H, W = 2, 64, 96
    inputs = _inputs(B, H, W)
    w = _rescaled(D.sensitive_weights(cfg, synth.make_weights(cfg), inputs[3]), 16)
    free = []
    for _ in range(10):
        e = _engine(cfg, H, W, B, w, "f16x3")
        e.set_inflight(2)
        outs = [np.empty((B, 2, 6), np.float32) for _ in range(2)]
        for out in outs:
            e.submit(*inputs[:3], out, depth=inputs[3])
        e.wait()
        e.synchronize()
        assert e.range_stats()["reissued"] >= 1
        e.close()
        free.append(hip_free_bytes())
    assert free[9] == free[0], free


def test_cli_runs_the_published_depth_variant_from_a_dump(tmp_path, c_oracle):
    """run_kitti_pose --version <published string> on a dump with -monodepth2_depth.npy files and a TF bundle: the trajectory
    matches the restatement on the same decoded files (default loader: worker processes filling shared buffers, depth among
    them; then the threaded loader)."""
    from davo_amd import run_kitti_pose, sequence as S, loader as L, tf_checkpoint as T
    cfg = parse_version(PUBLISHED)
    H, W, NF = 64, 96, 9
    dump = str(tmp_path / "dump")
    L.write_synthetic_dump(dump, 9, NF, H, W, depth=True)
    load = S.kitti_window_loader(dump, 9, NF, H, W, depth=True)
    weights = D.sensitive_weights(cfg, synth.make_weights(cfg), load(0, NF - 2)[3])
    _assert_depth_matters(cfg, load(0, NF - 2)[3], weights)
    ck = tmp_path / "ckpt"
    ck.mkdir()
    T.write_checkpoint(str(ck / "model-1"), weights)
    run_kitti_pose.main(["--concat_img_dir", dump, "--ckpt_file", str(ck), "--output_dir", str(tmp_path), "--version", PUBLISHED,
                         "--test_seq", "9", "--batch_size", "4", "--img_height", str(H), "--img_width", str(W)])
    got = S.read_kitti_poses(str(tmp_path / "09-pred_kitti_pose.txt"))
    run_kitti_pose.main(["--concat_img_dir", dump, "--ckpt_file", str(ck), "--output_dir", str(tmp_path / "threaded"), "--version", PUBLISHED,
                         "--test_seq", "9", "--batch_size", "4", "--img_height", str(H), "--img_width", str(W), "--loader_procs", "0"])
    assert np.array_equal(S.read_kitti_poses(str(tmp_path / "threaded" / "09-pred_kitti_pose.txt")), got)
    infer = lambda img, flow, seg, depth: D.forward(cfg, img, flow, seg, depth, weights, conv=c_oracle.conv2d_same)   # noqa: E731
    want, poses = S.run_sequence(infer, load.__call__, NF, 4)
    assert got.shape == (NF, 4, 4) and np.abs(got - np.array(want)).max() <= ABS_TOL
    # ... and the poses themselves at the parity bar, through the same loader and the class surface
    system = DAVO(version=PUBLISHED)
    system.setup_inference(H, W, "davo", 3, NF - 2)
    system.load_weights(weights)
    assert_pose_close(system.inference(None, "pose", inputs=load(0, NF - 2))["pose"], poses, "poses from the dump")
