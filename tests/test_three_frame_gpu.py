"""The three-frame PoseNN (`-dilatedPoseNN' without `-sharedNN'; davo_set_posenn_topology) on the GPU against the float64
restatement of tests/three_frame_ref.py.

Layer by layer with tests/layer_check.py's functions, each launch judged on the GPU's own input to it (Engine.debug_read):
  packed    against pack15 in the library's 16-channel order at PACKED_TOL; in float32 to the bit against the float32 products of
            the GPU's own tables;
  cnv1      against the float64 convolution of the GPU's packed tensor under TAU's cnv1 bar, on both arms of "patch_cnv1_t"
            (conv_patch_cnv1t_h3 and the implicit GEMM at cin = 16), which agree within 2e-6 of max|cnv1|;
  cnv2..7   under their existing bars; the six-column pose head from the GPU's cnv7 at POSE_REL;
and the poses end to end at tests/helpers.py's parity bar.  The conditions on the inputs are asserted on the restatement alone in
tests/test_three_frame.py."""
import ctypes
import os

import numpy as np
import pytest

import davo_amd
from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION, labels_to_u8, flow_to_f16
from davo_amd import loader as L
from davo_amd import sequence as S

import layer_check as LC
import three_frame_cases as K
import three_frame_ref as T
from helpers import assert_pose_close, hip_free_bytes
from test_stream import _rescaled

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "f32"]
PATCH_PLAN_ID = 96                       # last_plan(0)'s tile id of conv_patch_cnv1t_h3 (the implicit GEMM reports its tile's)
ARMS_REL = 2e-6                          # the two cnv1 arms against each other: test_patch_kernels_match_implicit_gemm's bar
INVALID = -1                             # DAVO_ERR_INVALID


def _engine(cfg, H, W, max_batch, weights, precision, **kw):
    e = Engine(cfg, H, W, max_batch, **kw)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


@pytest.fixture(scope="module", autouse=True)
def flagship_before():
    """One flagship forward before any three-frame engine exists in this process (the module's first act)."""
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, B = K.SMALL
    inp = K.inputs(H, W, B)
    out = {}
    for precision in PRECISIONS:
        e = _engine(cfg, H, W, B, synth.make_weights(cfg), precision)
        out[precision] = (e.forward(*inp), [e.last_plan(li) for li in range(7)])
        e.close()
    return out


def _shapes(H, W):
    sh = dict(LC.shapes(parse_version(FLAGSHIP_VERSION), H, W))
    sh["packed"] = (H, W, 16)
    return sh


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,B", K.SHAPES, ids=K.IDS)
def test_layer_by_layer(H, W, B, precision):
    cfg, inp, w = K.case(H, W, B)
    img, flow, seg = inp
    what = "%dx%d B=%d %s" % (H, W, B, precision)
    sh = _shapes(H, W)
    e = _engine(cfg, H, W, B, w, precision)
    arms = {}
    for arm in ((1, 0) if precision == "f16x3" else (0,)):       # float32 has the implicit GEMM alone
        e.set_option("patch_cnv1_t", arm)
        poses = LC.forward(e, *inp)
        plan = e.last_plan(0)
        assert (plan[0][1] == PATCH_PLAN_ID) == bool(arm), (what, arm, plan)
        arms[arm] = (poses, e.debug_read("cnv1", (B,) + sh["cnv1"]))
    # -- the tables and the packed tensor
    want_tab, rows = LC.ref_tables(cfg, img, flow, seg, w)
    tab = e.debug_read("att_table", (B, 3, 19))
    LC.check_table(tab, want_tab, rows, what)
    packed = e.debug_read("packed", (B,) + sh["packed"])
    want_p = T.pack16(T.pack15(cfg, *inp, w), cfg)
    err = LC.check_packed(packed, want_p, what)
    print("%s: packed max|err| %.3g" % (what, err))
    assert set(np.unique(seg[0]).astype(int)) >= set(range(19)) | {255}
    if precision == "f32":                                       # one float32 product per value, from the GPU's own tables
        tab32 = tab.copy()
        tab32[:, 0] = 1.0                                        # se_flow: the target's row is implied ones
        bits = T.pack16(T.pack15(cfg, *inp, w, dtype=np.float32, tab=tab32), cfg)
        assert bits.dtype == np.float32 and np.array_equal(packed, bits), what
    # -- cnv1 on both arms, from the GPU's packed tensor
    shifts = e.activation_range()[1] if precision == "f16x3" else {}
    floor = lambda name: LC.STORE_FLOOR * 2.0 ** -shifts.get(name, 0) if precision == "f16x3" else 0.0      # noqa: E731
    lay = T.layers(cfg, w)
    name, _, stride, rate, groups = lay[0]
    for arm, (_, c1) in arms.items():
        a, b = LC.check_layer("cnv1", c1, packed, groups, stride, rate, LC.TAU[precision]["cnv1"], "%s patch_cnv1_t %d" % (what, arm), floor("cnv1"))
        print("CNV1_WORST %s patch_cnv1_t %d: bar (a) %.3g, bar (b) %.3g of the L1 mass (tau %.3g)" % (what, arm, a, b, LC.TAU[precision]["cnv1"]))
    if len(arms) == 2:
        d = float(np.abs(arms[1][1].astype(np.float64) - arms[0][1]).max())
        scale = float(np.abs(arms[0][1]).max())
        print("%s: cnv1 arms differ by %.3g of max|cnv1|" % (what, d / scale))
        assert d <= ARMS_REL * scale, (what, d, scale)
        assert_pose_close(arms[1][0], arms[0][0], what + " the two arms' poses")
    # -- cnv2..cnv7 of the last forward (arm 0), each from the GPU's own input
    acts = {"cnv1": arms[0][1]}
    for name, prev, stride, rate, groups in lay[1:]:
        acts[name] = e.debug_read(name, (B,) + sh[name])
        LC.check_layer(name, acts[name], acts[prev], groups, stride, rate, LC.TAU[precision][name], what, floor(name))
        del acts[prev]
    # -- the six-column pose head from the GPU's cnv7, and the poses end to end
    poses = arms[0][0]
    LC.check_pose(poses, T.pose_from_cnv7(acts["cnv7"], w), what + " pose head")
    want = K.reference(H, W, B)
    for arm, (p, _) in arms.items():
        perr = assert_pose_close(p, want, "%s patch_cnv1_t %d" % (what, arm))
        print("%s patch_cnv1_t %d: pose max|err| %.3g of max|pose| %.3g" % (what, arm, perr, np.abs(want).max()))
    e.set_option("fuse_pose", 1)                                 # accepted, no effect: cnv7 stays stored
    assert np.array_equal(LC.forward(e, *inp), arms[0][0])
    e.debug_read("cnv7", (B,) + sh["cnv7"])
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("version", K.VERSIONS)
def test_the_six_versions(version, precision):
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B, version)
    e = _engine(cfg, H, W, B, w, precision)
    got = e.forward(*inp)
    want = K.reference(H, W, B, version)
    err = assert_pose_close(got, want, "%s %s" % (version, precision))
    print("%s %s: pose max|err| %.3g of max|pose| %.3g" % (version, precision, err, np.abs(want).max()))
    want_tab, rows = LC.ref_tables(cfg, *inp, w)
    LC.check_table(e.debug_read("att_table", (B, 3, 19)), want_tab, rows, version)
    LC.check_packed(e.debug_read("packed", (B, H, W, 16)), T.pack16(T.pack15(cfg, *inp, w), cfg), version)
    e.close()


# ---- entry points, to the bit against davo_forward ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_and_streaming_entry_points_and_repeats(precision):
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, precision)
    first = e.forward(*inp)
    assert_pose_close(first, K.reference(H, W, B), precision)
    for _ in range(50):
        assert np.array_equal(e.forward(*inp), first)
    e.set_option("host_chunk", 1)                                # one window per sub-batch
    assert np.array_equal(e.forward(*inp), first)
    e.set_option("host_chunk", 8)
    bufs = [e.alloc(a.nbytes).upload(a) for a in inp]
    d_pose = e.alloc(B * 12 * 4)
    e.forward_device(B, *bufs, d_pose)
    e.synchronize()
    assert np.array_equal(d_pose.download((B, 2, 6)), first)
    out = np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*inp, out)
    e.wait()
    assert np.array_equal(out, first)
    e.set_inflight(2)
    outs = [np.full((B, 2, 6), np.nan, np.float32) for _ in range(3)]
    for o in outs:
        e.submit(*inp, o)
    e.wait()
    assert all(np.array_equal(o, first) for o in outs)
    for b in bufs + [d_pose]:
        b.free()
    e.close()


@pytest.mark.parametrize("labels,flow_fmt", [("f32", "f32"), ("u8", "f16")])
def test_frame_entry_points_and_the_narrow_formats(labels, flow_fmt):
    """The three `_frames' calls against davo_forward on windows_from_frames of the same arrays, in the default formats and with
    byte labels and binary16 flow; the narrow formats against the float32 engine on the rounded flow."""
    H, W, N = 36, 100, 3
    cfg = parse_version(K.FLAGSHIP3)
    w = K.weights(K.FLAGSHIP3)
    fr = synth.make_frames(N + 2, H, W, labels=labels, flow=flow_fmt)
    win = davo_amd.windows_from_frames(*fr)
    e = _engine(cfg, H, W, N, w, "f16x3", labels=labels, flow=flow_fmt)
    want = e.forward(*win)
    assert np.array_equal(e.forward_frames(*fr), want)
    out = np.full((N, 2, 6), np.nan, np.float32)
    e.submit_frames(*fr, out)
    e.wait()
    assert np.array_equal(out, want)
    bufs = [e.alloc(a.nbytes).upload(a) for a in fr]
    d_pose = e.alloc(N * 12 * 4)
    e.forward_device_frames(N, *bufs, d_pose)
    e.synchronize()
    assert np.array_equal(d_pose.download((N, 2, 6)), want)
    for b in bufs + [d_pose]:
        b.free()
    e.close()
    if labels == "u8":                                           # the same network on float labels and the widened flow: the same bits
        fr32 = synth.make_frames(N + 2, H, W)
        assert np.array_equal(labels_to_u8(fr32[2]), fr[2]) and np.array_equal(flow_to_f16(fr32[1]), fr[1])
        win32 = davo_amd.windows_from_frames(fr32[0], fr[1].astype(np.float32), fr32[2])
        f = _engine(cfg, H, W, N, w, "f16x3")
        assert np.array_equal(f.forward(*win32), want)
        f.close()
    assert_pose_close(want, T.forward(cfg, win[0], np.asarray(win[1], np.float32), np.asarray(win[2], np.float32), w), "frames %s %s" % (labels, flow_fmt))


# ---- range recovery -------------------------------------------------------------------------------------------------------
def test_a_checkpoint_that_leaves_the_range_is_reissued_and_meets_the_bar():
    """tests/test_stream.py's rescaling (cnv3's activations 2^16 larger, undone in cnv4: the same function) through the host and
    the ticketed streaming path of a three-frame engine."""
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    want = K.reference(H, W, B)
    e = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    before = e.range_stats()
    assert_pose_close(e.forward(*inp), want, "rescaled, davo_forward")
    mid = e.range_stats()
    assert mid["reissued"] > before["reissued"] and mid["recalibrations"] > before["recalibrations"], (before, mid, e.range_report())
    assert mid["f32_batches"] == 0
    e.close()
    e = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    out = np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*inp, out)
    e.wait()
    e.synchronize()
    assert_pose_close(out, want, "rescaled, davo_submit")
    assert e.range_stats()["reissued"] > 0
    shifts = e.calibrate(*inp)                                   # davo_calibrate on a three-frame context
    assert shifts["cnv3"] < 0, shifts
    e.close()


# ---- error codes ------------------------------------------------------------------------------------------------------------
def test_error_codes():
    H, W, B = 16, 16, 1
    cfg, inp, w = K.case(16, 16, 3)
    e = _engine(cfg, H, W, B, w, "f16x3")
    for topology in (0, 1):                                      # after a weight
        rc = e._L.davo_set_posenn_topology(e._ctx, topology)
        assert rc == INVALID
        with pytest.raises(ValueError, match="before the first davo_load_weight"):
            e._check(rc)
    for pairs in ("src0", "src1"):
        with pytest.raises(ValueError, match="both poses"):
            e.set_pairs(pairs)
    e.set_pairs("both")
    with pytest.raises(ValueError, match="impl 1"):
        e.set_impl("direct")
    with pytest.raises(ValueError, match="feature export"):
        e.set_feature_export(True)
    with pytest.raises(ValueError, match="heat export"):
        e.set_heat_export(True)
    assert e._L.davo_set_posenn_se(e._ctx, 1) == INVALID
    e.set_feature_export(False)
    e.set_heat_export(False)
    assert_pose_close(e.forward(*[a[:1] for a in inp]), K.reference(16, 16, 3)[:1], "after the refused calls")
    e.close()
    # a fresh context: out-of-range values, and what must precede the call
    raw = Engine(parse_version(K.FLAGSHIP3.replace("-dilatedPoseNN", "-sharedNN-dilatedPoseNN")), H, W, B)
    assert raw._L.davo_set_posenn_topology(raw._ctx, 2) == INVALID and raw._L.davo_set_posenn_topology(raw._ctx, -1) == INVALID
    raw.set_pairs("src1")
    assert raw._L.davo_set_posenn_topology(raw._ctx, 1) == INVALID            # pairs other than both
    raw.set_pairs("both")
    assert raw._L.davo_set_posenn_topology(raw._ctx, 1) == 0 and raw._L.davo_set_posenn_topology(raw._ctx, 0) == 0
    # the pair network's cnv1 kernel is refused by a triplet context and the other way round
    k10 = np.zeros((7, 7, 10, 16), np.float32)
    load = lambda eng, a: eng._L.davo_load_weight(eng._ctx, b"pose_exp_net/cnv1/weights", a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)),      # noqa: E731
                                                  (ctypes.c_int64 * 4)(*a.shape), 4)
    assert raw._L.davo_set_posenn_topology(raw._ctx, 1) == 0
    assert load(raw, k10) == INVALID and load(raw, np.zeros((7, 7, 15, 16), np.float32)) == 0
    raw.close()
    se = Engine(parse_version("v1-sharedNN-dilatedPoseNN-no_segmask-se_insert"), H, W, B)      # after davo_set_posenn_se(ctx, 1)
    assert se._L.davo_set_posenn_topology(se._ctx, 1) == INVALID
    se.close()
    depth = Engine(parse_version("v1-sharedNN-dilatedPoseNN-segmask_all-se_depth_to_seg"), H, W, B)      # att_source 12
    assert depth._L.davo_set_posenn_topology(depth._ctx, 1) == INVALID
    depth.close()
    d = davo_amd.DAVO(K.FLAGSHIP3)
    d.setup_inference(H, W, 'davo', 3, B)
    with pytest.raises(ValueError, match="feature export"):      # the library's message
        d.enable_feature_mode()
    with pytest.raises(ValueError, match="heat export"):
        d.enable_feature_mode(features='heat')
    d.engine.close()


def test_the_davo_class_runs_pose_inference():
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    d = davo_amd.DAVO(K.FLAGSHIP3)
    d.setup_inference(H, W, 'davo', 3, B, input_img_uint8=inp[0], input_flow=inp[1], input_seglabel=inp[2])
    d.load_weights(w)
    assert_pose_close(d.inference(mode='pose')['pose'], K.reference(H, W, B), "DAVO.inference")
    d.engine.close()


def test_create_and_close_leaves_no_device_memory_behind():
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    free = []
    for _ in range(10):
        e = _engine(cfg, H, W, B, w, "f16x3")
        e.set_inflight(2)
        e.forward(*inp)
        out = np.empty((B, 2, 6), np.float32)
        e.submit(*inp, out)
        e.wait()
        e.close()
        free.append(hip_free_bytes())
    assert free[9] == free[0], free


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_flagship_is_untouched(flagship_before, precision):
    """A flagship engine beside a live three-frame engine of the same library: the plan and the bits of the one that ran before
    any such engine existed."""
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    t = _engine(cfg, H, W, B, w, precision)
    t.forward(*inp)
    fcfg = parse_version(FLAGSHIP_VERSION)
    f = _engine(fcfg, H, W, B, synth.make_weights(fcfg), precision)
    poses = f.forward(*inp)
    want_poses, want_plan = flagship_before[precision]
    assert [f.last_plan(li) for li in range(7)] == want_plan and np.array_equal(poses, want_poses)
    f.close()
    t.close()


def test_the_cli_writes_a_trajectory_from_a_dump(tmp_path):
    from davo_amd import run_kitti_pose as R
    H, W, seq, n_frames = 64, 96, 9, 6
    dump = str(tmp_path / "dump")
    L.write_synthetic_dump(dump, seq, n_frames, H, W, seed=1234)
    cfg = parse_version(K.FLAGSHIP3)
    w = K.weights(K.FLAGSHIP3)
    ckpt = str(tmp_path / "w.npz")
    np.savez(ckpt, **w)
    seen = {}
    inner = S.run_sequences

    def capturing(*a, **k):
        for s, traj, poses, timing in inner(*a, **k):
            seen[s] = poses.copy()
            yield s, traj, poses, timing
    S.run_sequences = capturing
    try:
        R.main(["--test_seq", str(seq), "--concat_img_dir", dump, "--ckpt_file", ckpt, "--version", K.FLAGSHIP3, "--batch_size", "2",
                "--output_dir", str(tmp_path / "out"), "--img_height", str(H), "--img_width", str(W), "--loader_procs", "0"])
    finally:
        S.run_sequences = inner
    lines = open(os.path.join(str(tmp_path / "out"), "%.2d-pred_kitti_pose.txt" % seq)).read().splitlines()
    assert len(lines) == n_frames
    fac = S.kitti_window_loader(dump, None, None, H, W)
    windows = (0, n_frames - 3)
    parts = [fac.load_inline(seq, k, k + 1) for k in windows]
    want = T.forward(cfg, *(np.concatenate([p[k] for p in parts]) for k in range(3)), w)
    assert seen[seq].shape == (n_frames - 2, 2, 6)
    assert_pose_close(seen[seq][list(windows)], want, "run_kitti_pose, windows %s" % (windows,))
    R.main(["--test_seq", str(seq), "--synthetic", "5", "--version", K.FLAGSHIP3, "--batch_size", "2",               # synthetic input too
            "--output_dir", str(tmp_path / "out2"), "--img_height", str(H), "--img_width", str(W)])
    assert len(open(os.path.join(str(tmp_path / "out2"), "%.2d-pred_kitti_pose.txt" % seq)).read().splitlines()) == 5
