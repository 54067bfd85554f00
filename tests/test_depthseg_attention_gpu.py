"""The depth-split flow attention (att_source 13: -se_flow_on_depthseg_seplayers) on the GPU, against the float64
restatement of tests/depthseg_attention_ref.py.  Bars: the ones tests/test_depth_source_gpu.py::test_layer_by_layer uses for
the same tensors - att_table (and att_table_far) at layer_check.check_table's 2e-6, packed at layer_check.check_packed's bar,
every conv layer under layer_check's bars (a) and (b) with its TAU, the pose head at layer_check.check_pose, the poses at
tests/helpers.py's parity bar (1e-4 absolute and relative).  Everything else here is an identity to the bit.
Each test asserts, on its own inputs and before it looks at a GPU result, that between 0.3 and 0.8 of every source plane lies
below the threshold: both sides of the select are exercised, or the test fails."""
import ctypes

import numpy as np
import pytest

from davo_amd import DAVO, Engine, synth, parse_version
from davo_amd.version import NUM_SEG_CLASSES, weight_shapes

import depth_source_ref as D
import depthseg_attention_ref as R
import heat_export_ref as HR
import layer_check as LC
from helpers import assert_pose_close, ABS_TOL, REL_TOL, hip_free_bytes

pytestmark = pytest.mark.gpu

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"
SUB = "-se_flow_on_depthseg_seplayers"
FULL = BASE + "-segmask_all" + SUB + "-abs_flow-fc_tanh"
ACTS = ["-fc_tanh", ""]
MASKINGS = ["-segmask_all", "-segmask_rgb"]
PRECISIONS = ["f16x3", "f32"]
SHAPES = [(36, 100, 3), (64, 96, 2), (128, 416, 1)]
TAB = lambda B: (B, 3, NUM_SEG_CLASSES)       # noqa: E731


def _version(masking="-segmask_all", act="-fc_tanh"):
    return BASE + masking + SUB + "-abs_flow" + act


def _engine(cfg, H, W, B, weights, precision):
    e = Engine(cfg, H, W, B)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


def _assert_both_sides(depth, thr):
    shares = R.near_shares(depth, thr)
    assert shares.min() >= 0.3 and shares.max() <= 0.8, shares
    return shares


def _inputs(B, H, W, weights=None, first_window=0):
    img, flow, seg = synth.make_inputs(B, H, W, first_window=first_window)
    seg[0, 0, :3, :5] = np.nan                  # labels outside the 19 classes: no table row on either side
    seg[-1, 2, :2] = 19.0
    seg[0, 2, 5:7, :9] = 255.0
    depth = synth.make_depth(B, H, W, first_window=first_window)
    _assert_both_sides(depth, 15.0 if weights is None else weights[R.THRESHOLD])
    return img, flow, seg, depth


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _forward(e, inputs):
    """one step, and the batch was not re-issued"""
    before = e.range_stats()
    got = e.forward(*inputs[:3], depth=inputs[3])
    after = e.range_stats()
    assert after["f32_batches"] == before["f32_batches"] and after["reissued"] == before["reissued"], (before, after, e.range_report())
    return got


# ---- layer by layer against float64 -------------------------------------------------------------------------------------
_CASES = {}


def _case(masking, act, H, W, B, conv):
    """(cfg, inputs, weights, float64 tables, reference poses), shared by the two precisions"""
    key = (masking, act, H, W, B)
    if key not in _CASES:
        cfg = parse_version(_version(masking, act))
        w = synth.make_weights(cfg)
        inputs = _inputs(B, H, W, w)
        near_t, far_t = R.class_tables(cfg, inputs[1], w)
        assert np.abs(near_t[:, 1:] - far_t[:, 1:]).max() > 100 * LC.TABLE_TOL           # two MLPs that can be told apart
        _CASES.clear()
        _CASES[key] = (cfg, inputs, w, near_t, far_t, R.forward(cfg, *inputs, w, conv=conv))
    return _CASES[key]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,B", SHAPES)
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("masking", MASKINGS)
def test_layer_by_layer(c_oracle, masking, act, H, W, B, precision):
    """tests/test_depth_source_gpu.py::test_layer_by_layer's walk and bars: both tables, packed, every conv layer against a
    float64 convolution of the GPU's own input to it (first and last pair image), the pose head and the poses.  The
    restatement's select compares the float32 depth the device holds with the float32 threshold it was loaded with, so every
    pixel of `packed' is compared."""
    cfg, inputs, w, near_t, far_t, want_pose = _case(masking, act, H, W, B, c_oracle.conv2d_same)
    what = "%s%s %dx%d B=%d %s" % (masking, act, H, W, B, precision)
    e = _engine(cfg, H, W, B, w, precision)
    e.set_option("fuse_pose", 0)                               # cnv7 is stored: the last layer is checked like the others
    poses = _forward(e, inputs)
    assert np.array_equal(poses, _forward(e, inputs))
    NB = 2 * B
    for name, want in (("att_table", near_t), ("att_table_far", far_t)):
        got = e.debug_read(name, TAB(B))
        err = LC.check_table(got, want, [1, 2], what + " " + name)
        print("%s: %s max|err| %.3g (bar %.1g)" % (what, name, err, LC.TABLE_TOL))
        assert np.array_equal(got[:, 0], np.ones((B, NUM_SEG_CLASSES), np.float32)), name       # the target's rows are ones
    sh = LC.shapes(cfg, H, W)
    want_p = R.pack(cfg, *inputs, w).reshape(NB, H, W, 10)[..., LC.PACK8]
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
    e.set_option("fuse_pose", 1)                               # the default plan
    assert_pose_close(_forward(e, inputs), want_pose, what + " fuse_pose 1")
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_reference_layout_packs_the_same_select(precision):
    """davo_set_impl(ctx, 1): mask_pack's LD = 10 form, against the restatement's ten channels"""
    cfg = parse_version(FULL)
    B, H, W = 2, 36, 100
    w = synth.make_weights(cfg)
    inputs = _inputs(B, H, W, w)
    e = _engine(cfg, H, W, B, w, precision)
    e.set_impl("direct")
    poses = _forward(e, inputs)
    got = e.debug_read("packed", (2 * B, H, W, 10))
    LC.check_packed(got, R.pack(cfg, *inputs, w).reshape(2 * B, H, W, 10), "LD 10")
    assert_pose_close(poses, R.forward(cfg, *inputs, w), "impl 1")
    e.close()


# ---- identities to the bit ------------------------------------------------------------------------------------------------
def _flagship_engine(cfg, H, W, B, weights, scope, precision):
    f = parse_version(cfg.version.replace(SUB, "-se_flow"))
    assert f.att_source == "se_flow" and f.as_c_ints()[:5] == cfg.as_c_ints()[:5] and f.as_c_ints()[6:] == cfg.as_c_ints()[6:]
    return _engine(f, H, W, B, R.flagship_weights(weights, scope), precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("B", [3, 1])
def test_equal_mlps_and_infinite_thresholds_are_the_flagship_to_the_bit(B, precision):
    """(a) near weights = far weights: poses, packed and both tables equal a -se_flow engine's with that MLP, on any depth;
    (b) threshold +inf: the near MLP's flagship, -inf: the far MLP's; (c) an all-NaN depth behaves as -inf.  B = 3 runs the
    excitation as launches of its own, B = 1 folded into the squeeze."""
    cfg = parse_version(FULL)
    H, W = 36, 100
    w = synth.make_weights(cfg)
    inputs = _inputs(B, H, W, w)
    NB = 2 * B
    flag = {}
    for scope in R.SCOPES:
        f = _flagship_engine(cfg, H, W, B, w, scope, precision)
        flag[scope] = (f.forward(*inputs[:3]), f.debug_read("packed", (NB, H, W, 8)), f.debug_read("att_table", TAB(B)))
        f.close()
    assert not np.array_equal(flag["se_flow_near"][0], flag["se_flow_far"][0])          # the two MLPs give different poses

    def run(weights, depth):
        e = _engine(cfg, H, W, B, weights, precision)
        out = (e.forward(*inputs[:3], depth=depth), e.debug_read("packed", (NB, H, W, 8)),
               e.debug_read("att_table", TAB(B)), e.debug_read("att_table_far", TAB(B)))
        e.close()
        return out

    def same(got, scope, what):
        assert _same_bits(got[0], flag[scope][0]), what + ": poses"
        assert _same_bits(got[1], flag[scope][1]), what + ": packed"

    other = D.other_depth(inputs[3])
    nan = np.full_like(inputs[3], np.nan)
    for scope in R.SCOPES:                                                              # (a)
        eq = R.with_mlps(w, near=R.mlp_of(w, scope), far=R.mlp_of(w, scope))
        for name, depth in (("own depth", inputs[3]), ("other depth", other), ("NaN depth", nan)):
            got = run(eq, depth)
            same(got, scope, "(a) %s %s" % (scope, name))
            assert _same_bits(got[2], got[3]) and _same_bits(got[2], flag[scope][2]), "(a) tables " + scope
    got = run(w, inputs[3])                                                             # the tables are each MLP's flagship table
    assert _same_bits(got[2], flag["se_flow_near"][2]) and _same_bits(got[3], flag["se_flow_far"][2])
    assert not _same_bits(got[0], flag["se_flow_near"][0]) and not _same_bits(got[0], flag["se_flow_far"][0])
    same(run(R.with_mlps(w, thr=np.inf), inputs[3]), "se_flow_near", "(b) +inf")        # (b)
    same(run(R.with_mlps(w, thr=-np.inf), inputs[3]), "se_flow_far", "(b) -inf")
    same(run(w, nan), "se_flow_far", "(c) NaN depth")                                    # (c)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_swapped_windows_fold_tails_and_repeats(precision):
    """(d) two windows swapped in the batch swap their poses; (e) "fold_tails" 0 and 1 give the same tables and poses;
    (f) 50 repeated forwards at B = 3 are bit-identical."""
    cfg = parse_version(FULL)
    B, H, W = 3, 36, 100
    w = synth.make_weights(cfg)
    inputs = _inputs(B, H, W, w)
    e = _engine(cfg, H, W, B, w, precision)
    first = _forward(e, inputs)
    tabs = (e.debug_read("att_table", TAB(B)), e.debug_read("att_table_far", TAB(B)))
    for _ in range(50):                                                                 # (f)
        assert _same_bits(_forward(e, inputs), first)
    perm = [2, 1, 0]                                                                    # (d)
    swapped = _forward(e, tuple(np.ascontiguousarray(a[perm]) for a in inputs))
    assert _same_bits(swapped, first[perm]) and not _same_bits(first[0], first[2])
    for fold in (0, 1, 2, -1):                                                          # (e)
        e.set_option("fold_tails", fold)
        e.profile(1)
        e.profile_reset()
        assert _same_bits(_forward(e, inputs), first), fold
        names = {k for k, (n, _) in e.profile_entries().items() if n > 0}
        e.profile(0)
        assert "se_squeeze_partial" in names and "mask_pack" in names and "se_depth_squeeze" not in names, names
        assert ("se_excite" in names) == ("se_excite_far" in names) == (fold in (0, -1)), (fold, names)       # B = 3: auto folds nothing
        assert _same_bits(e.debug_read("att_table", TAB(B)), tabs[0]) and _same_bits(e.debug_read("att_table_far", TAB(B)), tabs[1]), fold
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_depth_is_read_per_frame(precision):
    cfg = parse_version(FULL)
    B, H, W = 2, 64, 96
    w = synth.make_weights(cfg)
    img, flow, seg, depth = _inputs(B, H, W, w)
    e = _engine(cfg, H, W, B, w, precision)
    want = e.forward(img, flow, seg, depth=depth)
    exchanged = depth.copy()
    exchanged[:, 0], exchanged[:, 2] = depth[:, 2], depth[:, 0]
    got = e.forward(img, flow, seg, depth=exchanged)
    for b in range(B):
        for row in (0, 1):
            assert not np.array_equal(got[b, row], want[b, row]), (b, row)
    tgt_nan = depth.copy()
    tgt_nan[:, 1] = np.nan
    assert _same_bits(e.forward(img, flow, seg, depth=tgt_nan), want)
    e.close()


# ---- entry points ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_entry_points_agree_to_the_bit(precision):
    cfg = parse_version(FULL)
    B, H, W = 3, 64, 96
    w = synth.make_weights(cfg)
    inputs = _inputs(B, H, W, w)
    e = _engine(cfg, H, W, B, w, precision)
    host = e.forward(*inputs[:3], depth=inputs[3])
    bufs = [e.alloc(a.nbytes).upload(a) for a in inputs] + [e.alloc(B * 2 * 6 * 4)]
    # "host_chunk" 1: three sub-batches of one window, each with its own window of the depth planes.  A sub-batch is a forward
    # of ITS batch size, so window b is to the bit what the other entry points return on that window alone (across batch sizes
    # the convolutions agree to rounding only: split-K moves with the batch, tests/test_feature_export_gpu.py::
    # test_sub_batches_deliver_every_window), and the whole batch's poses at the parity bar
    e.set_option("host_chunk", 1)
    chunked = e.forward(*inputs[:3], depth=inputs[3])
    e.set_option("host_chunk", 8)
    assert_pose_close(chunked, host, "host_chunk 1 against one step")
    for b in range(B):
        one = tuple(np.ascontiguousarray(a[b:b + 1]) for a in inputs)
        assert _same_bits(e.forward(*one[:3], depth=one[3]), chunked[b:b + 1]), b
        for buf, a in zip(bufs, one):
            buf.upload(a)
        e.forward_device(1, bufs[0], bufs[1], bufs[2], bufs[4], depth=bufs[3])
        e.synchronize()
        assert _same_bits(bufs[4].download((1, 2, 6)), chunked[b:b + 1]), b
        out1 = np.full((1, 2, 6), np.nan, np.float32)
        e.submit(*one[:3], out1, depth=one[3])
        e.wait()
        assert _same_bits(out1, chunked[b:b + 1]), b
    for buf, a in zip(bufs, inputs):
        buf.upload(a)
    e.forward_device(B, bufs[0], bufs[1], bufs[2], bufs[4], depth=bufs[3])
    e.synchronize()
    assert _same_bits(bufs[4].download((B, 2, 6)), host)
    ms = e.forward_device(B, bufs[0], bufs[1], bufs[2], bufs[4], timed=True, depth=bufs[3])
    assert ms > 0 and _same_bits(bufs[4].download((B, 2, 6)), host)
    shifts = e.calibrate(*inputs[:3], depth=inputs[3])
    assert set(shifts) == set(e.LAYERS)
    e.set_activation_shifts(None)
    for b in bufs:
        b.free()
    # two in flight, the caller's input buffers recycled at once (hold = 0): batch 2 is another batch in the same arrays
    e.set_inflight(2)
    other = _inputs(B, H, W, w, first_window=7)
    want_other = None
    work = [a.copy() for a in inputs]
    outs = [np.full((B, 2, 6), np.nan, np.float32) for _ in range(3)]
    e.submit(*work[:3], outs[0], hold=0, depth=work[3])
    for dst, src in zip(work, other):
        dst[...] = src
    e.submit(*work[:3], outs[1], hold=0, depth=work[3])
    for dst, src in zip(work, inputs):
        dst[...] = src
    e.submit(*work[:3], outs[2], hold=0, depth=work[3])
    e.wait()
    e.set_inflight(1)
    want_other = e.forward(*other[:3], depth=other[3])
    assert _same_bits(outs[0], host) and _same_bits(outs[2], host) and _same_bits(outs[1], want_other)
    assert not _same_bits(host, want_other)
    with pytest.raises(ValueError, match="depth"):
        e.forward(*inputs[:3])
    e.close()


def test_three_input_forms_weights_and_debug_reads_are_refused_where_they_must():
    vp = ctypes.c_void_p
    cfg = parse_version(FULL)
    B, H, W = 2, 64, 96
    w = synth.make_weights(cfg)
    img, flow, seg, depth = _inputs(B, H, W, w)
    e = Engine(cfg, H, W, B)
    # davo_weights_missing counts the nine down to 0 with the rest
    names = list(weight_shapes(cfg))
    assert e._L.davo_weights_missing(e._ctx) == len(names) == 31
    fp = ctypes.POINTER(ctypes.c_float)
    thr = np.asarray(w[R.THRESHOLD], np.float32).reshape(1).copy()
    one = (ctypes.c_int64 * 1)(1)
    assert e._L.davo_load_weight(e._ctx, R.THRESHOLD.encode(), thr.ctypes.data_as(fp), one, 1) == -1       # rank 1: refused
    with pytest.raises(ValueError, match="shape"):
        e._check(-1)
    for part in R.PARTS:                                                                # none of se_flow/*_fc
        a = np.ascontiguousarray(w["pose_exp_net/se_flow_near/" + part])
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        assert e._L.davo_load_weight(e._ctx, ("pose_exp_net/se_flow/" + part).encode(), a.ctypes.data_as(fp), shape, a.ndim) == -1
    assert e._L.davo_weights_missing(e._ctx) == 31
    left = 31
    for name in names:
        a = np.asarray(w[name], np.float32)
        a = a.copy() if a.shape == () else np.ascontiguousarray(a)
        shape = (ctypes.c_int64 * a.ndim)(*a.shape)
        e._check(e._L.davo_load_weight(e._ctx, name.encode(), a.ctypes.data_as(fp), shape, a.ndim))
        left -= 1
        assert e._L.davo_weights_missing(e._ctx) == left, name
    assert left == 0
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
    for b in bufs:
        b.free()
    # loaded by hand above: the context computes what an engine loaded through Engine.load_weights computes
    e.set_precision("f32")
    got = e.forward(img, flow, seg, depth=depth)
    e2 = _engine(cfg, H, W, B, w, "f32")
    assert _same_bits(e2.forward(img, flow, seg, depth=depth), got)
    e2.close()
    e.close()
    # att_table_far exists for this source alone
    f = _flagship_engine(cfg, H, W, B, w, "se_flow_near", "f32")
    f.forward(img, flow, seg)
    f.debug_read("att_table", TAB(B))
    with pytest.raises(ValueError, match="att_table_far"):
        f.debug_read("att_table_far", TAB(B))
    assert f.forward(img, flow, seg).shape == (B, 2, 6)          # the context stays usable
    f.close()


# ---- one pair -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_pair_reads_nothing_of_the_other_source_frames_depth(precision):
    cfg = parse_version(FULL)
    B, H, W = 2, 36, 100
    w = synth.make_weights(cfg)
    img, flow, seg, depth = _inputs(B, H, W, w)
    e = _engine(cfg, H, W, B, w, precision)
    both = e.forward(img, flow, seg, depth=depth)
    bufs = [e.alloc(a.nbytes).upload(a) for a in (img, flow, seg)]
    d_depth, d_pose = e.alloc(depth.nbytes), e.alloc(B * 2 * 6 * 4)
    for pairs, row, plane in (("src1", 1, 0), ("src0", 0, 2)):
        hidden = depth.copy()
        hidden[:, plane] = np.nan                               # the unselected source frame's plane
        e.set_pairs(pairs)
        d_depth.upload(hidden)
        e.forward_device(B, bufs[0], bufs[1], bufs[2], d_pose, depth=d_depth)
        e.synchronize()
        got = d_pose.download((B, 2, 6))
        assert _same_bits(got[:, row], both[:, row]), pairs
        assert np.array_equal(_bits(got[:, 1 - row]), np.zeros((B, 6), np.uint32)), pairs       # +0.0
        assert _same_bits(e.forward(img, flow, seg, depth=hidden), got), pairs                   # the host path stages the same
    e.set_pairs("both")
    assert _same_bits(e.forward(img, flow, seg, depth=depth), both)
    for b in bufs + [d_depth, d_pose]:
        b.free()
    e.close()


# ---- range recovery -------------------------------------------------------------------------------------------------------
def _rescaled(weights, shift):
    """tests/test_depth_source_gpu.py's recipe: the same network with cnv3's activations 2^shift larger (ReLU is
    homogeneous): trips the f16x3 range guard"""
    w = dict(weights)
    s = np.float32(2.0 ** shift)
    w["pose_exp_net/cnv3/weights"] = weights["pose_exp_net/cnv3/weights"] * s
    w["pose_exp_net/cnv3/biases"] = weights["pose_exp_net/cnv3/biases"] * s
    w["pose_exp_net/cnv4/weights"] = weights["pose_exp_net/cnv4/weights"] / s
    return w


def test_recovery_reissues_a_batch_on_its_own_depth(c_oracle):
    """Batch A is submitted with hold = 0, its depth array overwritten at once with another field and handed to batch B: A is
    re-issued at its verdict from the context's copy of its inputs - the depth planes among them.  The same through
    davo_forward_device_depth, where the upload of the other field is ordered behind the batch on the context's stream."""
    cfg = parse_version(FULL)
    B, H, W = 2, 64, 96
    w = synth.make_weights(cfg)
    A = _inputs(B, H, W, w, first_window=0)
    Bt = _inputs(B, H, W, w, first_window=7)
    depth_b = np.ascontiguousarray(A[3][:, ::-1, ::-1, ::-1])          # the planes exchanged and turned: same values, other places
    _assert_both_sides(depth_b, w[R.THRESHOLD])
    conv = c_oracle.conv2d_same
    want_a = R.forward(cfg, *A, w, conv=conv)
    wrong_a = R.forward(cfg, *A[:3], depth_b, w, conv=conv)
    want_b = R.forward(cfg, *Bt[:3], depth_b, w, conv=conv)
    bar = max(ABS_TOL, REL_TOL * np.abs(want_a).max())
    assert np.abs(wrong_a - want_a).max() > 10 * bar, (np.abs(wrong_a - want_a).max(), bar)       # before any GPU result
    e = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    depth_buf = A[3].copy()
    out_a, out_b = np.full((B, 2, 6), np.nan, np.float32), np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*A[:3], out_a, hold=0, depth=depth_buf)
    depth_buf[...] = depth_b
    e.submit(*Bt[:3], out_b, hold=0, depth=depth_buf)
    e.wait(0)
    assert e.range_stats()["reissued"] >= 1, e.range_stats()
    assert_pose_close(out_a, want_a, "batch A, re-issued")
    assert_pose_close(out_b, want_b, "batch B")
    e.close()
    e2 = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    d = [e2.alloc(a.nbytes).upload(a) for a in A] + [e2.alloc(B * 2 * 6 * 4)]
    e2.forward_device(B, d[0], d[1], d[2], d[4], depth=d[3])
    d[3].upload(depth_b)                                        # ordered behind the batch on the context's stream
    e2.synchronize()
    assert e2.range_stats()["reissued"] >= 1
    assert_pose_close(d[4].download((B, 2, 6)), want_a, "davo_forward_device_depth, re-issued")
    for b in d:
        b.free()
    e2.close()


# ---- export ---------------------------------------------------------------------------------------------------------------
def _select(seg_plane, depth_plane, near_row, far_row, thr):
    """[B,H,W] float32: the numpy select of two debug-read table rows [B,19]"""
    lab = seg_plane[..., 0]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(lab) & (lab > -1.0) & (lab < 19.0)
        near = depth_plane[..., 0] < np.float32(thr)
    idx = np.where(ok, lab, 0.0).astype(np.int64)
    B = lab.shape[0]
    pick = lambda row: np.take_along_axis(row, idx.reshape(B, -1), axis=1).reshape(lab.shape)       # noqa: E731
    return np.where(ok, np.where(near, pick(near_row), pick(far_row)), np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("masking", MASKINGS)
def test_feature_and_heat_export(masking, precision):
    cfg = parse_version(_version(masking))
    B, H, W = 2, 36, 100
    w = synth.make_weights(cfg)
    img, flow, seg, depth = _inputs(B, H, W, w)
    e = _engine(cfg, H, W, B, w, precision)
    before = e.forward(img, flow, seg, depth=depth)
    e.set_feature_export(True)
    e.set_heat_export(True)
    maps = ("attention", "masked_image", "image", "feat_rot", "feat_trans")
    r = e.forward_features(img, flow, seg, depth=depth, want=maps + Engine.HEAT_OUTPUTS)
    assert set(r) == {"pose"} | set(maps) | set(Engine.HEAT_OUTPUTS)
    assert _same_bits(r["pose"], before)
    near_t, far_t = e.debug_read("att_table", TAB(B)), e.debug_read("att_table_far", TAB(B))
    packed = e.debug_read("packed", (2 * B, H, W, 8))
    thr = np.float32(w[R.THRESHOLD])
    assert np.array_equal(r["attention"][0], np.ones((B, H, W), np.float32))            # the target's map is ones
    for frame, plane in ((1, 0), (2, 2)):
        want = _select(seg[:, plane], depth[:, plane], near_t[:, frame], far_t[:, frame], thr)
        assert _same_bits(r["attention"][frame], want), frame
        assert len(np.unique(r["attention"][frame])) > NUM_SEG_CLASSES + 1               # more values than one table holds: both were used
    unit = (img.astype(np.float32) * np.float32(1.0 / 255.0)) * np.float32(2.0) - np.float32(1.0)
    for frame, slot in ((0, 1), (1, 0), (2, 2)):
        assert _same_bits(r["image"][frame], unit[:, :, slot * W:(slot + 1) * W]), frame
    if precision == "f32":                                     # the packed tensor holds mask_pack's own float32 values
        pk = packed.reshape(B, 2, H, W, 8)
        assert _same_bits(r["masked_image"][0], pk[:, 0, ..., 0:3]) and _same_bits(r["masked_image"][0], pk[:, 1, ..., 0:3])
        assert _same_bits(r["masked_image"][1], pk[:, 0, ..., 3:6]) and _same_bits(r["masked_image"][2], pk[:, 1, ..., 3:6])
    want_masked = r["image"] * r["attention"][..., None] if cfg.mask_rgb else r["image"]
    assert _same_bits(r["masked_image"], want_masked)
    for feat, plane, top in (("feat_rot", "heat_rot", "max_rot"), ("feat_trans", "heat_trans", "max_trans")):
        full = r[feat]                                         # tests/test_heat_export_gpu.py's rule for the same call's full maps
        bar = HR.BAR_REL * HR.corner_sum_max(full[:, ::4, ::4])
        err = np.abs(r[plane].astype(np.float64) - full.sum(-1, dtype=np.float64))
        assert err.shape == (B, H, W) and (err <= bar).all(), (plane, float((err / np.maximum(bar, 1e-300)).max()))
        assert _same_bits(r[top], full.max(axis=(1, 2, 3))), top
    # a non-NULL att_19 is refused, and the context stays usable
    for want in (("att_19",), ("att_19", "attention"), ("att_19", "max_rot")):
        with pytest.raises(ValueError, match="att_19"):
            e.forward_features(img, flow, seg, depth=depth, want=want)
    again = e.forward_features(img, flow, seg, depth=depth, want=("attention",))
    assert _same_bits(again["attention"], r["attention"]) and _same_bits(again["pose"], before)
    assert _same_bits(e.forward(img, flow, seg, depth=depth), before)
    e.close()


@pytest.mark.parametrize("features", ["full", "heat"])
def test_davo_inference_feature_mode(features):
    cfg = parse_version(FULL)
    B, H, W = 2, 36, 100
    w = synth.make_weights(cfg)
    inputs = _inputs(B, H, W, w)
    system = DAVO(version=FULL).enable_feature_mode(features)
    system.setup_inference(H, W, "davo", 3, B)
    system.load_weights(w)
    pose = system.inference(None, mode="pose", inputs=inputs)["pose"]
    r = system.inference(None, mode="feature", inputs=inputs)
    assert set(r) == {"pose", "masks", "features", "images", "seg_19"} and set(r["masks"]) == {"attention", "image", "att_19"}
    assert r["masks"]["att_19"] == [] and _same_bits(r["pose"], pose)
    assert [a.shape for a in r["masks"]["attention"]] == [(B, H, W, 1)] * 3 and [a.shape for a in r["masks"]["image"]] == [(B, H, W, 3)] * 3
    assert [a.shape for a in r["images"]] == [(B, H, W, 3)] * 3 and [a.shape for a in r["seg_19"]] == [(B, H, W, 19)] * 3
    e = system.engine
    near_t, far_t = e.debug_read("att_table", TAB(B)), e.debug_read("att_table_far", TAB(B))
    for frame, plane in ((1, 0), (2, 2)):
        want = _select(inputs[2][:, plane], inputs[3][:, plane], near_t[:, frame], far_t[:, frame], w[R.THRESHOLD])
        assert _same_bits(r["masks"]["attention"][frame][..., 0], want), frame
        assert _same_bits(r["masks"]["image"][frame], r["images"][frame] * r["masks"]["attention"][frame])
    assert set(r["features"]) == ({"rot", "trans"} if features == "full" else {"rot_sum", "trans_sum", "rot_avg", "trans_avg", "rot_max", "trans_max"})
    e.close()


# ---- resources ------------------------------------------------------------------------------------------------------------
def test_create_and_close_leaves_no_device_memory_behind_and_the_flagship_allocates_no_far_table():
    cfg = parse_version(FULL)
    B, H, W = 2, 64, 96
    w = synth.make_weights(cfg)
    inputs = _inputs(B, H, W, w)
    rw = _rescaled(w, 16)
    free = []
    for _ in range(4):
        e = _engine(cfg, H, W, B, rw, "f16x3")
        e.set_inflight(2)
        outs = [np.empty((B, 2, 6), np.float32) for _ in range(2)]
        for out in outs:
            e.submit(*inputs[:3], out, depth=inputs[3])
        e.wait()
        e.synchronize()
        assert e.range_stats()["reissued"] >= 1
        e.close()
        free.append(hip_free_bytes())
    assert free[3] == free[0], free
    # a flagship context allocates no far table: its free-memory delta is that of a second flagship context (and
    # davo_debug_read("att_table_far") finds none there: test_three_input_forms_weights_and_debug_reads_are_refused_where_they_must)
    fcfg = parse_version(FULL.replace(SUB, "-se_flow"))
    deltas = []
    keep = []
    for c in (fcfg, fcfg):
        a = hip_free_bytes()
        keep.append(Engine(c, H, W, B))
        deltas.append(a - hip_free_bytes())
    for e in keep:
        e.close()
    assert deltas[0] == deltas[1] and deltas[0] > 0, deltas
    assert hip_free_bytes() == free[0]


# ---- CLI ------------------------------------------------------------------------------------------------------------------
def test_cli_runs_the_variant_from_a_dump(tmp_path, c_oracle):
    """run_kitti_pose on a 13-frame synthetic dump with -monodepth2_depth.npy files and a TF bundle that holds the rank-0
    threshold: the trajectory the float64 restatement's poses stitch to, at tests/test_depth_source_gpu.py's CLI bar; then
    through --gpus 1 with the ranks' all-gather forced (the window-sharded driver's path in one process)."""
    from davo_amd import run_kitti_pose, sequence as S, loader as L, tf_checkpoint as T
    cfg = parse_version(FULL)
    H, W, NF = 64, 96, 13
    dump = str(tmp_path / "dump")
    L.write_synthetic_dump(dump, 9, NF, H, W, depth=True)
    load = S.kitti_window_loader(dump, 9, NF, H, W, depth=True)
    weights = synth.make_weights(cfg)
    windows = load(0, NF - 2)
    _assert_both_sides(windows[3], weights[R.THRESHOLD])
    ck = tmp_path / "ckpt"
    ck.mkdir()
    T.write_checkpoint(str(ck / "model-1"), weights)
    common = ["--concat_img_dir", dump, "--ckpt_file", str(ck), "--version", FULL, "--test_seq", "9", "--batch_size", "4",
              "--img_height", str(H), "--img_width", str(W)]
    run_kitti_pose.main(common + ["--output_dir", str(tmp_path)])
    got = S.read_kitti_poses(str(tmp_path / "09-pred_kitti_pose.txt"))
    infer = lambda img, flow, seg, depth: R.forward(cfg, img, flow, seg, depth, weights, conv=c_oracle.conv2d_same)   # noqa: E731
    want, poses = S.run_sequence(infer, load.__call__, NF, 4)
    assert got.shape == (NF, 4, 4) and np.abs(got - np.array(want)).max() <= ABS_TOL
    run_kitti_pose.main(common + ["--output_dir", str(tmp_path / "sharded"), "--gpus", "1", "--force_comm"])
    sharded = S.read_kitti_poses(str(tmp_path / "sharded" / "09-pred_kitti_pose.txt"))
    assert sharded.shape == (NF, 4, 4) and np.abs(sharded - np.array(want)).max() <= ABS_TOL
