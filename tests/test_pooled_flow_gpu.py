"""The pooled flow-attention variants (att_source 14..17: -se_gp2x2_flow_nobottle, -se_spp21_flow, -se_spp2_flow,
-se_spp864_flow) on the GPU, against the float64 restatement of tests/pooled_flow_ref.py.

Bars: `se_desc' per entry within 2^-20 x (sum of |t(flow)| over the cell) x inv_div - the export tests' form and constant
(tests/heat_export_ref.py: BAR_REL) - times pooled_flow_cases.DESC_BAR_FACTOR (1 everywhere but se_spp864_flow at 64x64: 1.13,
four times the float32 restatement's own error there; tests/test_pooled_flow.py shows the margins); att_table rows 1, 2 at
layer_check.check_table, row 0 ones to the bit; packed at layer_check.check_packed; every conv layer, the pose head and the
poses as tests/test_depthseg_attention_gpu.py::test_layer_by_layer walks them.  Everything else is an identity to the bit.
Every test asserts pooled_flow_ref.check_preconditions on its own inputs before it looks at a device result: the table tells
where in the frame the flow sits, so a kernel that pooled the wrong window, or the whole frame, cannot pass."""
import glob
import os

import numpy as np
import pytest

from davo_amd import DAVO, Engine, FLAGSHIP_VERSION, flow_from_f16, flow_to_f16, labels_to_u8, parse_version, synth, windows_from_frames
from davo_amd.pool import pool_plan
from davo_amd.version import NUM_SEG_CLASSES

import heat_export_ref as HR
import layer_check as LC
import pooled_flow_cases as K
import pooled_flow_ref as R
from helpers import assert_pose_close, hip_free_bytes

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "f32"]
TAB = lambda B: (B, 3, NUM_SEG_CLASSES)       # noqa: E731
assert HR.BAR_REL == 2.0 ** -20


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _engine(cfg, H, W, B, weights, precision="f16x3", **kw):
    e = Engine(cfg, H, W, B, **kw)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


def _forward(e, inputs):
    """one step, and the batch was not re-issued"""
    before = e.range_stats()
    got = e.forward(*inputs)
    after = e.range_stats()
    assert after["f32_batches"] == before["f32_batches"] and after["reissued"] == before["reissued"], (before, after, e.range_report())
    return got


def _desc_shape(cfg, B):
    return (B, 2, R.WIDTHS[cfg.att_source][0])


def _entry_case(src, precondition=True):
    H, W, B = K.ENTRY_SHAPE
    cfg, w = K.config((src, "-segmask_all", "-fc_tanh", "-abs_flow"))
    inputs = K.inputs(B, H, W)
    if precondition:
        R.check_preconditions(cfg, inputs[1], w, LC.TABLE_TOL)
    return cfg, w, inputs, H, W, B


# ---- layer by layer against float64 -------------------------------------------------------------------------------------
_CASES = {}


def _case(case, conv):
    """(cfg, weights, inputs, float64 descriptor, its bar, float64 tables, float64 packed, reference poses), shared by the two
    precisions; the preconditions are asserted here, before any device result"""
    if case not in _CASES:
        src, masking, act, transform, H, W, B = case
        cfg, w = K.config(case)
        inputs = K.inputs(B, H, W)
        R.check_preconditions(cfg, inputs[1], w, LC.TABLE_TOL, need_outside=K.has_outside(src, H, W))
        desc = R.descriptor(cfg, inputs[1])
        bar = R.descriptor_bar(cfg, inputs[1]) * K.desc_bar_factor(src, H, W)
        tab = R.tables_from_descriptor(cfg, desc, w)
        _CASES.clear()
        _CASES[case] = (cfg, w, inputs, desc, bar, tab, R.pack(cfg, *inputs, w), R.forward(cfg, *inputs, w, conv=conv))
    return _CASES[case]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", K.layer_cases(), ids=K.case_id)
def test_layer_by_layer(c_oracle, case, precision):
    """The descriptor, the table and the packed input against float64, then tests/test_depthseg_attention_gpu.py::
    test_layer_by_layer's walk: every conv layer against a float64 convolution of the GPU's own input to it (first and last
    pair image), the pose head and the poses."""
    H, W, B = case[4:]
    cfg, w, inputs, want_desc, desc_bar, want_tab, want_packed, want_pose = _case(case, c_oracle.conv2d_same)
    what = "%s %s" % (K.case_id(case), precision)
    e = _engine(cfg, H, W, B, w, precision)
    e.set_option("fuse_pose", 0)                               # cnv7 is stored: the last layer is checked like the others
    poses = _forward(e, inputs)
    assert np.array_equal(poses, _forward(e, inputs))
    NB = 2 * B
    desc = e.debug_read("se_desc", _desc_shape(cfg, B))
    err = np.abs(desc.astype(np.float64) - want_desc)
    worst = float((err / np.maximum(desc_bar, 1e-300)).max()) if (desc_bar > 0).any() else 0.0
    print("%s: se_desc max |err| / bar %.3g" % (what, worst))
    assert (err <= desc_bar).all(), (what, worst)
    assert np.array_equal(_bits(desc[desc_bar == 0]), np.zeros((desc_bar == 0).sum(), np.uint32))      # cells wholly in padding: +0.0
    got = e.debug_read("att_table", TAB(B))
    terr = LC.check_table(got, want_tab, [1, 2], what)
    print("%s: att_table max|err| %.3g (bar %.1g)" % (what, terr, LC.TABLE_TOL))
    assert np.array_equal(_bits(got[:, 0]), _bits(np.ones((B, NUM_SEG_CLASSES), np.float32)))           # the target's row is ones
    sh = LC.shapes(cfg, H, W)
    acts = {"packed": e.debug_read("packed", (NB,) + sh["packed"])}
    LC.check_packed(acts["packed"], want_packed.reshape(NB, H, W, 10)[..., LC.PACK8], what)
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
    for fold in (0, 1):                                        # "fold_tails" does not apply to these sources: the same launches, the same bits
        e.set_option("fold_tails", fold)
        e.forward(*inputs)
        assert _same(e.debug_read("se_desc", _desc_shape(cfg, B)), desc) and _same(e.debug_read("att_table", TAB(B)), got), fold
    e.close()


# ---- what lies outside every window is not read -----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", [s for s in K.SHAPES if s[:2] != (64, 64)])
@pytest.mark.parametrize("src", [s for s in K.SOURCES if s != "se_gp2x2_flow_nobottle"])
def test_unread_pixels_stay_unread(src, H, W, B):
    """NaN in every flow pixel outside all windows: the descriptor and the table keep their bits (a v1 network packs the raw
    flow, so its poses would not); a v0 network, whose only use of the flow is the squeeze, keeps its poses too.  Both flow
    formats."""
    cfg, w = K.config((src, "-segmask_all", "-fc_tanh", "-abs_flow"))
    img, flow, seg = K.inputs(B, H, W)
    figures = R.check_preconditions(cfg, flow, w, LC.TABLE_TOL, need_outside=True)
    dirty = K.nan_outside(flow, src)
    assert np.isnan(dirty[:, :2]).sum() == 2 * 2 * B * figures["outside"] and np.isnan(dirty).any()
    v0 = parse_version("v0-sharedNN-dilatedPoseNN-segmask" + R.SUBSTRING[src] + "-abs_flow-fc_tanh")
    assert v0.att_source == src and not v0.use_flow_info and v0.mask_rgb
    w0 = synth.make_weights(v0)
    for fmt in ("f32", "f16"):
        conv = (lambda a: a) if fmt == "f32" else flow_to_f16
        e = _engine(cfg, H, W, B, w, "f32", flow=fmt)
        e.forward(img, conv(flow), seg)
        clean = (e.debug_read("se_desc", _desc_shape(cfg, B)), e.debug_read("att_table", TAB(B)))
        e.forward(img, conv(dirty), seg)
        assert _same(e.debug_read("se_desc", _desc_shape(cfg, B)), clean[0]), fmt
        assert _same(e.debug_read("att_table", TAB(B)), clean[1]), fmt
        assert np.isfinite(clean[0]).all() and np.isfinite(clean[1]).all()
        e.close()
        e0 = _engine(v0, H, W, B, w0, "f16x3", flow=fmt)
        want = e0.forward(img, conv(flow), seg)
        assert np.isfinite(want).all() and _same(e0.forward(img, conv(dirty), seg), want), fmt
        e0.close()


# ---- spp [2] is gp2x2 on a square frame --------------------------------------------------------------------------------------
def test_spp2_is_gp2x2_at_64x64_to_the_bit():
    H, W, B = 64, 64, 2
    cfg2, w2 = K.config(("se_spp2_flow", "-segmask_all", "-fc_tanh", "-abs_flow"))
    cfgg, wg = K.config(("se_gp2x2_flow_nobottle", "-segmask_all", "-fc_tanh", "-abs_flow"))
    inputs = K.inputs(B, H, W)
    R.check_preconditions(cfg2, inputs[1], w2, LC.TABLE_TOL)
    R.check_preconditions(cfgg, inputs[1], wg, LC.TABLE_TOL)
    assert w2["pose_exp_net/se_flow/bottleneck_fc/kernel"].shape == (8, 8)
    descs = []
    for cfg, w in ((cfg2, w2), (cfgg, wg)):
        e = _engine(cfg, H, W, B, w, "f32")
        e.forward(*inputs)
        descs.append(e.debug_read("se_desc", (B, 2, 8)))
        e.close()
    assert _same(descs[0], descs[1]) and np.abs(descs[0]).min() > 0
    # and the table of spp2 is the restatement's on gp2x2's descriptor with spp2's [8,8] MLP
    want = R.tables_from_descriptor(cfg2, R.descriptor(cfgg, inputs[1]), w2)
    e = _engine(cfg2, H, W, B, w2, "f32")
    e.forward(*inputs)
    LC.check_table(e.debug_read("att_table", TAB(B)), want, [1, 2], "spp2 at 64x64")
    e.close()


# ---- entry points -----------------------------------------------------------------------------------------------------------
def _device_forward(e, B, img, flow, seg):
    bufs = [e.alloc(a.nbytes).upload(a) for a in (img, flow, seg)]
    d_pose = e.alloc(B * 12 * 4)
    try:
        e.forward_device(B, bufs[0], bufs[1], bufs[2], d_pose)
        e.synchronize()
        return d_pose.download((B, 2, 6))
    finally:
        for b in bufs + [d_pose]:
            b.free()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("src", K.ENTRY_SOURCES)
def test_entry_points_agree_to_the_bit(src, precision):
    """The window entry point, its sub-batches, the device and the streaming entry points: a float32-flow, float32-label engine
    on the rounded flow against a binary16-flow, byte-label engine on the halves, to the bit."""
    cfg, w, (img, flow, seg), H, W, B = _entry_case(src)
    h = flow_to_f16(flow)
    wide = flow_from_f16(h)
    R.check_preconditions(cfg, wide, w, LC.TABLE_TOL)
    seg8 = labels_to_u8(seg)
    e32 = _engine(cfg, H, W, B, w, precision)
    e16 = _engine(cfg, H, W, B, w, precision, labels="u8", flow="f16")
    want = e32.forward(img, wide, seg)
    tensors = (e32.debug_read("se_desc", _desc_shape(cfg, B)), e32.debug_read("att_table", TAB(B)), e32.debug_read("packed", (2 * B, H, W, 8)))
    assert np.isfinite(want).all() and np.abs(want).max() > 0
    assert _same(e16.forward(img, h, seg8), want)
    for got, ref in zip((e16.debug_read("se_desc", _desc_shape(cfg, B)), e16.debug_read("att_table", TAB(B)), e16.debug_read("packed", (2 * B, H, W, 8))), tensors):
        assert _same(got, ref)
    assert _same(_device_forward(e32, B, img, wide, seg), want) and _same(_device_forward(e16, B, img, h, seg8), want)
    # sub-batches of one window: window b is to the bit what the other entry points return on that window alone; the descriptor
    # and the table do not depend on the batch at all
    for e, f, s in ((e32, wide, seg), (e16, h, seg8)):
        e.set_option("host_chunk", 1)
        chunked = e.forward(img, f, s)
        e.set_option("host_chunk", 8)
        assert_pose_close(chunked, want, "host_chunk 1 against one step")
        for b in range(B):
            one = tuple(np.ascontiguousarray(a[b:b + 1]) for a in (img, f, s))
            assert _same(e.forward(*one), chunked[b:b + 1]), b
            assert _same(e.debug_read("se_desc", _desc_shape(cfg, 1)), tensors[0][b:b + 1]), b
            assert _same(e.debug_read("att_table", TAB(1)), tensors[1][b:b + 1]), b
            assert _same(_device_forward(e, 1, *one), chunked[b:b + 1]), b
            out1 = np.full((1, 2, 6), np.nan, np.float32)
            e.submit(*one, out1)
            e.wait()
            assert _same(out1, chunked[b:b + 1]), b
    # streaming: two in flight, the caller's arrays recycled at once (hold = 0)
    for e, f, s in ((e32, wide, seg), (e16, h, seg8)):
        e.set_inflight(2)
        work = [a.copy() for a in (img, f, s)]
        outs = [np.full((B, 2, 6), np.nan, np.float32) for _ in range(3)]
        for out in outs:
            for dst, src_a in zip(work, (img, f, s)):
                dst[...] = src_a
            e.submit(*work, out, hold=0)
            work[0][...] = 77
            work[1][...] = 1000.0
            work[2][...] = 3
        e.wait()
        e.synchronize()
        e.set_inflight(1)
        for out in outs:
            assert _same(out, want)
    shifts = e32.calibrate(img, wide, seg)
    assert set(shifts) == set(e32.LAYERS)
    e32.close()
    e16.close()


@pytest.mark.parametrize("src", K.ENTRY_SOURCES)
def test_the_frame_entry_points(src):
    """The three `_frames' forms against the window form on the windows the caller would have built; both formats."""
    H, W, N = 36, 100, 4
    cfg, w = K.config((src, "-segmask_all", "-fc_tanh", "-abs_flow"))
    frames, _, fseg = synth.make_frames(N + 2, H, W)
    flow2 = np.ascontiguousarray(R.make_flow(N, H, W, first_window=11)[:, :2])
    h2 = flow_to_f16(flow2)
    fr32 = (frames, flow_from_f16(h2), fseg)
    fr16 = (frames, h2, labels_to_u8(fseg))
    win32 = windows_from_frames(*fr32)
    R.check_preconditions(cfg, win32[1], w, LC.TABLE_TOL)
    e32 = _engine(cfg, H, W, N, w)
    e16 = _engine(cfg, H, W, N, w, labels="u8", flow="f16")
    want = e32.forward(*win32)
    desc = e32.debug_read("se_desc", _desc_shape(cfg, N))
    assert np.isfinite(want).all()
    for e, fr in ((e32, fr32), (e16, fr16)):
        assert _same(e.forward_frames(*fr), want)
        assert _same(e.debug_read("se_desc", _desc_shape(cfg, N)), desc)
        out = np.full((N, 2, 6), np.nan, np.float32)
        e.submit_frames(fr[0], fr[1], fr[2], out, hold=1)
        e.wait(0)
        e.synchronize()
        assert _same(out, want)
        bufs = [e.alloc(a.nbytes).upload(a) for a in fr]
        d_pose = e.alloc(N * 12 * 4)
        e.forward_device_frames(N, bufs[0], bufs[1], bufs[2], d_pose)
        e.synchronize()
        assert _same(d_pose.download((N, 2, 6)), want)
        for b in bufs + [d_pose]:
            b.free()
        # one pair from frames: the rows of the selected pair, the other row +0.0
        e.set_pairs("src1")
        one = e.forward_frames(*fr)
        assert _same(one, e.forward(*windows_from_frames(*fr))) and np.array_equal(_bits(one[:, 0]), np.zeros((N, 6), np.uint32))
        e.set_pairs("both")
    e32.close()
    e16.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("src", K.ENTRY_SOURCES)
def test_one_pair_reads_nothing_of_the_other_source_plane(src, precision):
    cfg, w, (img, flow, seg), H, W, B = _entry_case(src)
    e = _engine(cfg, H, W, B, w, precision)
    both = e.forward(img, flow, seg)
    desc, tab = e.debug_read("se_desc", _desc_shape(cfg, B)), e.debug_read("att_table", TAB(B))
    bufs = [e.alloc(a.nbytes).upload(a) for a in (img, flow, seg)]
    d_pose = e.alloc(B * 2 * 6 * 4)
    for pairs, row in (("src1", 1), ("src0", 0)):
        hidden = flow.copy()
        hidden[:, 1 - row] = np.nan                            # the unselected source frame's flow plane
        hidden[:, 2:] = np.nan                                 # planes 2, 3 are never read
        e.set_pairs(pairs)
        clean = e.forward(img, flow, seg)
        assert np.isfinite(clean[:, row]).all() and np.array_equal(_bits(clean[:, 1 - row]), np.zeros((B, 6), np.uint32)), pairs      # +0.0
        assert_pose_close(clean[:, row], both[:, row], pairs)
        assert _same(e.forward(img, hidden, seg), clean), pairs
        # the selected source's descriptor and table are the both-pairs batch's to the bit: the squeeze does not depend on the selection
        assert _same(e.debug_read("se_desc", _desc_shape(cfg, B))[:, row], desc[:, row]), pairs
        assert _same(e.debug_read("att_table", TAB(B))[:, 1 + row], tab[:, 1 + row]), pairs
        bufs[1].upload(hidden)
        e.forward_device(B, bufs[0], bufs[1], bufs[2], d_pose)
        e.synchronize()
        assert _same(d_pose.download((B, 2, 6)), clean), pairs
    e.set_pairs("both")
    assert _same(e.forward(img, flow, seg), both)
    for b in bufs + [d_pose]:
        b.free()
    e.close()


# ---- repeatability and memory -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("src", K.SOURCES)
def test_fifty_repeats_are_bit_identical(src, precision):
    cfg, w, inputs, H, W, B = _entry_case(src)
    e = _engine(cfg, H, W, B, w, precision)
    first = _forward(e, inputs)
    desc, tab = e.debug_read("se_desc", _desc_shape(cfg, B)), e.debug_read("att_table", TAB(B))
    for _ in range(50):
        assert _same(_forward(e, inputs), first)
    assert _same(e.debug_read("se_desc", _desc_shape(cfg, B)), desc) and _same(e.debug_read("att_table", TAB(B)), tab)
    perm = [2, 1, 0]                                           # swapped windows swap their results
    swapped = _forward(e, tuple(np.ascontiguousarray(a[perm]) for a in inputs))
    assert _same(swapped, first[perm]) and not _same(first[0], first[2])
    assert _same(e.debug_read("se_desc", _desc_shape(cfg, B)), desc[perm])
    e.close()


def _rescaled(weights, shift):
    """tests/test_depth_source_gpu.py's recipe: the same network with cnv3's activations 2^shift larger (ReLU is homogeneous):
    trips the f16x3 range guard"""
    w = dict(weights)
    s = np.float32(2.0 ** shift)
    w["pose_exp_net/cnv3/weights"] = weights["pose_exp_net/cnv3/weights"] * s
    w["pose_exp_net/cnv3/biases"] = weights["pose_exp_net/cnv3/biases"] * s
    w["pose_exp_net/cnv4/weights"] = weights["pose_exp_net/cnv4/weights"] / s
    return w


def test_create_and_close_leaves_no_device_memory_behind():
    cfg, w, inputs, H, W, B = _entry_case("se_spp864_flow")
    rw = _rescaled(w, 16)
    free = []
    for _ in range(4):
        e = _engine(cfg, H, W, B, rw)
        e.set_inflight(2)
        outs = [np.empty((B, 2, 6), np.float32) for _ in range(2)]
        for out in outs:
            e.submit(*inputs, out)
        e.wait()
        e.synchronize()
        assert e.range_stats()["reissued"] >= 1
        e.debug_read("se_desc", _desc_shape(cfg, B))
        e.close()
        free.append(hip_free_bytes())
    assert free[3] == free[0], free
    # `se_desc' exists for these sources alone, and a flagship context allocates none
    f = _engine(parse_version(FLAGSHIP_VERSION), H, W, B, synth.make_weights(FLAGSHIP_VERSION))
    f.forward(*inputs)
    with pytest.raises(ValueError, match="se_desc"):
        f.debug_read("se_desc", (B, 2, 2))
    assert f.forward(*inputs).shape == (B, 2, 6)
    f.close()
    assert hip_free_bytes() == free[0]


# ---- range recovery ---------------------------------------------------------------------------------------------------------
def test_recovery_reissues_a_batch_with_final_poses(c_oracle):
    """A checkpoint that trips the f16x3 guard: batch A is submitted with hold = 0 and its flow array overwritten at once with
    another batch's; A is re-issued at its verdict from the context's copy of its inputs and delivers its own poses."""
    cfg, w, A, H, W, B = _entry_case("se_spp864_flow")
    Bt = K.inputs(B, H, W, 7)
    R.check_preconditions(cfg, Bt[1], w, LC.TABLE_TOL)
    conv = c_oracle.conv2d_same
    want_a, want_b = R.forward(cfg, *A, w, conv=conv), R.forward(cfg, *Bt, w, conv=conv)
    e = _engine(cfg, H, W, B, _rescaled(w, 16))
    work = [a.copy() for a in A]
    out_a, out_b = np.full((B, 2, 6), np.nan, np.float32), np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*work, out_a, hold=0)
    for dst, src in zip(work, Bt):
        dst[...] = src
    e.submit(*work, out_b, hold=0)
    e.wait(0)
    assert e.range_stats()["reissued"] >= 1, e.range_stats()
    assert_pose_close(out_a, want_a, "batch A, re-issued")
    assert_pose_close(out_b, want_b, "batch B")
    LC.check_table(e.debug_read("att_table", TAB(B)), R.class_tables(cfg, Bt[1], w), [1, 2], "after the re-issue")
    e.close()


# ---- exports ----------------------------------------------------------------------------------------------------------------
def _lookup(seg_plane, rows):
    """[B,H,W] float32: rows [B,19] looked up through a label plane [B,H,W,1]; 0 outside the classes"""
    lab = seg_plane[..., 0]
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(lab) & (lab > -1.0) & (lab < 19.0)
    idx = np.where(ok, lab, 0.0).astype(np.int64)
    B = lab.shape[0]
    pick = np.take_along_axis(rows, idx.reshape(B, -1), axis=1).reshape(lab.shape)
    return np.where(ok, pick, np.float32(0.0)).astype(np.float32)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("src", K.ENTRY_SOURCES)
def test_feature_and_heat_export(src, precision):
    cfg, w, (img, flow, seg), H, W, B = _entry_case(src)
    e = _engine(cfg, H, W, B, w, precision)
    before = e.forward(img, flow, seg)
    e.set_feature_export(True)
    e.set_heat_export(True)
    maps = ("att_19", "attention", "masked_image", "image", "feat_rot", "feat_trans")
    r = e.forward_features(img, flow, seg, want=maps + Engine.HEAT_OUTPUTS)
    assert set(r) == {"pose"} | set(maps) | set(Engine.HEAT_OUTPUTS) and _same(r["pose"], before)
    tab = e.debug_read("att_table", TAB(B))
    LC.check_table(tab, R.class_tables(cfg, flow, w), [1, 2], "export")
    assert _same(r["att_19"], np.ascontiguousarray(tab.transpose(1, 0, 2)))
    assert np.array_equal(r["attention"][0], np.ones((B, H, W), np.float32))            # the target's map is ones
    for frame, plane in ((1, 0), (2, 2)):
        assert _same(r["attention"][frame], _lookup(seg[:, plane], tab[:, frame])), frame
    unit = (img.astype(np.float32) * np.float32(1.0 / 255.0)) * np.float32(2.0) - np.float32(1.0)
    for frame, slot in ((0, 1), (1, 0), (2, 2)):
        assert _same(r["image"][frame], unit[:, :, slot * W:(slot + 1) * W]), frame
    assert _same(r["masked_image"], r["image"] * r["attention"][..., None])
    for feat, plane, top in (("feat_rot", "heat_rot", "max_rot"), ("feat_trans", "heat_trans", "max_trans")):
        full = r[feat]                                         # tests/test_heat_export_gpu.py's rule for the same call's full maps
        bar = HR.BAR_REL * HR.corner_sum_max(full[:, ::4, ::4])
        err = np.abs(r[plane].astype(np.float64) - full.sum(-1, dtype=np.float64))
        assert err.shape == (B, H, W) and (err <= bar).all(), plane
        assert _same(r[top], full.max(axis=(1, 2, 3))), top
    assert _same(e.forward(img, flow, seg), before)
    e.close()


@pytest.mark.parametrize("features", ["full", "heat"])
def test_davo_inference_feature_mode(features):
    src = "se_spp864_flow"
    cfg, w, inputs, H, W, B = _entry_case(src)
    system = DAVO(version=cfg.version).enable_feature_mode(features)
    system.setup_inference(H, W, "davo", 3, B)
    system.load_weights(w)
    pose = system.inference(None, mode="pose", inputs=inputs)["pose"]
    r = system.inference(None, mode="feature", inputs=inputs)
    assert set(r) == {"pose", "masks", "features", "images", "seg_19"} and set(r["masks"]) == {"attention", "image", "att_19"}
    assert _same(r["pose"], pose)
    assert [a.shape for a in r["masks"]["attention"]] == [(B, H, W, 1)] * 3 and [a.shape for a in r["masks"]["image"]] == [(B, H, W, 3)] * 3
    e = system.engine
    tab = e.debug_read("att_table", TAB(B))
    LC.check_table(tab, R.class_tables(cfg, inputs[1], w), [1, 2], "DAVO")
    for frame, plane in ((1, 0), (2, 2)):
        assert _same(r["masks"]["attention"][frame][..., 0], _lookup(inputs[2][:, plane], tab[:, frame])), frame
        assert _same(np.asarray(r["masks"]["att_19"][frame]).reshape(B, NUM_SEG_CLASSES), tab[:, frame]), frame
    assert set(r["features"]) == ({"rot", "trans"} if features == "full" else {"rot_sum", "trans_sum", "rot_avg", "trans_avg", "rot_max", "trans_max"})
    e.close()


# ---- CLI --------------------------------------------------------------------------------------------------------------------
def test_cli_runs_the_variant_from_a_dump(tmp_path, c_oracle):
    """run_kitti_pose on a 9-frame synthetic dump whose flow files hold pooled_flow_ref.make_flow's fields, with a TF bundle
    that holds the [232,8] bottleneck: the trajectory the float64 restatement's poses stitch to."""
    from davo_amd import run_kitti_pose, sequence as S, loader as L, tf_checkpoint as T
    cfg, weights = K.config(("se_spp864_flow", "-segmask_all", "-fc_tanh", "-abs_flow"))
    H, W, NF = 64, 96, 9
    dump = str(tmp_path / "dump")
    L.write_synthetic_dump(dump, 9, NF, H, W)
    files = sorted(glob.glob(os.path.join(dump, "*", "*-flownet2.npy")))
    assert len(files) >= NF - 2
    for k, path in enumerate(files):
        assert np.load(path).shape == (4, H, W, 2)
        np.save(path, R.make_flow(1, H, W, first_window=k)[0])
    load = S.kitti_window_loader(dump, 9, NF, H, W)
    windows = load(0, NF - 2)
    R.check_preconditions(cfg, windows[1], weights, LC.TABLE_TOL)
    ck = tmp_path / "ckpt"
    ck.mkdir()
    T.write_checkpoint(str(ck / "model-1"), weights)
    run_kitti_pose.main(["--concat_img_dir", dump, "--ckpt_file", str(ck), "--output_dir", str(tmp_path), "--version", cfg.version,
                         "--test_seq", "9", "--batch_size", "4", "--img_height", str(H), "--img_width", str(W)])
    got = S.read_kitti_poses(str(tmp_path / "09-pred_kitti_pose.txt"))
    infer = lambda img, flow, seg: R.forward(cfg, img, flow, seg, weights, conv=c_oracle.conv2d_same)   # noqa: E731
    want, _ = S.run_sequence(infer, load.__call__, NF, 4)
    assert got.shape == (NF, 4, 4) and np.abs(got - np.array(want)).max() < 2e-4


# ---- the flagship is untouched ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_flagship_is_untouched(precision):
    """The flagship's launches are the ones it had (no pooled launch, its own squeeze), its pool plan is empty, and its poses
    are bit-equal before and after a pooled context has been created, run and closed beside it on the same inputs."""
    cfg = parse_version(FLAGSHIP_VERSION)
    assert pool_plan(128, 416, cfg.att_source)[0].shape == (0, 4) and pool_plan(36, 100, cfg.as_c_ints()[5])[0].shape == (0, 4)
    H, W, B = K.ENTRY_SHAPE
    inputs = K.inputs(B, H, W)
    w = synth.make_weights(cfg)
    f = _engine(cfg, H, W, B, w, precision)
    before = f.forward(*inputs)
    tab = f.debug_read("att_table", TAB(B))
    pc, pw, _, _, _, _ = _entry_case("se_spp864_flow")
    p = _engine(pc, H, W, B, pw, precision)
    p.profile(1)
    p.forward(*inputs)
    names = {k for k, (n, _) in p.profile_entries().items() if n > 0}
    assert {"se_pool_squeeze", "se_pool_excite", "mask_pack"} <= names or {"se_pool_squeeze", "se_pool_excite"} <= names, names
    assert "se_squeeze_partial" not in names and "se_excite" not in names, names
    p.close()
    f.profile(1)
    f.profile_reset()
    after = f.forward(*inputs)
    names = {k for k, (n, _) in f.profile_entries().items() if n > 0}
    f.profile(0)
    assert "se_squeeze_partial" in names and not any(n.startswith("se_pool") for n in names), names
    assert _same(after, before) and _same(f.debug_read("att_table", TAB(B)), tab)
    LC.check_table(tab, LC.ref_tables(cfg, *inputs, w)[0], [1, 2], "flagship")
    f.close()
