"""Mirrored inputs on the GPU (include/davo_hip.h: davo_set_flip; csrc/window_mirror.h).

The whole contract is one sentence: an engine with flip on, given X, computes bit for bit what the same engine with flip off
computes on flip_windows(X).  So every comparison here is between a flip-on engine on X and a flip-off engine - same weights,
formats, options and call sequence - on davo_amd.flip_windows(X) (flip_frames for the frame layout), to the bit.  No tolerance
appears in this file.  The flip-off engine's own comparison against float64 exists already (tests/test_plan_layers_gpu.py and
the variants' own files).

Shapes, the smallest that reach every row form of the mirror kernel: 36x100 (W % 16 == 4: 25 four-pixel groups per row, an odd
number, so a middle group that is its own partner; strip rows move as dwords; u8 label rows of 100 bytes), 32x24 (W % 16 == 8,
six groups), 64x64 (the 16-byte units everywhere).  B = 1 and 3, and "host_chunk" 1 under B = 3 so that one call is three
sub-batches.  The label maps are drawn per pixel (synth's come in 8x8 blocks, which would hide a group that is not reversed
inside itself)."""
import ctypes

import numpy as np
import pytest

from davo_amd import DAVO, Engine, FLAGSHIP_VERSION, flip_frames, flip_windows, parse_version, synth, windows_from_frames

from helpers import hip_free_bytes

pytestmark = pytest.mark.gpu

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"
SEGFLOW = BASE + "-segmask_all-se_SegFlow_to_seg-abs_flow-fc_tanh"            # a class-table source that attends the target
DEPTH_SOURCE = BASE + "-segmask_all-se_depth_to_seg-fc_tanh"
DEPTH_SPLIT = BASE + "-segmask_all-se_flow_on_depthseg_seplayers-abs_flow-fc_tanh"
TRIPLET = "v1-decay100k-dilatedPoseNN-cnv6_128-segmask_all-se_flow-abs_flow-fc_tanh"
SHAPES = [(36, 100), (32, 24), (64, 64)]
FORMATS = [("f32", "f32"), ("u8", "f32"), ("f32", "f16"), ("u8", "f16")]      # (labels, flow)
PRECISIONS = ("f16x3", "f32")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _pixel_labels(shape, seed, labels):
    """label maps with a class of its own draw in every pixel, 3 % ignore (255)"""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, 19, shape).astype(np.float32)
    ids[rng.random(shape) < 0.03] = 255.0
    return ids.astype(np.uint8) if labels == "u8" else ids


def _inputs(cfg, B, H, W, labels="f32", flow="f32", first_window=3):
    img, fl, _ = synth.make_inputs(B, H, W, first_window=first_window, flow=flow)
    X = (img, fl, _pixel_labels((B, 3, H, W, 1), 11 * B + H + first_window, labels))
    return X + ((synth.make_depth(B, H, W, first_window=first_window),) if cfg.needs_depth else ())


def _frames(cfg, N, H, W, labels="f32", flow="f32"):
    fr = synth.make_frames(N + 2, H, W, depth=cfg.needs_depth, flow=flow)
    return (fr[0], fr[1], _pixel_labels((N + 2, H, W, 1), 7 * N + W, labels)) + tuple(fr[3:])


def _pair(cfg, H, W, max_batch, labels="f32", flow="f32", weights=None, inflight=2):
    """-> (the flip-off engine, the flip-on engine), same weights and formats"""
    weights = synth.make_weights(cfg) if weights is None else weights
    pair = (Engine(cfg, H, W, max_batch, labels=labels, flow=flow), Engine(cfg, H, W, max_batch, labels=labels, flow=flow))
    for e in pair:
        e.load_weights(weights)
        e.set_inflight(inflight)
    assert pair[1].flip is False
    pair[1].set_flip(True)
    assert pair[0].flip is False and pair[1].flip is True
    return pair


def _tensors(e, cfg, B, H, W):
    """davo_debug_read of the last forward: packed, the class tables, cnv1"""
    trip = cfg.posenn == "triplet"
    nimg = B if trip else 2 * B
    out = {"packed": e.debug_read("packed", (nimg, H, W, 16 if trip else 8)),
           "cnv1": e.debug_read("cnv1", (nimg, (H + 1) // 2, (W + 1) // 2, 16))}
    if cfg.att_source != "ones":
        out["att_table"] = e.debug_read("att_table", (B, 3, 19))
    if cfg.att_source == "se_flow_depthseg_sep":
        out["att_table_far"] = e.debug_read("att_table_far", (B, 3, 19))
    return out


def _split(X):
    return tuple(X[:3]), (X[3] if len(X) == 4 else None)


def _device_forward(e, X, timed=False):
    """davo_forward_device[_depth] on uploads of X -> (poses, the caller's device buffers read back afterwards)"""
    B = X[0].shape[0]
    bufs = [e.alloc(a.nbytes).upload(a) for a in X]
    d_pose = e.alloc(B * 12 * 4)
    try:
        e.forward_device(B, bufs[0], bufs[1], bufs[2], d_pose, timed=timed, depth=bufs[3] if len(X) == 4 else None)
        e.synchronize()
        return d_pose.download((B, 2, 6)), [b.download(a.shape, a.dtype) for b, a in zip(bufs, X)]
    finally:
        for b in bufs + [d_pose]:
            b.free()


def _device_frames(e, fr):
    N = fr[1].shape[0]
    bufs = [e.alloc(a.nbytes).upload(a) for a in fr]
    d_pose = e.alloc(N * 12 * 4)
    try:
        e.forward_device_frames(N, bufs[0], bufs[1], bufs[2], d_pose, depth=bufs[3] if len(fr) == 4 else None)
        e.synchronize()
        return d_pose.download((N, 2, 6)), [b.download(a.shape, a.dtype) for b, a in zip(bufs, fr)]
    finally:
        for b in bufs + [d_pose]:
            b.free()


def _streamed(e, X, n=3, frames=False):
    """n submits (hold 0, two slots) from scratch arrays overwritten as soon as each submit returns"""
    inputs, depth = _split(X)
    scratch = [np.empty_like(a) for a in X]
    outs = [np.full((X[1].shape[0], 2, 6), np.nan, np.float32) for _ in range(n)]
    for out in outs:
        for dst, src in zip(scratch, X):
            dst[...] = src
        (e.submit_frames if frames else e.submit)(scratch[0], scratch[1], scratch[2], out, hold=0, depth=scratch[3] if depth is not None else None)
        scratch[0][...] = 77
        scratch[1][...] = 1000.0
        scratch[2][...] = 3
        if depth is not None:
            scratch[3][...] = 0.25
    e.wait(0)
    e.synchronize()
    return outs


def _check_every_entry_point(cfg, off, on, B, H, W, labels, flow, what, frames=True):
    X = _inputs(cfg, B, H, W, labels, flow)
    FX = flip_windows(*X)
    assert not _same(FX[0], X[0]) and not _same(FX[1], X[1]) and not _same(FX[2], X[2])
    for precision in PRECISIONS:
        for e in (off, on):
            e.set_precision(precision)
        w = "%s %s" % (what, precision)
        want = off.forward(*FX)
        want_t = _tensors(off, cfg, B, H, W)
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        assert not _same(off.forward(*X), want), w + ": the mirrored batch is another batch"
        assert _same(on.forward(*X), want), w + ": davo_forward"
        for k, t in _tensors(on, cfg, B, H, W).items():
            assert _same(t, want_t[k]), w + ": davo_forward, " + k
        for timed in (False, True):
            got, after = _device_forward(on, X, timed)
            assert _same(got, want), w + ": davo_forward_device timed=%s" % timed
            for a, b in zip(after, X):
                assert _same(a, b), w + ": davo_forward_device wrote a caller's buffer"
        for k, t in _tensors(on, cfg, B, H, W).items():
            assert _same(t, want_t[k]), w + ": davo_forward_device, " + k
        assert _same(_device_forward(off, FX)[0], want)
        for got in _streamed(on, X):
            assert _same(got, want), w + ": davo_submit"
        for k, t in _tensors(on, cfg, B, H, W).items():
            assert _same(t, want_t[k]), w + ": davo_submit, " + k
        if not frames:
            continue
        fr = _frames(cfg, B, H, W, labels, flow)
        want_f = off.forward(*flip_windows(*windows_from_frames(*fr)))
        want_ft = _tensors(off, cfg, B, H, W)
        assert _same(off.forward_frames(*flip_frames(*fr)), want_f)
        assert _same(on.forward_frames(*fr), want_f), w + ": davo_forward_frames"
        for k, t in _tensors(on, cfg, B, H, W).items():
            assert _same(t, want_ft[k]), w + ": davo_forward_frames, " + k
        for got in _streamed(on, fr, frames=True):
            assert _same(got, want_f), w + ": davo_submit_frames"
        got, after = _device_frames(on, fr)
        assert _same(got, want_f), w + ": davo_forward_device_frames"
        for a, b in zip(after, fr):
            assert _same(a, b), w + ": davo_forward_device_frames wrote a caller's buffer"
    assert off.range_stats() == on.range_stats()


# ---- every entry point, format, precision and row form -----------------------------------------------------------------------
@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("name,version", [("flagship", FLAGSHIP_VERSION), ("se_SegFlow_to_seg", SEGFLOW)])
def test_every_entry_point_and_format(name, version, H, W):
    cfg = parse_version(version)
    weights = synth.make_weights(cfg)
    for labels, flow in FORMATS:
        off, on = _pair(cfg, H, W, 3, labels, flow, weights)
        for B in (1, 3):
            _check_every_entry_point(cfg, off, on, B, H, W, labels, flow, "%s %dx%d %s/%s B=%d" % (name, H, W, labels, flow, B))
        off.close()
        on.close()


@pytest.mark.parametrize("labels,flow", [("f32", "f32"), ("u8", "f16")])
def test_a_call_of_several_sub_batches(labels, flow):
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    off, on = _pair(cfg, H, W, B, labels, flow)
    X = _inputs(cfg, B, H, W, labels, flow)
    want = off.forward(*flip_windows(*X))
    for e in (off, on):
        e.set_option("host_chunk", 1)                         # B >= 2 chunks: three sub-batches, three window_mirror launches
    on.profile(1)
    on.profile_reset()
    assert _same(on.forward(*X), want) and _same(off.forward(*flip_windows(*X)), want)
    assert on.profile_entries()["window_mirror"][0] == 3
    on.profile(0)
    fr = _frames(cfg, B, H, W, labels, flow)
    assert _same(on.forward_frames(*fr), off.forward_frames(*flip_frames(*fr)))
    off.close()
    on.close()


# ---- variants ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,version", [("se_depth_to_seg", DEPTH_SOURCE), ("depthseg_seplayers", DEPTH_SPLIT)])
def test_the_depth_forms(name, version):
    cfg = parse_version(version)
    assert cfg.needs_depth
    H, W = 36, 100
    off, on = _pair(cfg, H, W, 3)
    for B in (1, 3):
        _check_every_entry_point(cfg, off, on, B, H, W, "f32", "f32", "%s B=%d" % (name, B))
    off.close()
    on.close()


def test_a_pooled_source_whose_squeeze_is_not_mirror_symmetric():
    import pooled_flow_ref as R
    cfg = parse_version(R.version("se_spp864_flow"))
    B, H, W = 3, 36, 100
    img, flow, _ = R.make_inputs(B, H, W, 3)
    X = (img, flow, _pixel_labels((B, 3, H, W, 1), 5, "f32"))
    off, on = _pair(cfg, H, W, B)
    off.forward(*X)
    plain = off.debug_read("att_table", (B, 3, 19))
    want = off.forward(*flip_windows(*X))
    mirrored = off.debug_read("att_table", (B, 3, 19))
    assert not _same(plain, mirrored) and np.abs(plain - mirrored).max() > 1e-4      # the pooled descriptor sees the mirror
    assert _same(on.forward(*X), want) and _same(on.debug_read("att_table", (B, 3, 19)), mirrored)
    _check_every_entry_point(cfg, off, on, B, H, W, "f32", "f32", "se_spp864_flow", frames=True)
    off.close()
    on.close()


def test_the_three_frame_topology():
    cfg = parse_version(TRIPLET)
    assert cfg.posenn == "triplet"
    H, W = 36, 100
    off, on = _pair(cfg, H, W, 3, "u8", "f16")
    for B in (1, 3):
        _check_every_entry_point(cfg, off, on, B, H, W, "u8", "f16", "three-frame B=%d" % B)
    off.close()
    on.close()


# ---- pair selection: what no selected pair reads is neither read nor written --------------------------------------------------
@pytest.mark.parametrize("name,version", [("flagship", FLAGSHIP_VERSION), ("se_depth_to_seg", DEPTH_SOURCE), ("depthseg_seplayers", DEPTH_SPLIT)])
def test_one_pair_with_the_unread_planes_poisoned(name, version):
    cfg = parse_version(version)
    B, H, W = 3, 36, 100
    off, on = _pair(cfg, H, W, B)
    X = _inputs(cfg, B, H, W)
    for e in (off, on):
        e.set_pairs("src1")
    want = off.forward(*flip_windows(*X))
    assert _same(on.forward(*X), want)
    clean_range = on.activation_range()
    P = [a.copy() for a in X]
    P[0][:, :, :W] = 0xA5                                     # src0's third of the strip
    P[1][:, 0] = np.nan                                       # its flow plane, and the two planes nothing reads
    P[1][:, 2:] = np.nan
    P[2][:, 0] = np.nan                                       # its label map
    if not cfg.tgt_attended:
        P[2][:, 1] = np.nan                                   # the target's map where the variant does not attend it
    if cfg.needs_depth:
        P[3][:, 0] = np.nan                                   # src0's depth plane
        if cfg.att_source == "se_flow_depthseg_sep":
            P[3][:, 1] = np.nan                               # the depth-split attention reads the source frame's plane alone
    for what, got in (("davo_forward", on.forward(*P)), ("davo_forward_device", _device_forward(on, P)[0]), ("davo_submit", _streamed(on, P)[0])):
        assert np.isfinite(got).all() and _same(got, want), "%s: %s" % (name, what)
    assert on.activation_range() == clean_range
    # frame layout: the frames no selected window reads (frame 0 of the pixels; the header's table)
    fr = _frames(cfg, B, H, W)
    want_f = off.forward_frames(*flip_frames(*fr))
    Pf = [a.copy() for a in fr]
    Pf[0][0] = 0xA5
    Pf[1][:, 0] = np.nan
    Pf[2][0 if cfg.tgt_attended else slice(0, 2)] = np.nan
    assert _same(on.forward_frames(*Pf), want_f) and _same(_device_frames(on, Pf)[0], want_f)
    off.close()
    on.close()


# ---- launches -----------------------------------------------------------------------------------------------------------------
def _launches(e, call):
    e.profile(1)
    e.profile_reset()
    call()
    e.synchronize()
    out = {k: n for k, (n, _) in e.profile_entries().items() if n > 0}
    e.profile(0)
    return out


def test_launch_counts():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    off, on = _pair(cfg, H, W, B)
    X, fr = _inputs(cfg, B, H, W), _frames(cfg, B, H, W)
    FX, Ffr = flip_windows(*X), flip_frames(*fr)
    for call_on, call_off in ((lambda: on.forward_frames(*fr), lambda: off.forward_frames(*Ffr)),
                              (lambda: _device_frames(on, fr), lambda: _device_frames(off, Ffr))):
        a, b = _launches(on, call_on), _launches(off, call_off)
        assert a == b and a["window_gather"] == 1 and "window_mirror" not in a, (a, b)
    for call_on, call_off in ((lambda: on.forward(*X), lambda: off.forward(*FX)),
                              (lambda: _device_forward(on, X), lambda: _device_forward(off, FX)),
                              (lambda: _streamed(on, X, n=1), lambda: _streamed(off, FX, n=1))):
        a, b = _launches(on, call_on), _launches(off, call_off)
        assert a.pop("window_mirror") == 1 and a == b, (a, b)         # exactly one launch more, and it is the mirror
    off.close()
    on.close()


# ---- range recovery: a re-issue must not mirror again -------------------------------------------------------------------------
def _rescaled(weights, shift):
    """tests/test_hip_parity.py's guard recipe: cnv3's activations x 2^shift, undone in cnv4 - the same network, outside the
    fp16-pair range of the default scales."""
    k = np.float32(2.0 ** shift)
    w2 = dict(weights)
    w2["pose_exp_net/cnv3/weights"] = weights["pose_exp_net/cnv3/weights"] * k
    w2["pose_exp_net/cnv3/biases"] = weights["pose_exp_net/cnv3/biases"] * k
    w2["pose_exp_net/cnv4/weights"] = weights["pose_exp_net/cnv4/weights"] / k
    return w2


@pytest.mark.parametrize("entry", ["davo_forward", "davo_submit", "davo_forward_device", "davo_forward_frames"])
def test_a_reissued_batch_is_not_mirrored_twice(entry):
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    X, fr = _inputs(cfg, B, H, W), _frames(cfg, B, H, W)
    FX = flip_windows(*X)
    calls = {"davo_forward": lambda e, on: e.forward(*(X if on else FX)),
             "davo_submit": lambda e, on: _streamed(e, X if on else FX, n=1)[0],
             "davo_forward_device": lambda e, on: _device_forward(e, X if on else FX)[0],
             "davo_forward_frames": lambda e, on: e.forward_frames(*(fr if on else flip_frames(*fr)))}
    off, on = _pair(cfg, H, W, B, weights=_rescaled(synth.make_weights(cfg), 16))
    want, got = calls[entry](off, False), calls[entry](on, True)
    assert np.isfinite(want).all() and np.abs(want).max() > 0 and _same(got, want)
    st = on.range_stats()
    assert st["reissued"] >= 1 and st["recalibrations"] >= 1 and st == off.range_stats(), (st, on.range_report())
    assert on.activation_range() == off.activation_range()
    off.close()
    on.close()


@pytest.mark.parametrize("entry", ["davo_forward", "davo_submit", "davo_forward_device"])
def test_a_batch_reissued_on_the_float32_kernels_is_not_mirrored_twice(entry):
    """tests/test_hip_parity.py's recipe: cnv3's activations at 2^-80, which no storage scale brings into the fp16-pair range - the
    re-issue ends on the float32 kernels, reading the same mirrored copy"""
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    X = _inputs(cfg, B, H, W)
    FX = flip_windows(*X)
    calls = {"davo_forward": lambda e, A: e.forward(*A), "davo_submit": lambda e, A: _streamed(e, A, n=1)[0],
             "davo_forward_device": lambda e, A: _device_forward(e, A)[0]}
    off, on = _pair(cfg, H, W, B, weights=_rescaled(synth.make_weights(cfg), -80))
    want, got = calls[entry](off, FX), calls[entry](on, X)
    assert np.isfinite(want).all() and np.abs(want).max() > 0 and _same(got, want)
    st = on.range_stats()
    assert st["f32_batches"] >= 1 and st["reissued"] >= 1 and st == off.range_stats(), (st, on.range_report())
    off.close()
    on.close()


# ---- toggling -----------------------------------------------------------------------------------------------------------------
def test_toggling_between_batches():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    X = _inputs(cfg, B, H, W)
    off, on = _pair(cfg, H, W, B)
    want_plain, want_flip = off.forward(*X), off.forward(*flip_windows(*X))
    assert not _same(want_plain, want_flip)
    outs = [np.full((B, 2, 6), np.nan, np.float32) for _ in range(4)]
    for i, out in enumerate(outs):                            # on, off, on, off: each batch is delivered with the setting it was issued with
        on.set_flip(i % 2 == 0)
        on.submit(*X, out)
    on.set_flip(True)                                         # a change after the last submit touches none of them
    on.wait(0)
    on.synchronize()
    for i, out in enumerate(outs):
        assert _same(out, want_flip if i % 2 == 0 else want_plain), i
    # flipped once, then off again: a fresh flip-off engine's bits and plan
    on.set_flip(False)
    assert on.flip is False
    fresh = Engine(cfg, H, W, B)
    fresh.load_weights(synth.make_weights(cfg))
    for precision in PRECISIONS:
        for e in (on, fresh):
            e.set_precision(precision)
        assert _same(on.forward(*X), fresh.forward(*X))
        assert [on.last_plan(l) for l in range(7)] == [fresh.last_plan(l) for l in range(7)]
        assert _same(_device_forward(on, X)[0], _device_forward(fresh, X)[0])
    names = _launches(on, lambda: on.forward(*X))
    assert "window_mirror" not in names and names == _launches(fresh, lambda: fresh.forward(*X))
    for e in (off, on, fresh):
        e.close()


# ---- exports and the class ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,version", [("flagship", FLAGSHIP_VERSION), ("se_SegFlow_to_seg", SEGFLOW)])
def test_exports(name, version):
    cfg = parse_version(version)
    B, H, W = 3, 36, 100
    X = _inputs(cfg, B, H, W)
    FX = flip_windows(*X)
    want_all = Engine.FEATURE_OUTPUTS + Engine.HEAT_OUTPUTS
    off, on = _pair(cfg, H, W, B)
    got = []
    for e, A in ((off, FX), (on, X)):
        e.set_feature_export(True)
        e.set_heat_export(True)
        r = [e.forward_features(*A, want=want_all)]
        e.set_option("host_chunk", 1)                        # sub-batches of one window
        r.append(e.forward_features(*A, want=want_all))
        got.append(r)
    for r_off, r_on in zip(*got):
        assert set(r_off) == set(r_on) == {"pose"} | set(want_all)
        for k in r_off:
            assert _same(r_off[k], r_on[k]), "%s: %s differs" % (name, k)
    assert not _same(got[0][0]["attention"], off.forward_features(*X, want=("attention",))["attention"])
    off.close()
    on.close()


def _flat(x, prefix=""):
    if isinstance(x, dict):
        return {k2: v2 for k, v in x.items() for k2, v2 in _flat(v, prefix + k + ".").items()}
    if isinstance(x, list):
        return {k2: v2 for i, v in enumerate(x) for k2, v2 in _flat(v, prefix + "%d." % i).items()}
    return {prefix: x}


@pytest.mark.parametrize("features", ["full", "heat"])
def test_the_reference_call_surface(features):
    B, H, W = 2, 36, 100
    cfg = parse_version(FLAGSHIP_VERSION)
    X = _inputs(cfg, B, H, W)
    FX = flip_windows(*X)
    weights = synth.make_weights(cfg)
    outs = []
    for flip, A in ((False, FX), (True, X)):
        d = DAVO(FLAGSHIP_VERSION, flip=flip).enable_feature_mode(features=features)
        d.setup_inference(H, W, "davo", 3, B, input_img_uint8=A[0], input_flow=A[1], input_seglabel=A[2])
        d.load_weights(weights)
        assert d.engine.flip is flip
        out = d.inference(mode="feature")
        assert _same(d.inference(mode="pose")["pose"], out["pose"])
        it = DAVO(FLAGSHIP_VERSION)
        it.setup_inference(H, W, "davo", 3, B, input_img_uint8=iter([A] * 2), flip=flip)      # the iterator inputs go through davo_submit
        it.load_weights(weights)
        assert it.engine.flip is flip
        assert _same(it.inference()["pose"], out["pose"]) and _same(it.inference()["pose"], out["pose"])
        it.engine.close()
        d.engine.close()
        outs.append(out)
    want, got = _flat(outs[0]), _flat(outs[1])
    assert set(got) == set(want) and len(want) > 8
    for k in want:
        assert _same(got[k], want[k]), k


# ---- housekeeping ---------------------------------------------------------------------------------------------------------------
def test_errors():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 1, 16, 16
    X = _inputs(cfg, B, H, W)
    e = Engine(cfg, H, W, B)
    e.load_weights(synth.make_weights(cfg))
    L = e._L
    for bad in (2, -1, 3):
        assert L.davo_set_flip(e._ctx, bad) == -1 and b"flip must be 0 (off) or 1 (on)" in L.davo_last_error(e._ctx)
        assert L.davo_get_flip(e._ctx) == 0
    with pytest.raises(ValueError, match="flip"):
        e.set_flip(2)
    assert L.davo_set_flip(e._ctx, 1) == 0 and L.davo_get_flip(e._ctx) == 1 and e.flip is True
    # independent of the other settings, before and after inputs were taken
    assert L.davo_set_pairs(e._ctx, 2) == 0 and L.davo_set_flip(e._ctx, 0) == 0 and L.davo_set_pairs(e._ctx, 3) == 0
    e.forward(*X)
    e.set_flip(True)
    # with flip on the mirror reads the caller's device buffers in 16-byte units
    bufs = [e.alloc(a.nbytes + 64).upload(a) for a in X]
    d_pose = e.alloc(B * 12 * 4)
    rc = L.davo_forward_device(e._ctx, B, ctypes.c_void_p(bufs[0].ptr.value + 4), bufs[1].ptr, bufs[2].ptr, d_pose.ptr, None)
    assert rc == -1 and b"16-byte aligned" in L.davo_last_error(e._ctx)
    assert L.davo_forward_device(e._ctx, B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, d_pose.ptr, None) == 0
    e.synchronize()
    for b in bufs + [d_pose]:
        b.free()
    assert e.pending() == 0
    e.close()


def test_ten_cycles_leave_no_device_memory_behind():
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 3, 36, 100
    X, fr = _inputs(cfg, B, H, W), _frames(cfg, B, H, W)
    weights = _rescaled(synth.make_weights(cfg), 16)          # every cycle also re-issues a batch
    free = []
    for _ in range(10):
        e = Engine(cfg, H, W, B)
        e.load_weights(weights)
        e.set_inflight(2)
        e.set_flip(True)
        _streamed(e, X, n=2)
        _streamed(e, fr, n=2, frames=True)
        e.forward(*X)
        _device_forward(e, X)
        assert e.range_stats()["reissued"] >= 1
        e.close()
        free.append(hip_free_bytes())
    assert all(f == free[0] for f in free), free


def test_the_driver_with_flip_from_a_dump_equals_the_driver_on_the_flipped_dump(tmp_path):
    """run_kitti_pose.main in this process (like the other driver tests).  The dumps' strips are stored losslessly (PNG data under
    the .jpg names, Pillow reads by content): a JPEG of a mirrored strip does not decode to the mirror of the JPEG."""
    import os
    from PIL import Image
    from davo_amd import loader as L, run_kitti_pose as R
    H, W, seq, n = 36, 100, 3, 7
    X = synth.make_inputs(n - 2, H, W, first_window=20)
    X = (X[0], X[1], _pixel_labels(X[2].shape, 3, "f32"))
    dumps = {"plain": X, "flipped": flip_windows(*X)}
    for name, (img, flow, seg) in dumps.items():
        os.makedirs(str(tmp_path / name / ("%.2d" % seq)))
        for w in range(n - 2):
            jpg, flo, sg = L.window_paths(str(tmp_path / name), seq, w + 1)
            Image.fromarray(img[w]).save(jpg, format="PNG")
            np.save(flo, flow[w])
            np.save(sg, seg[w])
    ckpt = str(tmp_path / "w.npz")
    np.savez(ckpt, **synth.make_weights(FLAGSHIP_VERSION))
    files = {}
    for out, dump, extra in (("a", "plain", ["--flip"]), ("b", "flipped", []), ("c", "plain", [])):
        args = ["--test_seq", str(seq), "--concat_img_dir", str(tmp_path / dump), "--ckpt_file", ckpt, "--output_dir", str(tmp_path / out),
                "--img_height", str(H), "--img_width", str(W), "--batch_size", "2", "--loader_procs", "2"] + extra
        try:
            R.main(args)
        except Exception:
            import traceback
            pytest.fail("run_kitti_pose %s failed:\n%s" % (" ".join(args), traceback.format_exc()), pytrace=False)
        files[out] = open(str(tmp_path / out / ("%.2d-pred_kitti_pose.txt" % seq)), "rb").read()
    assert files["a"] == files["b"] and files["a"] != files["c"] and len(files["a"].splitlines()) == n
