"""Binary16 depth planes on the GPU (include/davo_hip.h: davo_set_depth_format).

Every comparison is between a float32-depth engine on depth_from_f16(h) and a binary16-depth engine on h, with the same
weights, options, other inputs and call sequence, and every such comparison is to the bit: the kernels widen each half exactly
(csrc/input_decode.h: depth_fetch4) and run the float32 format's expressions in its order from there on.  Each case also holds
the binary16 engine against the float64 restatements (tests/depth_source_ref.py, tests/depthseg_attention_ref.py) at the
project's existing bars - layer_check's table and packed bars, helpers' pose bar - so the two engines cannot be wrong together
(the cases that compute nothing of their own - error codes, device memory, launch counts - excepted).
The cases, and why reading anything but the halves' values would show, are tests/f16_depth_cases.py's (preconditions checked in
tests/test_f16_depth.py)."""
import ctypes

import numpy as np
import pytest

from davo_amd import DAVO, Engine, depth_from_f16, flip_frames, flip_windows, flow_to_f16, labels_to_u8, synth, windows_from_frames

import f16_depth_cases as C
import layer_check as LC
from helpers import assert_pose_close, hip_free_bytes

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["%dx%d" % s[:2] for s in C.SHAPES]
NAN16, INF16 = 0x7E00, 0x7C00


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _engines(c, H, W, max_batch, weights=None, **fmt):
    """-> (the float32-depth engine, the binary16-depth engine), same weights and other formats"""
    pair = (Engine(c.cfg, H, W, max_batch, **fmt), Engine(c.cfg, H, W, max_batch, depth="f16", **fmt))
    for e in pair:
        e.load_weights(c.weights if weights is None else weights)
    assert pair[0]._L.davo_get_depth_format(pair[0]._ctx) == 0 and pair[1]._L.davo_get_depth_format(pair[1]._ctx) == 1
    assert pair[0].depth == "f32" and pair[1].depth == "f16"
    return pair


def _close(*engines):
    for e in engines:
        e.close()


def _tensors(e, c, B, H, W, pairs=2):
    out = {"att_table": e.debug_read("att_table", (B, 3, 19)), "packed": e.debug_read("packed", (pairs * B, H, W, 8)),
           "cnv1": e.debug_read("cnv1", (pairs * B, (H + 1) // 2, (W + 1) // 2, 16))}
    if c.source == 13:
        out["att_table_far"] = e.debug_read("att_table_far", (B, 3, 19))
    return out


# ---- tensors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", C.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("source", C.SOURCES)
def test_tensors_are_the_float32_engines_to_the_bit(source, H, W, B):
    """att_table (and att_table_far), packed, cnv1 and the poses, both precisions, the squeeze with the excitation folded in and
    as a launch of its own ("fold_tails" 1 / 0: both FOLD arms of se_depth_squeeze); then the binary16 engine against float64."""
    c = C.case(source, H, W, B)
    e32, e16 = _engines(c, H, W, B)
    what = "source %d %dx%d B=%d" % (source, H, W, B)
    for precision in ("f16x3", "f32"):
        for fold in (0, 1, -1):
            got = []
            for e, depth in ((e32, c.wide), (e16, c.h)):
                e.set_precision(precision)
                e.set_option("fold_tails", fold)
                t = {"pose": e.forward(c.img, c.flow, c.seg, depth)}
                t.update(_tensors(e, c, B, H, W))
                got.append(t)
            for k in got[0]:
                assert _same(got[0][k], got[1][k]), "%s %s fold_tails=%d: %s differs" % (what, precision, fold, k)
            assert np.isfinite(got[1]["pose"]).all() and np.abs(got[1]["pose"]).max() > 0
            assert e32.activation_range() == e16.activation_range()
        # ... and against the float64 restatement on the widened halves, at the existing bars
        t = got[1]
        if source == 13:
            near, far = C.reference_tables(c)
            LC.check_table(t["att_table"], near, [1, 2], what + " near")
            LC.check_table(t["att_table_far"], far, [1, 2], what + " far")
        else:
            LC.check_table(t["att_table"], C.reference_tables(c), [0, 1, 2] if c.cfg.tgt_attended else [1, 2], what)
        want_p = C.ref(source).pack(c.cfg, c.img, c.flow, c.seg, c.wide, c.weights).reshape(2 * B, H, W, 10)[..., LC.PACK8]
        LC.check_packed(t["packed"], want_p, what + " " + precision)
        err = assert_pose_close(t["pose"], C.reference_poses(c, None), what + " " + precision)
        print("%s %s: pose max|err| against float64 %.3g" % (what, precision, err))
    assert e32.range_stats() == e16.range_stats()
    _close(e32, e16)


# ---- special values ---------------------------------------------------------------------------------------------------
SUB_MIN, SUB_MAX, ZERO, NZERO, MAX16, NMAX16, NINF16 = 0x0001, 0x03FF, 0x0000, 0x8000, 0x7BFF, 0xFBFF, 0xFC00
SPECIAL_BITS = (SUB_MIN, 0x8001, SUB_MAX, 0x83FF, ZERO, NZERO, MAX16, NMAX16, INF16, NINF16, NAN16)
#               smallest / largest subnormal (+-), +-0, +-65504, +-inf, the quiet NaN
SPOTS = ((0, 0), (35, 99), (0, 99), (35, 0), (17, 3), (18, 50), (5, 97), (30, 64), (9, 9), (20, 20), (33, 1))      # first and last pixel, unit edges


def _table_specials(h):
    """Sources 11, 12 at 36x100, B = 3 - a plane's SUM is what the kernel makes of it, so every kind of special value gets planes
    of its own:
      window 0   finite specials alone, in all three planes: subnormals, +-0, and +65504 twice against -65504 once - the sums stay
                 finite and move by 65504 a plane (a mean shifted by 18: a widening that made 65504 an infinity, or lost its sign,
                 shows in the table against float64);
      window 1   +inf alone in src0's plane, -inf alone in src1's: an infinite sum of either sign reaches the excitation, not a NaN
                 (tanh saturates: the rows are finite and differ from window 0's); the target's plane is finite;
      window 2   NaN alone, in src1's plane: that frame's row is NaN, the other two rows are untouched."""
    hh = h.copy()
    raw = hh.view(np.uint16)
    finite = (SUB_MIN, 0x8001, SUB_MAX, 0x83FF, ZERO, NZERO, MAX16, NMAX16, MAX16, SUB_MAX, NZERO)
    for plane in range(3):
        for (y, x), bits in zip(SPOTS, finite):
            raw[0, plane, y, x, 0] = bits
    raw[1, 0, 17, 3, 0] = INF16
    raw[1, 2, 35, 99, 0] = NINF16
    raw[2, 2, 0, 0, 0] = NAN16
    return hh


@pytest.mark.parametrize("source", [11, 12])
def test_special_values_reach_the_tables(source):
    """Float32 precision (no range guard), both FOLD arms: att_table and packed to the bit against the float32 engine on the
    widened halves, and att_table against the float64 restatement at layer_check's bar - window by window, so that each kind of
    special value is judged on planes that hold no other.  (A zero's sign cannot show in any output: a sum with other terms
    drops it and -0 < thr is +0 < thr; the exact-sum test below covers subnormals and zeros on planes of their own.)"""
    H, W, B = 36, 100, 3
    c = C.case(source, H, W, B)
    hh = _table_specials(c.h)
    wide = depth_from_f16(hh)
    assert np.isfinite(wide[0]).all() and (wide[0] == 65504).sum() == 6 and (wide[0] == -65504).sum() == 3
    assert np.isposinf(wide[1, 0]).sum() == 1 and np.isneginf(wide[1, 2]).sum() == 1 and np.isfinite(wide[1, 1]).all()
    assert np.isnan(wide[2, 2]).sum() == 1 and np.isfinite(wide[2, :2]).all() and np.array_equal(np.signbit(wide), np.signbit(hh))
    with np.errstate(invalid="ignore", over="ignore"):
        want = C.ref(source).class_tables(c.cfg, wide, c.weights)
        plain = C.ref(source).class_tables(c.cfg, c.wide, c.weights)
    rows = [0, 1, 2] if c.cfg.tgt_attended else [1, 2]
    assert np.isfinite(want[:2]).all() and np.isnan(want[2, 2]).all() and np.isfinite(want[2, :2]).all()
    for b in (0, 1):                                         # on the restatement: the special values decide these tables
        assert np.abs(want[b, 1:] - plain[b, 1:]).max() > 100 * LC.TABLE_TOL, b
    e32, e16 = _engines(c, H, W, B)
    for fold in (0, 1):
        got = []
        for e, depth in ((e32, wide), (e16, hh)):
            e.set_precision("f32")
            e.set_option("fold_tails", fold)
            e.forward(c.img, c.flow, c.seg, depth)
            got.append(_tensors(e, c, B, H, W))
        what = "source %d fold_tails=%d" % (source, fold)
        for k in ("att_table", "packed"):
            assert _same(got[0][k], got[1][k]), "%s: %s differs" % (what, k)
        tab = got[1]["att_table"]
        for b in (0, 1):
            assert np.isfinite(tab[b]).all()
            LC.check_table(tab[b:b + 1], want[b:b + 1], rows, "%s window %d" % (what, b))
        assert np.isnan(tab[2, 2]).all(), what + ": the NaN plane's row"
        LC.check_table(tab[2:3], want[2:3], [r for r in rows if r != 2], what + " window 2")
    _close(e32, e16)


def _split_specials(h):
    """Source 13: every special value in both source planes of every window, on the first and the last pixel and on unit edges"""
    hh = h.copy()
    raw = hh.view(np.uint16)
    k = 0
    for b in range(hh.shape[0]):
        for plane in range(3):
            for y, x in SPOTS:
                raw[b, plane, y, x, 0] = SPECIAL_BITS[k % len(SPECIAL_BITS)]
                k += 1
    for bits in SPECIAL_BITS:
        assert (raw[:, (0, 2)] == bits).any()
    return hh


def test_special_values_against_the_threshold():
    """Source 13, float32 precision, both arms of "fold_tails": the tables and packed to the bit, and packed against the
    restatement, whose float32 compare sends a NaN depth to the far side, as the header says, -inf, -65504, the zeros and the
    subnormals near and +65504 and +inf far."""
    source, H, W, B = 13, 36, 100, 3
    c = C.case(source, H, W, B)
    hh = _split_specials(c.h)
    wide = depth_from_f16(hh)
    assert np.isnan(wide).any() and np.isinf(wide).any() and np.array_equal(np.signbit(wide), np.signbit(hh))
    R = C.ref(13)
    near = R.near_mask(wide, c.weights[R.THRESHOLD])
    raw = hh.view(np.uint16)[..., 0]
    for bits, side in ((NAN16, False), (INF16, False), (MAX16, False), (NINF16, True), (NMAX16, True), (ZERO, True), (NZERO, True),
                       (SUB_MIN, True), (SUB_MAX, True)):
        assert (near[raw == bits] == side).all(), hex(bits)
    want_p = R.pack(c.cfg, c.img, c.flow, c.seg, wide, c.weights).reshape(2 * B, H, W, 10)[..., LC.PACK8]
    e32, e16 = _engines(c, H, W, B)
    for fold in (0, 1):
        got = []
        for e, depth in ((e32, wide), (e16, hh)):
            e.set_precision("f32")
            e.set_option("fold_tails", fold)
            e.forward(c.img, c.flow, c.seg, depth)
            got.append(_tensors(e, c, B, H, W))
        for k in ("att_table", "att_table_far", "packed"):
            assert _same(got[0][k], got[1][k]), "source 13 fold_tails=%d: %s differs" % (fold, k)
        LC.check_packed(got[1]["packed"], want_p, "source 13 special values")
    _close(e32, e16)


@pytest.mark.parametrize("source", [11, 12])
def test_the_squeeze_sums_planes_of_small_halves_exactly(source):
    """Subnormals and signed zeros alone: every partial sum of se_depth_squeeze is exact in float32 (integers times 2^-24), so
    the table is that of the exact mean - a widening that flushed subnormals to zero would give the all-zero planes' table.
    Both FOLD arms."""
    H, W, B = 36, 100, 3
    c = C.case(source, H, W, B)
    rng = np.random.default_rng(7)
    raw = rng.integers(1, 0x0400, c.h.shape).astype(np.uint16)          # subnormals only ...
    raw[rng.random(c.h.shape) < 0.05] = NZERO                            # ... and some zeros of either sign
    raw[rng.random(c.h.shape) < 0.05] = ZERO
    hh = raw.view(np.float16)
    wide = depth_from_f16(hh)
    assert (wide >= 0).all() and wide.max() < 2.0 ** -14 and (wide > 0).mean() > 0.8
    big = dict(c.weights)
    k = "pose_exp_net/se_depth/bottleneck_fc/kernel"
    big[k] = (np.asarray(c.weights[k], np.float64) * 2.0 ** 19).astype(np.float32)      # the tiny mean decides the table
    zero = C.ref(source).class_tables(c.cfg, np.zeros_like(wide), big)
    want = C.ref(source).class_tables(c.cfg, wide, big)
    rows = [0, 1, 2] if c.cfg.tgt_attended else [1, 2]
    assert np.abs(want - zero)[:, rows].max() > 100 * LC.TABLE_TOL
    e32, e16 = _engines(c, H, W, B, big)
    for fold in (0, 1):
        for e, depth in ((e32, wide), (e16, hh)):
            e.set_precision("f32")
            e.set_option("fold_tails", fold)
            e.forward(c.img, c.flow, c.seg, depth)
        got = e16.debug_read("att_table", (B, 3, 19))
        assert _same(got, e32.debug_read("att_table", (B, 3, 19)))
        LC.check_table(got, want, rows, "source %d subnormal depth fold_tails=%d" % (source, fold))
    _close(e32, e16)


# ---- every entry point ------------------------------------------------------------------------------------------------
def _device_forward(e, B, img, flow, seg, depth, timed=False):
    arrays = [img, flow, seg, depth]
    bufs = [e.alloc(a.nbytes).upload(a) for a in arrays]
    d_pose = e.alloc(B * 12 * 4)
    try:
        e.forward_device(B, bufs[0], bufs[1], bufs[2], d_pose, timed=timed, depth=bufs[3])
        e.synchronize()
        return d_pose.download((B, 2, 6)), [b.download(a.shape, a.dtype) for b, a in zip(bufs, arrays)]
    finally:
        for b in bufs + [d_pose]:
            b.free()


def _streamed(e, img, flow, seg, depth, n=3, hold=0, frames=False):
    """n submits of the batch; hold = 0: from scratch arrays that are overwritten as soon as each submit returns"""
    src = (img, flow, seg, depth)
    scratch = [np.empty_like(a) for a in src]
    if hold:
        scratch = [[s.copy() for s in scratch] for _ in range(n)]
    outs = [np.full((flow.shape[0], 2, 6), np.nan, np.float32) for _ in range(n)]
    for i, out in enumerate(outs):
        sc = scratch[i] if hold else scratch
        for dst, a in zip(sc, src):
            dst[...] = a
        (e.submit_frames if frames else e.submit)(sc[0], sc[1], sc[2], out, hold=hold, depth=sc[3])
        if not hold:
            sc[0][...] = 77
            sc[1][...] = 1000.0
            sc[2][...] = 3
            sc[3][...] = 0.25
    e.wait(0)
    e.synchronize()
    return outs


def _in_pieces(fn, B, step, *arrays):
    return np.concatenate([fn(*[a[b0:b0 + step] for a in arrays]) for b0 in range(0, B, step)])


ROWS = {"both": [0, 1], "src0": [0], "src1": [1]}


def _hide_unread(h, source, pairs):
    """NaN halves in the depth planes no selected pair reads: source 13 never reads the target's plane; a one-pair batch does
    not read the other source's plane - and sources 11, 12 still read the target's."""
    hh = h.copy()
    raw = hh.view(np.uint16)
    if source == 13:
        raw[:, 1] = NAN16
    if pairs != "both":
        raw[:, 2 if pairs == "src0" else 0] = NAN16
    return hh


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("source", C.SOURCES)
def test_every_depth_entry_point(source, B):
    """davo_forward_depth (in pieces of max_batch and, on a larger context, in the library's own sub-batches of "host_chunk"),
    davo_forward_device_depth, davo_submit_depth and davo_calibrate_depth - with byte labels and binary16 flow, under every pair
    selection, the unread depth planes holding NaN halves."""
    H, W, MAXB = 36, 100, 4
    c = C.case(source, H, W, B)
    img, flow, seg = c.img, flow_to_f16(c.flow), labels_to_u8(c.seg)
    fmt = {"labels": "u8", "flow": "f16"}
    e32, e16 = _engines(c, H, W, MAXB, **fmt)
    big = _engines(c, H, W, 9, **fmt)
    for e in (e32, e16):
        e.set_inflight(4)
    step = min(B, MAXB)
    ref64 = C.reference_poses(c, None, flow16=True)          # the restatement on the widened halves and the rounded flow
    for pairs in ("src0", "src1", "both"):
        hh = _hide_unread(c.h, source, pairs)
        wide = depth_from_f16(hh)
        assert np.isnan(wide).any() == (source == 13 or pairs != "both")
        for e in (e32, e16) + big:
            e.set_pairs(pairs)
        what = "source %d B=%d %s" % (source, B, pairs)
        want = _in_pieces(e32.forward, B, step, img, flow, seg, wide)
        assert np.isfinite(want).all() and np.abs(want).max() > 0
        got16 = _in_pieces(e16.forward, B, step, img, flow, seg, hh)
        assert _same(got16, want), what + ": davo_forward_depth"
        rows = ROWS[pairs]                                     # ... and against float64: the rows the selection computes
        assert_pose_close(got16[:, rows], ref64[:, rows], what + " against float64")
        for chunk in (8, 2):
            for e in big:
                e.set_option("host_chunk", chunk)
            assert _same(big[1].forward(img, flow, seg, hh), big[0].forward(img, flow, seg, wide)), what + ": davo_forward_depth, host_chunk %d" % chunk
        for timed in (False, True):
            dev = _in_pieces(lambda *a: _device_forward(e32, len(a[0]), *a, timed=timed)[0], B, step, img, flow, seg, wide)
            got = _in_pieces(lambda *a: _device_forward(e16, len(a[0]), *a, timed=timed)[0], B, step, img, flow, seg, hh)
            assert _same(dev, want) and _same(got, want), what + ": davo_forward_device_depth timed=%s" % timed
        for hold in (0, 1):
            for b0 in range(0, B, step):
                part = [a[b0:b0 + step] for a in (img, flow, seg, wide, hh)]
                s32 = _streamed(e32, part[0], part[1], part[2], part[3], hold=hold)
                s16 = _streamed(e16, part[0], part[1], part[2], part[4], hold=hold)
                for a, b in zip(s32, s16):
                    assert _same(a, want[b0:b0 + step]) and _same(b, a), what + ": davo_submit_depth hold=%d" % hold
    n = min(B, MAXB)
    hh = _hide_unread(c.h, source, "both")
    assert e32.calibrate(img[:n], flow[:n], seg[:n], depth_from_f16(hh)[:n]) == e16.calibrate(img[:n], flow[:n], seg[:n], hh[:n])
    for e in (e32, e16):
        e.set_pairs("both")
    assert _same(e32.forward(img[:n], flow[:n], seg[:n], depth_from_f16(hh)[:n]), e16.forward(img[:n], flow[:n], seg[:n], hh[:n]))
    assert e32.range_stats() == e16.range_stats() and e32.activation_range() == e16.activation_range()
    _close(e32, e16, *big)


def _device_frames(e, N, fr, timed=False):
    bufs = [e.alloc(a.nbytes).upload(a) for a in fr]
    d_pose = e.alloc(N * 12 * 4)
    try:
        e.forward_device_frames(N, bufs[0], bufs[1], bufs[2], d_pose, timed=timed, depth=bufs[3])
        e.synchronize()
        return d_pose.download((N, 2, 6)), [b.download(a.shape, a.dtype) for b, a in zip(bufs, fr)]
    finally:
        for b in bufs + [d_pose]:
            b.free()


@pytest.mark.parametrize("N", [1, 9])
@pytest.mark.parametrize("source", C.SOURCES)
def test_the_frame_layout(source, N):
    """the three `_frames' forms (davo_forward_frames in sub-batches of "host_chunk"): to the bit against the float32 engine's
    `_frames' call and against the binary16 engine's own window call on windows_from_frames; and against the float64 restatement
    on the windows the frames expand to (f16_depth_cases.frames_case, preconditions in tests/test_f16_depth.py)"""
    H, W = 36, 100
    c, fr = C.frames_case(source, N, H, W)
    fr16 = (fr[0], flow_to_f16(fr[1]), labels_to_u8(fr[2]), fr[4])
    assert fr16[3].dtype == np.float16 and fr16[3].shape == (N + 2, H, W, 1)
    fr32 = fr16[:3] + (depth_from_f16(fr16[3]),)
    win16 = windows_from_frames(*fr16)
    assert win16[3].dtype == np.float16 and np.array_equal(win16[3].view(np.uint16), c.h.view(np.uint16))
    ref64 = C.reference_poses(c, None, flow16=True)
    e32, e16 = _engines(c, H, W, 9, labels="u8", flow="f16")
    for e in (e32, e16):
        e.set_inflight(2)
    for pairs in ("both", "src1", "src0"):
        for e in (e32, e16):
            e.set_pairs(pairs)
        what = "source %d N=%d %s" % (source, N, pairs)
        for chunk in (2, 8):                                # (a call's sub-batching decides its launch plans: like with like)
            for e in (e32, e16):
                e.set_option("host_chunk", chunk)
            want = e32.forward_frames(*fr32)
            assert np.isfinite(want).all() and np.abs(want).max() > 0
            assert _same(e16.forward_frames(*fr16), want), what + ": davo_forward_frames, host_chunk %d" % chunk
            assert _same(e16.forward(*win16), want), what + ": the window form on the windows the caller would have built"
            assert_pose_close(want[:, ROWS[pairs]], ref64[:, ROWS[pairs]], what + " against float64, host_chunk %d" % chunk)
        s32, s16 = _streamed(e32, *fr32, hold=1, frames=True), _streamed(e16, *fr16, hold=1, frames=True)
        for a, b in zip(s32, s16):
            assert np.isfinite(a).all() and _same(a, s32[0]) and _same(b, a), what + ": davo_submit_frames"
        for timed in (False, True):
            dev = _device_frames(e32, N, fr32, timed)[0]
            got, after = _device_frames(e16, N, fr16, timed)
            assert np.isfinite(dev).all() and _same(dev, s32[0]) and _same(got, dev), what + ": davo_forward_device_frames timed=%s" % timed
            assert_pose_close(got[:, ROWS[pairs]], ref64[:, ROWS[pairs]], what + ": davo_forward_device_frames against float64")
            assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(after, fr16))
    _close(e32, e16)


# ---- flip -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,B", C.SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("source", [12, 13])
def test_flip(source, H, W, B):
    """a flip-on binary16 engine on h against a flip-off binary16 engine on flip_windows(h): window, device and frame layouts;
    the caller's device buffers are byte-identical afterwards.  (12 reads all three planes, 13 the two sources'.)"""
    c = C.case(source, H, W, B)
    off, on = (Engine(c.cfg, H, W, B, depth="f16") for _ in range(2))
    for e in (off, on):
        e.load_weights(c.weights)
        e.set_inflight(2)
    on.set_flip(True)
    X = (c.img, c.flow, c.seg, c.h)
    FX = flip_windows(*X)
    assert FX[3].dtype == np.float16 and not np.array_equal(FX[3], c.h)
    what = "source %d %dx%d B=%d" % (source, H, W, B)
    # the float64 restatement on the mirrored batch (the widened halves): what both engines must compute
    ref64 = C.ref(source).forward(c.cfg, FX[0], FX[1], FX[2], depth_from_f16(FX[3]), c.weights)
    fr = synth.make_frames(B + 2, H, W, depth="f16")
    Ffr = flip_windows(*windows_from_frames(*fr))
    ref64_f = C.ref(source).forward(c.cfg, Ffr[0], Ffr[1], Ffr[2], depth_from_f16(Ffr[3]), c.weights)
    for precision in ("f16x3", "f32"):
        for e in (off, on):
            e.set_precision(precision)
        want = off.forward(*FX)
        assert_pose_close(want, ref64, what + " %s: the mirrored batch against float64" % precision)
        want_t = _tensors(off, c, B, H, W)
        assert np.isfinite(want).all() and not _same(off.forward(*X), want), what + ": the mirrored batch is another batch"
        assert _same(on.forward(*X), want), what + ": davo_forward_depth"
        for k, t in _tensors(on, c, B, H, W).items():
            assert _same(t, want_t[k]), what + ": davo_forward_depth, " + k
        got, after = _device_forward(on, B, *X)
        assert _same(got, want), what + ": davo_forward_device_depth"
        for a, b in zip(after, X):
            assert np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what + ": a caller's device buffer was written"
        for k, t in _tensors(on, c, B, H, W).items():
            assert _same(t, want_t[k]), what + ": davo_forward_device_depth, " + k
        for got in _streamed(on, *X):
            assert _same(got, want), what + ": davo_submit_depth"
        want_f = off.forward(*Ffr)
        assert_pose_close(want_f, ref64_f, what + " %s: the mirrored frames against float64" % precision)
        assert _same(off.forward_frames(*flip_frames(*fr)), want_f)
        assert _same(on.forward_frames(*fr), want_f), what + ": davo_forward_frames"
        for got in _streamed(on, *fr, frames=True):
            assert _same(got, want_f), what + ": davo_submit_frames"
        got, after = _device_frames(on, B, fr)
        assert _same(got, want_f), what + ": davo_forward_device_frames"
        for a, b in zip(after, fr):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), what + ": a caller's frame buffer was written"
    assert off.range_stats() == on.range_stats()
    _close(off, on)


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


@pytest.mark.parametrize("streamed", [False, True], ids=["davo_forward_depth", "davo_submit_depth"])
@pytest.mark.parametrize("source", [11, 13])
def test_a_batch_that_trips_the_range_guard_is_reissued_from_the_halves(source, streamed):
    H, W, B = 36, 100, 3
    c = C.case(source, H, W, B)
    e32, e16 = _engines(c, H, W, B, _rescaled(c.weights, 16))
    if streamed:
        for e in (e32, e16):
            e.set_inflight(2)
        got32 = _streamed(e32, c.img, c.flow, c.seg, c.wide)       # scratch arrays overwritten: re-issued from the library's own copy
        got16 = _streamed(e16, c.img, c.flow, c.seg, c.h)
    else:
        got32, got16 = [e32.forward(c.img, c.flow, c.seg, c.wide)], [e16.forward(c.img, c.flow, c.seg, c.h)]
    for a, b in zip(got32, got16):
        assert np.isfinite(a).all() and np.abs(a).max() > 0 and _same(a, b)
        assert_pose_close(b, C.reference_poses(c, None), "source %d re-issued" % source)
    st, st16 = e32.range_stats(), e16.range_stats()
    assert st["reissued"] >= 1 and st["recalibrations"] >= 1, (st, e32.range_report())
    if streamed:      # how many batches were issued before the first verdict arrived depends on the host's timing
        assert st16["reissued"] >= 1 and {k: v for k, v in st16.items() if k != "reissued"} == {k: v for k, v in st.items() if k != "reissued"}, (st16, st)
    else:
        assert st16 == st, (st16, e16.range_report())
    assert e16.activation_range()[1] == e32.activation_range()[1]
    _close(e32, e16)


# ---- exports and the class --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", [12, 13])
def test_exports(source):
    H, W, B = 36, 100, 3
    c = C.case(source, H, W, B)
    want_all = tuple(k for k in Engine.FEATURE_OUTPUTS + Engine.HEAT_OUTPUTS if not (source == 13 and k == "att_19"))
    e32, e16 = _engines(c, H, W, B)
    got = []
    for e, depth in ((e32, c.wide), (e16, c.h)):
        e.set_feature_export(True)
        e.set_heat_export(True)
        r = [e.forward_features(c.img, c.flow, c.seg, depth, want=want_all)]
        e.set_option("host_chunk", 1)                        # sub-batches of one window
        r.append(e.forward_features(c.img, c.flow, c.seg, depth, want=("attention", "masked_image")))
        got.append(r)
    for r32, r16 in zip(*got):
        assert set(r32) == set(r16)
        for k in r32:
            assert _same(r32[k], r16[k]), "source %d: %s differs" % (source, k)
    assert set(got[0][0]) == {"pose"} | set(want_all)
    for r in got[1]:
        assert_pose_close(r["pose"], C.reference_poses(c, None), "source %d export" % source)
    if source == 12:                                         # the rows the export reports, against the float64 tables on the halves' values
        LC.check_table(np.ascontiguousarray(got[1][0]["att_19"].transpose(1, 0, 2)), C.reference_tables(c), [0, 1, 2], "source 12 att_19")
    if source == 13:                                         # the select's map against the restatement: near / far per pixel by the halves' values
        att = C.ref(13).attention(c.cfg, c.flow, c.seg, c.wide, c.weights)
        for frame in range(3):
            assert np.abs(got[1][0]["attention"][frame] - att[frame][..., 0]).max() <= LC.TABLE_TOL
    _close(e32, e16)


def _flat(x, prefix=""):
    if isinstance(x, dict):
        return {k2: v2 for k, v in x.items() for k2, v2 in _flat(v, prefix + k + ".").items()}
    if isinstance(x, (list, tuple)):
        return {k2: v2 for i, v in enumerate(x) for k2, v2 in _flat(v, prefix + "%d." % i).items()}
    return {prefix: x}


@pytest.mark.parametrize("features", ["full", "heat"])
def test_the_reference_call_surface_takes_halves(features):
    H, W, B = 36, 100, 3
    c = C.case(13, H, W, B)
    version = C.VERSIONS[13]
    outs = []
    for fmt, depth in (("f32", c.wide), ("f16", c.h)):
        d = DAVO(version).enable_feature_mode(features=features)
        d.setup_inference(H, W, "davo", 3, B, input_img_uint8=c.img, input_flow=c.flow, input_seglabel=c.seg, input_depth=depth)      # picked up from the dtype
        d.load_weights(c.weights)
        assert d.engine.depth == fmt
        out = d.inference(mode="feature")
        assert _same(d.inference(mode="pose")["pose"], out["pose"])
        assert _same(d.inference(mode="pose", inputs=(c.img, c.flow, c.seg, depth))["pose"], out["pose"])
        it = DAVO(version)
        if fmt == "f16":
            assert it.use_f16_depth() is it
        it.setup_inference(H, W, "davo", 3, B, input_img_uint8=iter([(c.img, c.flow, c.seg, depth)] * 2))
        it.load_weights(c.weights)
        assert it.engine.depth == fmt
        assert _same(it.inference()["pose"], out["pose"]) and _same(it.inference()["pose"], out["pose"])
        it.engine.close()
        outs.append(out)
        d.engine.close()
    want, got = _flat(outs[0]), _flat(outs[1])
    assert set(got) == set(want) and len(want) > 6
    for k in want:
        assert _same(np.asarray(got[k]), np.asarray(want[k])), k
    assert_pose_close(outs[1]["pose"], C.reference_poses(c, None), "DAVO, binary16 depth")
    with pytest.raises(Exception, match="before setup_inference"):
        d.use_f16_depth()


# ---- errors -----------------------------------------------------------------------------------------------------------
def test_errors():
    H, W, B = 16, 16, 1
    c = C.case(11, H, W, B)
    e32, e16 = _engines(c, H, W, B)
    L = e32._L
    assert L.davo_set_depth_format(e32._ctx, 2) == -1 and b"DAVO_DEPTH" in L.davo_last_error(e32._ctx)
    assert L.davo_set_depth_format(e32._ctx, -1) == -1
    assert L.davo_set_depth_format(e32._ctx, 1) == 0 and L.davo_get_depth_format(e32._ctx) == 1       # before any input: either way
    assert L.davo_set_depth_format(e32._ctx, 0) == 0 and L.davo_get_depth_format(e32._ctx) == 0
    # independent of the other settings, in any order
    assert L.davo_set_label_format(e32._ctx, 1) == 0 and L.davo_set_depth_format(e32._ctx, 1) == 0 and L.davo_set_flow_format(e32._ctx, 1) == 0
    assert L.davo_set_pairs(e32._ctx, 2) == 0 and L.davo_set_flip(e32._ctx, 1) == 0
    assert (L.davo_get_label_format(e32._ctx), L.davo_get_flow_format(e32._ctx), L.davo_get_depth_format(e32._ctx), L.davo_get_pairs(e32._ctx),
            L.davo_get_flip(e32._ctx)) == (1, 1, 1, 2, 1)
    assert L.davo_set_flip(e32._ctx, 0) == 0 and L.davo_set_depth_format(e32._ctx, 0) == 0 and L.davo_set_flow_format(e32._ctx, 0) == 0
    assert L.davo_set_label_format(e32._ctx, 0) == 0 and L.davo_set_pairs(e32._ctx, 3) == 0
    assert (L.davo_get_label_format(e32._ctx), L.davo_get_flow_format(e32._ctx), L.davo_get_depth_format(e32._ctx)) == (0, 0, 0)
    e32.forward(c.img, c.flow, c.seg, c.wide)
    assert L.davo_set_depth_format(e32._ctx, 1) == -1 and b"before the first call that takes inputs" in L.davo_last_error(e32._ctx)
    assert L.davo_get_depth_format(e32._ctx) == 0
    with pytest.raises(ValueError, match="before the first call"):
        e32.set_depth_format("f16")
    assert e32.depth == "f32"
    e16.forward(c.img, c.flow, c.seg, c.h)
    with pytest.raises(ValueError, match="before the first call"):
        e16.set_depth_format("f32")
    with pytest.raises(ValueError, match="depth"):
        Engine(c.cfg, H, W, B, depth="half")
    # ... and once a streaming slot's staging set exists (a submit built it)
    e = Engine(c.cfg, H, W, B)
    e.load_weights(c.weights)
    out = np.empty((B, 2, 6), np.float32)
    e.submit(c.img, c.flow, c.seg, out, depth=c.wide)
    e.wait(0)
    assert L.davo_set_depth_format(e._ctx, 1) == -1 and b"staging sets" in L.davo_last_error(e._ctx)
    assert L.davo_get_depth_format(e._ctx) == 0
    e.close()
    # a context whose variant reads no depth accepts the call and still ignores every depth pointer
    from davo_amd import FLAGSHIP_VERSION, parse_version
    fcfg = parse_version(FLAGSHIP_VERSION)
    fw = synth.make_weights(fcfg)
    plain, half = Engine(fcfg, H, W, B), Engine(fcfg, H, W, B, depth="f16")
    for e in (plain, half):
        e.load_weights(fw)
    assert half._L.davo_get_depth_format(half._ctx) == 1
    want = plain.forward(c.img, c.flow, c.seg)
    assert _same(half.forward(c.img, c.flow, c.seg), want) and _same(half.forward(c.img, c.flow, c.seg, c.wide), want)
    pose = np.empty((B, 2, 6), np.float32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    assert half._L.davo_forward_depth(half._ctx, B, vp(c.img), vp(c.flow), vp(c.seg), None, vp(pose)) == 0 and _same(pose, want)
    _close(plain, half)
    # a misaligned device depth pointer
    bufs = [e16.alloc(a.nbytes + 64).upload(a) for a in (c.img, c.flow, c.seg, c.h)]
    d_pose = e16.alloc(B * 12 * 4)
    rc = L.davo_forward_device_depth(e16._ctx, B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, ctypes.c_void_p(bufs[3].ptr.value + 8), d_pose.ptr, None)
    assert rc == -1 and b"16-byte aligned" in L.davo_last_error(e16._ctx)
    assert L.davo_forward_device_depth(e16._ctx, B, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, d_pose.ptr, None) == 0
    e16.synchronize()
    for b in bufs + [d_pose]:
        b.free()
    # nothing converts silently, in either direction, at any entry point
    out = np.empty((B, 2, 6), np.float32)
    for e, wrong in ((e16, c.wide), (e32, c.h), (e16, c.wide.astype(np.float64))):
        with pytest.raises(ValueError, match="depth"):
            e.forward(c.img, c.flow, c.seg, wrong)
        with pytest.raises(ValueError, match="depth"):
            e.submit(c.img, c.flow, c.seg, out, depth=wrong)
        with pytest.raises(ValueError, match="depth"):
            e.calibrate(c.img, c.flow, c.seg, wrong)
        with pytest.raises(ValueError, match="depth"):
            e.forward_features(c.img, c.flow, c.seg, wrong)
        with pytest.raises(ValueError, match="depth"):
            e.forward_frames(*(synth.make_frames(B + 2, H, W)[:3] + (np.zeros((B + 2, H, W, 1), wrong.dtype),)))
    with pytest.raises(ValueError, match="float16 depth array"):      # the hold > 0 contiguity rule, for the format's dtype
        e16.submit(c.img, c.flow, c.seg, out, hold=1, depth=np.asfortranarray(c.h))
    with pytest.raises(ValueError, match="float16 depth array"):
        e16.submit(c.img, c.flow, c.seg, out, hold=1, depth=c.wide)
    with pytest.raises(ValueError, match="float32 depth array"):
        e32.submit(c.img, c.flow, c.seg, out, hold=1, depth=c.h)
    bufs = [e32.alloc(a.nbytes).upload(a) for a in (c.img, c.flow, c.seg, c.h)]
    with pytest.raises(ValueError, match="depth"):
        e32.forward_device(B, bufs[0], bufs[1], bufs[2], bufs[0], depth=bufs[3])
    for b in bufs:
        b.free()
    assert e32.pending() == 0 and e16.pending() == 0
    _close(e32, e16)


# ---- memory -----------------------------------------------------------------------------------------------------------
def _use_everything(e, X, fr, slots):
    """staging sets of every slot, the snapshot ring (the first ticketed submit builds it), the frame buffers, davo_forward's set"""
    e.set_inflight(slots)
    outs = [np.empty((X[0].shape[0], 2, 6), np.float32) for _ in range(2 * slots)]
    for out in outs[:slots]:
        e.submit(X[0], X[1], X[2], out, hold=8, depth=X[3])
    for out in outs[slots:]:
        e.submit_frames(fr[0], fr[1], fr[2], out, hold=8, depth=fr[3])
    e.wait(0)
    e.synchronize()
    e.forward(*X)


def _held_by_format(H, W, B, slots, cycles=3):
    """device memory a context of each depth format and max_batch B holds after it has built everything sized by a depth plane
    (every buffer is sized by max_batch, so one window per call builds them all); checks that nothing is left behind after
    davo_destroy, over several create / destroy cycles"""
    c = C.case(11, H, W, 1)
    X16, X32 = (c.img, c.flow, c.seg, c.h), (c.img, c.flow, c.seg, c.wide)
    fr16 = synth.make_frames(3, H, W, depth="f16")
    fr32 = fr16[:3] + (depth_from_f16(fr16[3]),)
    free = []
    for _ in range(cycles):
        e = Engine(c.cfg, H, W, B, depth="f16")
        e.load_weights(c.weights)
        _use_everything(e, X16, fr16, slots)
        e.close()
        free.append(hip_free_bytes())
    assert len(set(free)) == 1, free                         # create / use / close: back to the baseline, nothing left behind
    held = {}
    for fmt, X, fr in (("f32", X32, fr32), ("f16", X16, fr16), ("f32 again", X32, fr32)):
        e = Engine(c.cfg, H, W, B, depth=fmt[:3])
        e.load_weights(c.weights)
        _use_everything(e, X, fr, slots)
        held[fmt] = free[0] - hip_free_bytes()
        e.close()
    assert hip_free_bytes() == free[0]
    assert held["f32 again"] == held["f32"]
    return held


def test_device_memory():
    # plane_bytes: a window's depth block is 3 H W x 4 bytes as float32 and half that as binary16: 6 H W bytes saved per window of
    # max_batch in every streaming slot's staging set, in davo_forward's set and in each of the range guard's eight snapshots; a
    # slot's frame buffer holds max_batch + 2 planes of H W elements: 2 H W (max_batch + 2) bytes saved per slot.
    # The allocation-granule method of tests/test_f16_flow_gpu.py: at 128x512 and max_batch 16 a staging set's depth buffer is
    # 12 MiB as float32 and 6 MiB as binary16 - whole 2 MiB granules in both formats - and every other buffer of those sets is the
    # same in both contexts, so their part of the difference is exact.  A frame buffer's depth planes are 4.5 MiB / 2.25 MiB, no
    # whole number of granules: within one granule per buffer.
    H, W, B, slots = 128, 512, 16, 2
    nbuf = slots + 1 + 8
    held = _held_by_format(H, W, B, slots)
    saved = held["f32"] - held["f16"]
    sets, frames = 6 * H * W * B * nbuf, 2 * H * W * (B + 2) * slots
    print("device memory held at %dx%d B=%d: float32 depth %d B, binary16 depth %d B, saved %d B (plane_bytes says %d B in %d staging "
          "sets and snapshots + %d B in %d frame buffers)" % (H, W, B, held["f32"], held["f16"], saved, sets, nbuf, frames, slots))
    assert sets == nbuf * (6 << 20)
    assert held["f16"] <= held["f32"]
    assert sets <= saved <= sets + frames + slots * (2 << 20)      # at least the staging sets' depth halves, exactly; the frame buffers by granules
    # a small context over more cycles: never above the float32 context's, nothing left behind
    held = _held_by_format(36, 100, 3, 4, cycles=5)
    assert held["f16"] <= held["f32"]


# ---- launches ---------------------------------------------------------------------------------------------------------
def _launches(e, call):
    e.profile(1)
    e.profile_reset()
    call()
    e.synchronize()
    out = {k: n for k, (n, _) in e.profile_entries().items() if n > 0}
    e.profile(0)
    return out


@pytest.mark.parametrize("source", [11, 13])
def test_launch_counts(source):
    """no launch more than the float32 context's, in any layout, flip off and on"""
    H, W, B = 36, 100, 3
    c = C.case(source, H, W, B)
    e32, e16 = _engines(c, H, W, B)
    X32, X16 = (c.img, c.flow, c.seg, c.wide), (c.img, c.flow, c.seg, c.h)
    fr16 = synth.make_frames(B + 2, H, W, depth="f16")
    fr32 = fr16[:3] + (depth_from_f16(fr16[3]),)
    for flip in (False, True):
        for e in (e32, e16):
            e.set_flip(flip)
        calls = ((lambda e, X, fr: e.forward(*X)), (lambda e, X, fr: _device_forward(e, B, *X)), (lambda e, X, fr: _streamed(e, *X, n=1)),
                 (lambda e, X, fr: e.forward_frames(*fr)), (lambda e, X, fr: _device_frames(e, B, fr)),
                 (lambda e, X, fr: _streamed(e, *fr, n=1, frames=True)))
        for i, call in enumerate(calls):
            a, b = _launches(e32, lambda: call(e32, X32, fr32)), _launches(e16, lambda: call(e16, X16, fr16))
            assert a == b and sum(a.values()) > 0, (source, flip, i, a, b)
    _close(e32, e16)


# ---- the driver -------------------------------------------------------------------------------------------------------
def test_the_driver_writes_the_same_files(tmp_path):
    """run_kitti_pose --depth f16 on a float16 dump and on a float32 dump against --depth f32 on the widened dump: the
    byte-identical trajectory file.  run_kitti_pose.main is what `python -m davo_amd.run_kitti_pose' runs; called in this process
    so that the launches cost no interpreter and HIP start-ups of their own."""
    from davo_amd import loader as L, run_kitti_pose as R
    H, W, frames = 36, 100, {3: 7}
    version = C.VERSIONS[13]
    dumps = {"widened": str(tmp_path / "widened"), "f16": str(tmp_path / "f16"), "f32": str(tmp_path / "f32")}
    for fmt, d in dumps.items():
        for seq, n in frames.items():
            L.write_synthetic_dump(d, seq, n, H, W, seed=40 + seq, depth=True if fmt == "f32" else fmt)
    ckpt = str(tmp_path / "w.npz")
    np.savez(ckpt, **synth.make_weights(version))
    files = []
    for dump, depth in (("widened", "f32"), ("f16", "f16"), ("f32", "f16")):      # f32 dump, --depth f16: rounded by the loader's workers
        out = tmp_path / ("out_%s_%s" % (dump, depth))
        args = ["--test_seq", "3", "--concat_img_dir", dumps[dump], "--ckpt_file", ckpt, "--output_dir", str(out), "--img_height", str(H),
                "--img_width", str(W), "--batch_size", "2", "--loader_procs", "2", "--version", version, "--depth", depth]
        try:
            R.main(args)
        except Exception:
            import traceback
            pytest.fail("run_kitti_pose %s failed:\n%s" % (" ".join(args), traceback.format_exc()), pytrace=False)
        files.append([open(str(out / ("%.2d-pred_kitti_pose.txt" % seq)), "rb").read() for seq in frames])
    assert all(len(f) > 0 for f in files[0])
    assert files[1] == files[0], "float16 dump, --depth f16"
    assert files[2] == files[0], "float32 dump, --depth f16"
