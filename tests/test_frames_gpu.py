"""The frame layout on the GPU (include/davo_hip.h "Frame sequences"; csrc/window_gather.h).

The reference in every test is the window entry point on davo_amd.windows_from_frames of the same arrays, issued with the same
batch size, and every comparison is bit for bit: a window gathered on the device is byte for byte the window the caller would
have built, and the window path is already pinned layer by layer to the float64 restatement.

Shapes - the smallest that reach every path of the gather: 16x16 (48-byte row pieces: the 16-byte path), 16x20 (60-byte
pieces: dwords only), 32x48; N = 1, 2, 5 with max_batch 5.  synth.make_frames' frames differ from each other in every plane, so
a swapped index cannot pass."""
import ctypes

import numpy as np
import pytest

import davo_amd
from davo_amd import Engine, FLAGSHIP_VERSION, parse_version, synth
from davo_amd import sequence as S
from davo_amd.frames import frames_plan

from helpers import hip_free_bytes
from test_stream import _rescaled

pytestmark = pytest.mark.gpu

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"
VARIANTS = {"flagship": FLAGSHIP_VERSION,
            "se_rgb_to_seg": BASE + "-segmask_all-se_rgb_to_seg-fc_tanh",                      # a class-table source that attends the target
            "se_depth_to_seg": BASE + "-segmask_all-se_depth_to_seg-fc_tanh",                  # a depth source
            "depthseg_seplayers": BASE + "-segmask_all-se_flow_on_depthseg_seplayers-abs_flow-fc_tanh"}
SHAPES = [(16, 16), (16, 20), (32, 48)]
BATCHES = [1, 2, 5]
MAXB = 5
_WEIGHTS = {}


def _weights(cfg):
    if cfg.version not in _WEIGHTS:
        _WEIGHTS[cfg.version] = synth.make_weights(cfg)
    return _WEIGHTS[cfg.version]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _engine(cfg, H, W, max_batch=MAXB, labels="f32", precision="f16x3", weights=None):
    e = Engine(cfg, H, W, max_batch, labels=labels)
    e.load_weights(_weights(cfg) if weights is None else weights)
    e.set_precision(precision)
    return e


def _frames(cfg, N, H, W, labels="f32", seed=synth.SEED):
    """-> (frame-layout arrays, window-layout arrays), depth last in both where the variant reads it"""
    fr = synth.make_frames(N + 2, H, W, seed=seed, depth=cfg.needs_depth, labels=labels)
    return fr, davo_amd.windows_from_frames(*fr)


def _device_run(e, cfg, N, parts, frames):
    """one device-path batch -> {pose, packed, att_table[, att_table_far]}"""
    H, W = e.H, e.W
    bufs = [e.alloc(a.nbytes).upload(a) for a in parts]
    pose = e.alloc(N * 12 * 4)
    depth = {"depth": bufs[3]} if cfg.needs_depth else {}
    if frames:
        e.forward_device_frames(N, bufs[0], bufs[1], bufs[2], pose, **depth)
    else:
        e.forward_device(N, bufs[0], bufs[1], bufs[2], pose, **depth)
    e.synchronize()
    out = {"pose": pose.download((N, 2, 6)), "packed": e.debug_read("packed", (2 * N, H, W, 8)),
           "att_table": e.debug_read("att_table", (N, 3, 19))}
    if cfg.att_source == "se_flow_depthseg_sep":
        out["att_table_far"] = e.debug_read("att_table_far", (N, 3, 19))
    for b in bufs + [pose]:
        b.free()
    return out


# ---- 1. per-pixel mapping ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["f32", "u8"])
@pytest.mark.parametrize("name", list(VARIANTS))
def test_device_frames_land_where_the_windows_hold_them(name, labels):
    cfg = parse_version(VARIANTS[name])
    for H, W in SHAPES:
        e = _engine(cfg, H, W, labels=labels)
        for N in BATCHES:
            fr, win = _frames(cfg, N, H, W, labels, seed=1000 * N + W)       # fresh data per batch: nothing stale can pass
            want = _device_run(e, cfg, N, win, False)
            got = _device_run(e, cfg, N, fr, True)
            assert np.abs(want["pose"]).max() > 0 and np.isfinite(want["packed"]).all()
            for k in want:
                assert _same(got[k], want[k]), "%s %s %dx%d N=%d: %s differs" % (name, labels, H, W, N, k)
        e.close()


# ---- 2. precisions and sub-batches ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("name", ["flagship", "se_depth_to_seg"])
def test_forward_frames_is_forward_to_the_bit(name, precision):
    cfg = parse_version(VARIANTS[name])
    for H, W in SHAPES:
        e = _engine(cfg, H, W, precision=precision)
        for N in BATCHES:
            fr, win = _frames(cfg, N, H, W, seed=77 * N + H)
            assert _same(e.forward_frames(*fr), e.forward(*win)), (name, precision, H, W, N)
        # sub-batches of 2, 2, 1: windows [b0, b0 + nb) take frames [b0, b0 + nb + 2)
        fr, win = _frames(cfg, 5, H, W, seed=5)
        whole = e.forward(*win)
        e.set_option("host_chunk", 2)
        assert _same(e.forward_frames(*fr), e.forward(*win))
        assert _same(e.forward_frames(*fr), whole)
        e.close()


# ---- 3. streaming --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", ["f32", "u8"])
@pytest.mark.parametrize("inflight", [1, 4])
def test_submit_frames_is_submit_to_the_bit(inflight, labels):
    """Nine batches of fresh arrays, hold = 0, ONE set of host arrays overwritten right after every call"""
    cfg = parse_version(VARIANTS["se_depth_to_seg"])
    H, W, n = 16, 20, 9
    data = [_frames(cfg, (5, 1, 2)[k % 3], H, W, labels, seed=300 + k) for k in range(n)]
    e = _engine(cfg, H, W, labels=labels)
    e.set_inflight(inflight)
    want = [np.full((d[1][0].shape[0], 2, 6), np.nan, np.float32) for d in data]
    for k, (_, win) in enumerate(data):
        e.submit(*win[:3], want[k], depth=win[3])
    e.synchronize()
    got = [np.full_like(w, np.nan) for w in want]
    bufs = [np.empty((MAXB + 2,) + a.shape[1:], a.dtype) for a in data[0][0]]
    for k, (fr, _) in enumerate(data):
        N = fr[1].shape[0]
        views = [buf[:len(a)] for buf, a in zip(bufs, fr)]
        for v, a in zip(views, fr):
            v[...] = a
        e.submit_frames(*views[:3], got[k], depth=views[3])
        for buf in bufs:
            buf[...] = 255 if buf.dtype == np.uint8 else np.nan      # consumed: the caller may do anything to them now
        assert N == got[k].shape[0]
    assert 0 < e.pending() <= 8
    e.synchronize()
    assert e.pending() == 0
    for k in range(n):
        assert not np.isnan(want[k]).any() and _same(got[k], want[k]), (k, inflight, labels)
    # one stream of window and frame batches interleaved
    mixed = [np.full_like(w, np.nan) for w in want]
    for k, (fr, win) in enumerate(data):
        if k % 2:
            e.submit(*win[:3], mixed[k], depth=win[3])
        else:
            e.submit_frames(*fr[:3], mixed[k], depth=fr[3])
    e.wait()
    for k in range(n):
        assert _same(mixed[k], want[k]), (k, "interleaved")
    e.close()


@pytest.mark.parametrize("name,labels", [("flagship", "f32"), ("se_depth_to_seg", "u8")])
def test_layouts_interleaved_among_busy_slots(name, labels):
    """Twelve submits on four slots, hold = 0, window and frame layout alternating, batches of 5, 1, 2 of fresh arrays, and one
    forward_frames after the sixth (it delivers what is pending first): a staging set, a frame buffer and a pose ring entry are
    reused across the layouts while other slots are busy.  Every delivered batch is, to the bit, forward() on the windows of
    the same arrays on a second, fresh engine."""
    cfg = parse_version(VARIANTS[name])
    H, W, n = 16, 20, 12
    data = [_frames(cfg, (5, 1, 2)[k % 3], H, W, labels, seed=500 + k) for k in range(n + 1)]      # [n]: the forward_frames call's
    depth = (lambda parts: {"depth": parts[3]}) if cfg.needs_depth else (lambda parts: {})
    e = _engine(cfg, H, W, labels=labels)
    e.set_inflight(4)
    got = [np.full((d[0][1].shape[0], 2, 6), np.nan, np.float32) for d in data]
    for k in range(n):
        fr, win = data[k]
        if k % 2:
            e.submit_frames(*fr[:3], got[k], **depth(fr))
        else:
            e.submit(*win[:3], got[k], **depth(win))
        if k == 5:
            assert e.pending() > 0
            got[n] = e.forward_frames(*data[n][0][:3], **depth(data[n][0]))
            assert e.pending() == 0 and not any(np.isnan(g).any() for g in got[:6])
    e.wait()
    assert e.pending() == 0
    e.close()
    ref = _engine(cfg, H, W, labels=labels)
    for k, (_, win) in enumerate(data):
        want = ref.forward(*win[:3], **depth(win))
        assert np.abs(want).max() > 0 and _same(got[k], want), (name, labels, k)
    ref.close()


# ---- 4. one pair -----------------------------------------------------------------------------------------------------------
def _poisoned(fr, plan, labels):
    """the frame arrays with everything outside the selection's ranges overwritten: 0xFF bytes, NaN floats"""
    frames, flow2, seg = (a.copy() for a in fr[:3])
    keep = np.zeros(len(frames), bool)
    keep[plan["frames"][0]:plan["frames"][1]] = True
    frames[~keep] = 0xFF
    for p in range(2):
        if not plan["flow"][0] <= p < plan["flow"][1]:
            flow2[:, p] = np.nan
    keep[:] = False
    keep[plan["seg"][0]:plan["seg"][1]] = True
    seg[~keep] = 0xFF if labels == "u8" else np.nan
    out = (frames, flow2, seg)
    if len(fr) == 4:
        depth = fr[3].copy()
        keep[:] = False
        keep[plan["depth"][0]:plan["depth"][1]] = True
        depth[~keep] = np.nan
        out += (depth,)
    return out


@pytest.mark.parametrize("pairs", ["src0", "src1"])
@pytest.mark.parametrize("name,labels", [("flagship", "f32"), ("se_rgb_to_seg", "u8"), ("se_depth_to_seg", "f32"), ("depthseg_seplayers", "u8")])
def test_one_pair_copies_and_reads_only_its_frames(name, labels, pairs):
    cfg = parse_version(VARIANTS[name])
    for (H, W), N in zip(SHAPES, (5, 2, 1)):
        e = _engine(cfg, H, W, labels=labels)
        e.set_pairs(pairs)
        fr, win = _frames(cfg, N, H, W, labels, seed=41 + N)
        want = e.forward(*win)
        row, other = (0, 1) if pairs == "src0" else (1, 0)
        assert np.abs(want[:, row]).max() > 0 and not _bits(want[:, other]).any()       # +0.0, not -0.0
        bad = _poisoned(fr, frames_plan(H, W, N, pairs, cfg.att_source, labels), labels)
        assert any(not np.array_equal(a, b, equal_nan=False) for a, b in zip(bad, fr))
        depth = {"depth": bad[3]} if cfg.needs_depth else {}
        assert _same(e.forward_frames(*bad[:3], **depth), want), (name, pairs, H, W, "forward_frames")
        out = np.full((N, 2, 6), np.nan, np.float32)
        e.submit_frames(*bad[:3], out, **depth)
        e.synchronize()
        assert _same(out, want), (name, pairs, H, W, "submit_frames")
        got = _device_run_pose(e, cfg, N, bad)
        assert _same(got, want), (name, pairs, H, W, "forward_device_frames")
        e.close()


def _device_run_pose(e, cfg, N, parts):
    bufs = [e.alloc(a.nbytes).upload(a) for a in parts]
    pose = e.alloc(N * 12 * 4)
    e.forward_device_frames(N, bufs[0], bufs[1], bufs[2], pose, **({"depth": bufs[3]} if cfg.needs_depth else {}))
    e.synchronize()
    out = pose.download((N, 2, 6))
    for b in bufs + [pose]:
        b.free()
    return out


# ---- 5. range guard --------------------------------------------------------------------------------------------------------
def test_a_guard_tripping_checkpoint_is_reissued_from_the_gathered_copy():
    """tests/test_stream.py's checkpoint (cnv3's activations leave the fp16-pair range) through submit_frames with ONE recycled
    set of host arrays: the re-issue reads the library's snapshot of the gathered windows.  Two engines with the same history,
    one fed windows and one fed frames, deliver the same bits."""
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, N, n = 64, 96, 2, 6
    weights = _rescaled(_weights(cfg), 16)
    data = [_frames(cfg, N, H, W, seed=900 + k) for k in range(n)]
    outs = {}
    for layout in ("windows", "frames"):
        e = _engine(cfg, H, W, N, weights=weights)
        e.set_inflight(2)
        outs[layout] = [np.full((N, 2, 6), np.nan, np.float32) for _ in range(n)]
        bufs = [np.empty_like(a) for a in data[0][layout == "windows"]]
        for k in range(n):
            for buf, a in zip(bufs, data[k][layout == "windows"]):
                buf[...] = a
            (e.submit if layout == "windows" else e.submit_frames)(*bufs, outs[layout][k])
            for buf in bufs:
                buf[...] = 255 if buf.dtype == np.uint8 else np.nan
        e.synchronize()
        stats = e.range_stats()
        assert stats["reissued"] > 0 and stats["f32_batches"] == 0, (layout, stats)
        e.close()
    for k in range(n):
        assert np.isfinite(outs["windows"][k]).all() and _same(outs["frames"][k], outs["windows"][k]), k


# ---- 6. error codes --------------------------------------------------------------------------------------------------------
def test_error_codes():
    H, W = 16, 16
    vp = ctypes.c_void_p
    for name in ("flagship", "se_depth_to_seg"):
        cfg = parse_version(VARIANTS[name])
        e = _engine(cfg, H, W)
        L, ctx = e._L, e._ctx
        fr, _ = _frames(cfg, MAXB, H, W)
        p = [a.ctypes.data_as(vp) for a in fr] + ([None] if len(fr) == 3 else [])
        out = np.zeros((MAXB + 1, 2, 6), np.float32)
        o = out.ctypes.data_as(vp)
        dbufs = [e.alloc(a.nbytes).upload(a) for a in fr]
        d = [b.ptr for b in dbufs] + ([None] if len(fr) == 3 else [])
        dpose = e.alloc(out.nbytes)
        calls = {"forward": lambda N, q, po: L.davo_forward_frames(ctx, N, q[0], q[1], q[2], q[3], po),
                 "submit": lambda N, q, po: L.davo_submit_frames(ctx, N, q[0], q[1], q[2], q[3], po, 0),
                 "device": lambda N, q, po: L.davo_forward_device_frames(ctx, N, q[0], q[1], q[2], q[3], po, None)}
        for fn, call in calls.items():
            args, po = (d, dpose.ptr) if fn == "device" else (p, o)
            for N in (0, -1, MAXB + 1):
                assert call(N, args, po) == -1, (name, fn, N)
                assert b"batch" in L.davo_last_error(ctx)
            for k in range(3):
                q = list(args)
                q[k] = None
                assert call(2, q, po) == -1 and b"null" in L.davo_last_error(ctx), (name, fn, k)
            assert call(2, args, None) == -1
            if cfg.needs_depth:                              # depth missing on a depth variant: refused, and the message says why
                q = list(args)
                q[3] = None
                assert call(2, q, po) == -1, (name, fn)
                msg = L.davo_last_error(ctx).decode()
                assert "depth" in msg and "NULL" in msg, msg
        assert L.davo_submit_frames(ctx, 2, p[0], p[1], p[2], p[3], o, -1) == -1
        q = list(d)
        q[0] = vp(d[0].value + 4)                           # device pointers are 16-byte aligned
        assert calls["device"](2, q, dpose.ptr) == -1 and b"aligned" in L.davo_last_error(ctx)
        assert e.pending() == 0
        # the context is as usable as before
        want = e.forward(*davo_amd.windows_from_frames(*fr))
        assert _same(e.forward_frames(*fr), want)
        for b in dbufs + [dpose]:
            b.free()
        # the Python layer: wrong label dtype is a ValueError, nothing converts silently
        with pytest.raises(ValueError):
            e.forward_frames(fr[0], fr[1], davo_amd.labels_to_u8(fr[2]), *fr[3:])
        with pytest.raises(ValueError):
            e.forward_frames(fr[0][:-1], *fr[1:])
        with pytest.raises(ValueError):
            e.submit_frames(*fr[:3], np.empty((MAXB, 2, 6), np.float64), **({"depth": fr[3]} if cfg.needs_depth else {}))
        if cfg.needs_depth:
            with pytest.raises(ValueError):
                e.forward_frames(*fr[:3])
        e.close()


# ---- 7. the window path is unchanged ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_window_calls_after_frame_calls_are_a_fresh_contexts(precision):
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, N = 32, 48, 3
    fr, _ = _frames(cfg, N, H, W, seed=1)
    _, win = _frames(cfg, N, H, W, seed=2)

    def window_calls(e):
        out = np.full((N, 2, 6), np.nan, np.float32)
        e.submit(*win, out)
        e.synchronize()
        dev = _device_run(e, cfg, N, win, False)
        return [e.forward(*win), out, dev["pose"], dev["packed"], dev["att_table"]]

    a = _engine(cfg, H, W, precision=precision)
    a.set_inflight(2)
    a.forward_frames(*fr)
    outs = [np.empty((N, 2, 6), np.float32) for _ in range(3)]
    for out in outs:
        a.submit_frames(*fr, out)
    _device_run(a, cfg, N, fr, True)
    got = window_calls(a)
    a.close()
    b = _engine(cfg, H, W, precision=precision)
    b.set_inflight(2)
    want = window_calls(b)
    b.close()
    for k, (x, y) in enumerate(zip(got, want)):
        assert _same(x, y), k


# ---- 8. device memory ------------------------------------------------------------------------------------------------------
def _all_entry_points(e, cfg, fr, win, slots, layout):
    N = fr[1].shape[0]
    outs = [np.empty((N, 2, 6), np.float32) for _ in range(slots)]
    if layout == "windows":
        e.forward(*win)
        for out in outs:
            e.submit(*win, out)
        e.wait()
        for _ in range(slots):
            _device_run(e, cfg, N, win, False)
    else:
        e.forward_frames(*fr)
        for out in outs:
            e.submit_frames(*fr, out)
        e.wait()
        for _ in range(slots):
            _device_run(e, cfg, N, fr, True)


def test_device_memory():
    """max_batch 16 at 128x416 so that every frame buffer plane is more than one 2 MiB granule of the allocator (18 frames:
    2.9 MB of pixels, 3.8 MB of float32 label maps); the batches themselves are one window."""
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, B, slots = 128, 416, 16, 4
    fr, win = _frames(cfg, 1, H, W)
    e = _engine(cfg, H, W, B)
    e.set_inflight(slots)
    _all_entry_points(e, cfg, fr, win, slots, "windows")      # everything window work builds lazily exists now
    before = hip_free_bytes()
    _all_entry_points(e, cfg, fr, win, slots, "windows")
    assert hip_free_bytes() == before                        # window-only work: nothing new
    out = np.empty((1, 2, 6), np.float32)
    e.submit_frames(*fr, out)
    e.synchronize()
    first = hip_free_bytes()
    assert before - first >= 2 << 20, (before, first)        # the first `_frames' call: its slot's frame buffer
    _all_entry_points(e, cfg, fr, win, slots, "frames")
    held = hip_free_bytes()
    assert held < first                                      # the other slots' frame buffers
    _all_entry_points(e, cfg, fr, win, slots, "frames")
    assert hip_free_bytes() == held                          # built once
    e.close()
    free = []
    for _ in range(3):                                       # whole lifetimes: all three entry points on four slots leave nothing behind
        e = _engine(cfg, H, W, B)
        e.set_inflight(slots)
        _all_entry_points(e, cfg, fr, win, slots, "frames")
        e.close()
        free.append(hip_free_bytes())
    assert free[2] == free[1] == free[0], free
    # a context that only ever ran the device entry point built staging sets, and they went with it too
    e = _engine(cfg, H, W, B)
    _device_run(e, cfg, 1, fr, True)
    e.close()
    assert hip_free_bytes() == free[0]


# ---- 9. the sequence driver -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pairs", ["both", "trajectory"])
def test_run_frames_against_window_calls_on_the_same_partition(pairs):
    cfg = parse_version(VARIANTS["se_depth_to_seg"])
    H, W, n_frames, B = 16, 20, 13, 4
    seq = synth.make_frames(n_frames, H, W, depth=True)

    def load(lo, hi):
        return tuple(np.ascontiguousarray(a[lo:hi] if k == 1 else a[lo:hi + 2]) for k, a in enumerate(seq))

    e = _engine(cfg, H, W, B)
    want = np.zeros((n_frames - 2, 2, 6), np.float32)
    for lo in (0, 4, 8):                                     # 4, 4, 3
        hi = min(lo + B, n_frames - 2)
        e.set_pairs(S.batch_pairs(pairs, lo) or "both")
        want[lo:hi] = e.forward(*davo_amd.windows_from_frames(*load(lo, hi)))
    e.set_pairs("both")
    traj, poses = S.run_frames(e, load, n_frames, B, pairs=pairs)
    assert _same(poses, want) and np.abs(want[:, 1]).min() > 0
    ref = S.stitch_trajectory(want)
    assert len(traj) == n_frames and all(np.array_equal(a, b) for a, b in zip(traj, ref))
    e.set_pairs("both")
    stream = S.PoseStream(e, inflight=2, hold=0)             # (load's arrays go away with the loop's next round)
    traj, poses = S.run_frames(stream, load, n_frames, B, pairs=pairs)
    assert _same(poses, want) and all(np.array_equal(a, b) for a, b in zip(traj, ref))
    e.close()
