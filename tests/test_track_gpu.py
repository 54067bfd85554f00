"""Online tracking on the GPU (include/davo_hip.h "Online tracking"; csrc/window_gather.h: the ring form of the gather).

The reference in every test is an existing entry point - davo_forward, davo_forward_frames or davo_submit - on the windows
(lane s, frames t - 2 .. t) of push t, built on the host by davo_amd.windows_from_frames, under the same pair selection and with
the same batch size (the lanes), and every comparison is bit for bit.

Shapes: 16x16 (16-byte strip path, less than one cnv1 tile), 36x100 (dword strip path, ragged tiles), 64x64; lanes 1 and 3; eight
pushes a session (a ring of three or four places goes round twice), fourteen where four slots make it six places.
synth.make_frames' frames differ from each other in every plane, and every lane draws from a seed of its own, so a swapped frame,
place or lane cannot pass."""
import ctypes
import os

import numpy as np
import pytest

import davo_amd
from davo_amd import Engine, FLAGSHIP_VERSION, parse_version, synth

from helpers import hip_free_bytes
from test_stream import _rescaled

pytestmark = pytest.mark.gpu

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"
VARIANTS = {"flagship": FLAGSHIP_VERSION,
            "se_rgb_to_seg": BASE + "-segmask_all-se_rgb_to_seg-fc_tanh",                      # attends the target's label map
            "se_depth_to_seg": BASE + "-segmask_all-se_depth_to_seg-fc_tanh",                  # att_source 12: a depth source
            "depthseg_seplayers": BASE + "-segmask_all-se_flow_on_depthseg_seplayers-abs_flow-fc_tanh",      # 13: the depth split
            "se_spp21_flow": BASE + "-segmask_all-se_spp21_flow-abs_flow-fc_tanh",             # a pooled source
            "triplet": FLAGSHIP_VERSION.replace("-sharedNN", ""),                              # the three-frame network
            "coupled": FLAGSHIP_VERSION.replace("dilatedPoseNN", "dilatedCouplePoseNN")}       # the coupled network
SHAPES = [(16, 16), (36, 100), (64, 64)]
PUSHES = 8
_WEIGHTS = {}


def _weights(cfg):
    if cfg.version not in _WEIGHTS:
        _WEIGHTS[cfg.version] = synth.make_weights(cfg)
    return _WEIGHTS[cfg.version]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _engine(cfg, H, W, max_batch=3, precision="f16x3", weights=None, **fmt):
    e = Engine(cfg, H, W, max_batch, **fmt)
    e.load_weights(_weights(cfg) if weights is None else weights)
    e.set_precision(precision)
    return e


class Lanes:
    """S synthetic videos of n frames in the engine's formats: what push t carries, and the window batch it completes"""

    def __init__(self, cfg, S, n, H, W, seed=0, labels="f32", flow="f32", depth="f32"):
        d = ("f16" if depth == "f16" else True) if cfg.needs_depth else False
        self.seqs = [synth.make_frames(n, H, W, seed=synth.SEED + 1000 * seed + 17 * s, depth=d, labels=labels, flow=flow) for s in range(S)]
        self.S, self.n, self.depth = S, n, bool(d)

    def push(self, t):
        """(frames [S,H,W,3], flow2 [S,2,H,W,2] or None, seg [S,H,W,1], depth [S,H,W,1] or None), fresh arrays"""
        per = [davo_amd.track_pushes(*q)[t] for q in self.seqs]
        return tuple(None if per[0][k] is None else np.ascontiguousarray(np.concatenate([p[k] for p in per])) for k in range(4))

    def windows(self, t):
        """the S windows push t completes, window layout: (img, flow, seg[, depth])"""
        per = [davo_amd.windows_from_frames(*(a[t - 2:t - 1] if k == 1 else a[t - 2:t + 1] for k, a in enumerate(q))) for q in self.seqs]
        return tuple(np.ascontiguousarray(np.concatenate([p[k] for p in per])) for k in range(len(per[0])))


def _selection(policy, t, cycle=("both", "src1", "src0")):
    if policy == "trajectory":
        return "both" if t == 2 else "src1"
    return cycle[t % len(cycle)]


def _want(ref, lanes, policy, pushes=PUSHES, triplet=False, flip_from=None):
    """davo_forward on the windows of every push, under the push's selection"""
    out = {}
    for t in range(2, pushes):
        sel = "both" if triplet else _selection(policy, t)
        if ref.pairs != sel:
            ref.set_pairs(sel)
        if flip_from is not None:
            ref.set_flip(t >= flip_from)
        out[t] = ref.forward(*lanes.windows(t))
    return out


def _track(e, lanes, policy, pushes=PUSHES, hold=0, triplet=False, flip_from=None, scribble=True, between=None):
    """a session of `pushes' pushes -> {t: poses}; with hold = 0 the caller's arrays are overwritten right after each push"""
    e.track_begin(lanes.S, policy)
    got = {}
    kept = []
    for t in range(pushes):
        if policy == "as_set" and t >= 2 and not triplet:
            e.set_pairs(_selection(policy, t))
        if flip_from is not None:
            e.set_flip(t >= flip_from)
        p = lanes.push(t)
        out = np.full((lanes.S, 2, 6), np.nan, np.float32)
        n = e.track_push(p[0], p[1], p[2], out, hold, depth=p[3])
        assert n == (lanes.S if t >= 2 else 0) and e.track_frames() == t + 1
        if t >= 2:
            got[t] = out
        if scribble and hold == 0:
            for a in p:
                if a is not None:
                    a[...] = 255 if a.dtype == np.uint8 else np.nan
        kept.append(p)
        if between is not None:
            between(t)
    e.wait()
    assert e.pending() == 0
    e.track_end()
    return got


def _check(got, want, what):
    assert sorted(got) == sorted(want)
    for t in want:
        assert np.isfinite(want[t]).all() and np.abs(want[t]).max() > 0
        assert _same(got[t], want[t]), "%s: push %d differs" % (what, t)


# ---- 1. flagship, both precisions, both policies ------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["trajectory", "as_set"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_pushes_are_the_offline_windows_to_the_bit(precision, policy):
    cfg = parse_version(FLAGSHIP_VERSION)
    for (H, W), S in zip(SHAPES + SHAPES[:1], (1, 3, 1, 3)):
        lanes = Lanes(cfg, S, PUSHES, H, W, seed=H + S)
        ref, e = _engine(cfg, H, W, precision=precision), _engine(cfg, H, W, precision=precision)
        want = _want(ref, lanes, policy)
        got = _track(e, lanes, policy)
        _check(got, want, "%s %s %dx%d S=%d" % (precision, policy, H, W, S))
        if policy == "trajectory":                           # row 0 is +0.0 from the second window on; the first window has both
            assert _bits(got[2][:, 0]).any()
            for t in range(3, PUSHES):
                assert not _bits(got[t][:, 0]).any() and _bits(got[t][:, 1]).all()
        # the packed tensor of the last push is the offline call's (want[PUSHES - 1] was ref's last forward)
        images = S * (2 if _selection(policy, PUSHES - 1) == "both" else 1)
        assert _same(e.debug_read("packed", (images, H, W, 8)), ref.debug_read("packed", (images, H, W, 8)))
        ref.close()
        e.close()


# ---- 2. formats -------------------------------------------------------------------------------------------------------------
def test_byte_labels_and_binary16_flow():
    cfg = parse_version(VARIANTS["se_rgb_to_seg"])
    fmt = dict(labels="u8", flow="f16")
    for (H, W), S in zip(SHAPES, (3, 1, 3)):
        lanes = Lanes(cfg, S, PUSHES, H, W, seed=3, **fmt)
        ref, e = _engine(cfg, H, W, **fmt), _engine(cfg, H, W, **fmt)
        _check(_track(e, lanes, "trajectory"), _want(ref, lanes, "trajectory"), "u8/f16 %dx%d S=%d" % (H, W, S))
        ref.close()
        e.close()


# ---- 3. depth ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se_depth_to_seg", "depthseg_seplayers"])
def test_depth_variants_with_binary16_depth_and_poison_where_nothing_reads(name):
    """Under the trajectory policy a push from the second window on reads neither the flow plane tgt->src0 nor anything of the
    oldest ring place (src0's frame, label map and depth plane): NaN in the one and 0xFF bytes - NaN as float32 and binary16 -
    in the other change no bit."""
    cfg = parse_version(VARIANTS[name])
    for (H, W), S in zip(SHAPES, (1, 3, 1)):
        lanes = Lanes(cfg, S, PUSHES, H, W, seed=11, depth="f16")
        ref, e = _engine(cfg, H, W, depth="f16"), _engine(cfg, H, W, depth="f16")
        want = _want(ref, lanes, "trajectory")
        _check(_track(e, lanes, "trajectory"), want, "%s %dx%d S=%d" % (name, H, W, S))
        e.track_begin(S, "trajectory")
        got = {}
        for t in range(PUSHES):
            p = list(lanes.push(t))
            if t >= 3:
                p[1][:, 0] = np.nan
                assert e._L.davo_track_debug_fill(e._ctx, e_ring(e, t)["read"][0], 0xFF) == 0
            got[t] = np.full((S, 2, 6), np.nan, np.float32)
            e.track_push(p[0], p[1], p[2], got[t], depth=p[3])
        e.wait()
        e.track_end()
        del got[0], got[1]
        _check(got, want, "%s %dx%d S=%d poisoned" % (name, H, W, S))
        ref.close()
        e.close()


def e_ring(e, t, inflight=1):
    return davo_amd.track_ring(inflight, t)


# ---- 4. attention sources and topologies ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["se_rgb_to_seg", "se_spp21_flow", "triplet", "coupled"])
@pytest.mark.parametrize("policy", ["trajectory", "as_set"])
def test_sources_and_topologies(name, policy):
    cfg = parse_version(VARIANTS[name])
    tri = name == "triplet"
    for (H, W), S in zip(SHAPES[1:], (3, 1)):
        lanes = Lanes(cfg, S, PUSHES, H, W, seed=5)
        ref, e = _engine(cfg, H, W), _engine(cfg, H, W)
        want = _want(ref, lanes, policy, triplet=tri)
        got = _track(e, lanes, policy, triplet=tri)
        _check(got, want, "%s %s %dx%d S=%d" % (name, policy, H, W, S))
        if tri:                                              # whole windows under either policy
            assert all(_bits(got[t][:, 0]).any() for t in got)
        ref.close()
        e.close()


# ---- 5. flip ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip_from", [0, 4])
def test_flip_inside_the_gather(flip_from):
    """flip on from the start, and toggled at push 4 (the ring holds frames as pushed: the pushes before are not mirrored, the
    pushes after are, and the frames pushed before the toggle are mirrored when a later window reads them)"""
    cfg = parse_version(VARIANTS["se_depth_to_seg"])
    for (H, W), S in zip(SHAPES, (3, 3, 1)):
        lanes = Lanes(cfg, S, PUSHES, H, W, seed=9, labels="u8")
        ref, e = _engine(cfg, H, W, labels="u8"), _engine(cfg, H, W, labels="u8")
        want = _want(ref, lanes, "trajectory", flip_from=flip_from)
        off = _want(ref, lanes, "trajectory", flip_from=PUSHES)
        assert not _same(want[PUSHES - 1], off[PUSHES - 1])                        # the mirror matters
        _check(_track(e, lanes, "trajectory", flip_from=flip_from), want, "flip from %d %dx%d S=%d" % (flip_from, H, W, S))
        ref.close()
        e.close()


def test_flip_adds_no_launch():
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, S = 36, 100, 3
    lanes = Lanes(cfg, S, PUSHES, H, W)
    counts = {}
    for flip in (False, True):
        e = _engine(cfg, H, W)
        e.set_flip(flip)
        e.profile(True)
        _track(e, lanes, "trajectory")
        counts[flip] = {k: v[0] for k, v in e.profile_entries().items()}
        e.close()
    assert counts[True] == counts[False], counts
    assert counts[True]["window_gather"] == PUSHES - 2 and "window_mirror" not in counts[True]


# ---- 6. slots and mixed calls -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflight,hold", [(1, 0), (4, 0), (4, 2), (2, 9)])
def test_slots_hold_and_delivery_order(inflight, hold):
    cfg = parse_version(VARIANTS["se_depth_to_seg"])
    H, W, S, n = 36, 100, 3, 14                              # four slots: a ring of six places goes round twice
    lanes = Lanes(cfg, S, n, H, W, seed=inflight)
    ref, e = _engine(cfg, H, W), _engine(cfg, H, W)
    want = _want(ref, lanes, "trajectory", n)
    e.set_inflight(inflight)
    assert davo_amd.track_ring(inflight, 0)["R"] == inflight + 2
    _check(_track(e, lanes, "trajectory", n, hold=hold), want, "inflight %d hold %d" % (inflight, hold))
    # delivery order: the oldest push first
    e.track_begin(S, "trajectory")
    outs = []
    for t in range(6):
        p = lanes.push(t)
        outs.append(np.full((S, 2, 6), np.nan, np.float32))
        e.track_push(p[0], p[1], p[2], outs[t], hold, depth=p[3])
    e.wait(2)
    assert e.pending() <= 2 and not np.isnan(outs[2]).any() and not np.isnan(outs[3]).any()
    e.wait()
    for t in range(2, 6):
        assert _same(outs[t], want[t]), t
    # refused while the session is open, with a message; the session goes on
    with pytest.raises(ValueError, match="tracking session"):
        e.set_inflight(2)
    e.track_end()
    ref.close()
    e.close()


def test_other_calls_between_pushes_leave_the_ring_alone():
    """a davo_forward_frames, a davo_forward, a streamed submit and a device batch of OTHER content between pushes (they use the
    slots' staging sets and frame buffers and rotate the slots): the pushes' bits stay"""
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, S = 36, 100, 3
    lanes, other = Lanes(cfg, S, PUSHES, H, W, seed=1), Lanes(cfg, S, PUSHES, H, W, seed=2)
    ref, e = _engine(cfg, H, W), _engine(cfg, H, W)
    want = _want(ref, lanes, "trajectory")
    e.set_inflight(2)
    extra = {}

    def between(t):
        if t == 3:
            fr = tuple(np.concatenate([q[k][:S + 2] if k != 1 else q[k][:S] for q in other.seqs[:1]]) for k in range(3))
            extra["frames"] = (e.forward_frames(*fr), fr)
        if t == 4:
            e.set_pairs("both")
            extra["forward"] = e.forward(*other.windows(4))
        if t == 5:
            extra["submit"] = np.full((S, 2, 6), np.nan, np.float32)
            e.submit(*other.windows(5), extra["submit"])

    _check(_track(e, lanes, "trajectory", between=between), want, "mixed calls")
    ref.set_pairs("both")
    assert _same(extra["frames"][0], ref.forward_frames(*extra["frames"][1]))
    assert _same(extra["forward"], ref.forward(*other.windows(4))) and _same(extra["submit"], ref.forward(*other.windows(5)))
    ref.close()
    e.close()


# ---- 7. the device form -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flagship", "se_depth_to_seg"])
def test_device_pushes_and_untouched_buffers(name):
    cfg = parse_version(VARIANTS[name])
    H, W, S = 36, 100, 3
    lanes = Lanes(cfg, S, PUSHES, H, W, seed=4)
    ref, e = _engine(cfg, H, W), _engine(cfg, H, W)
    want = _want(ref, lanes, "trajectory")
    e.set_inflight(2)
    e.track_begin(S, "trajectory")
    held = []
    for t in range(PUSHES):
        p = lanes.push(t)
        if p[1] is None:
            p = (p[0], np.zeros((S, 2, H, W, 2), np.float32)) + p[2:]
        bufs = [None if a is None else e.alloc(a.nbytes).upload(a) for a in p]
        pose = e.alloc(S * 12 * 4)
        n, ms = e.track_push_device(bufs[0], bufs[1], bufs[2], pose, timed=(t == 5), depth=bufs[3])
        assert n == (S if t >= 2 else 0) and (ms is None or ms > 0)
        held.append((p, bufs, pose))
    e.synchronize()
    for t, (p, bufs, pose) in enumerate(held):
        if t >= 2:
            assert _same(pose.download((S, 2, 6)), want[t]), t
        for a, b in zip(p, bufs):
            if a is not None:
                assert np.array_equal(b.download(a.shape, a.dtype).view(np.uint8), a.view(np.uint8))       # only ever read
        for b in bufs + [pose]:
            if b is not None:
                b.free()
    e.track_end()
    ref.close()
    e.close()


# ---- 8. range recovery ------------------------------------------------------------------------------------------------------
def test_a_guard_tripping_push_is_reissued_from_the_gathered_copy():
    """tests/test_stream.py's checkpoint (cnv3's activations leave the fp16-pair range) through track_push with the caller's
    arrays overwritten at once: the re-issue reads the library's snapshot of the staging set, never the ring, and the pushes
    after it are unaffected.  Two engines with the same history, one fed windows through davo_submit under the same selections
    and one fed pushes, deliver the same bits."""
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, S = 64, 64, 2
    weights = _rescaled(_weights(cfg), 16)
    lanes = Lanes(cfg, S, PUSHES, H, W, seed=8)
    a = _engine(cfg, H, W, S, weights=weights)
    a.set_inflight(2)
    want = {t: np.full((S, 2, 6), np.nan, np.float32) for t in range(2, PUSHES)}
    for t in want:
        a.set_pairs(_selection("trajectory", t))
        a.submit(*lanes.windows(t), want[t])
    a.synchronize()
    b = _engine(cfg, H, W, S, weights=weights)
    b.set_inflight(2)
    got = _track(b, lanes, "trajectory")
    for e in (a, b):
        stats = e.range_stats()
        assert stats["reissued"] > 0 and stats["f32_batches"] == 0, stats
    _check(got, want, "re-issued")
    a.close()
    b.close()


# ---- 9. errors --------------------------------------------------------------------------------------------------------------
def test_error_codes():
    H, W, S = 16, 16, 2
    vp = ctypes.c_void_p
    for name in ("flagship", "se_depth_to_seg"):
        cfg = parse_version(VARIANTS[name])
        e = _engine(cfg, H, W)
        L, ctx = e._L, e._ctx
        lanes = Lanes(cfg, S, 4, H, W)
        p = [None if a is None else a.ctypes.data_as(vp) for a in lanes.push(3)]
        out = np.zeros((S, 2, 6), np.float32)
        o = out.ctypes.data_as(vp)
        err = lambda: L.davo_last_error(ctx).decode()      # noqa: E731
        assert L.davo_track_push(ctx, p[0], p[1], p[2], p[3], o, 0) == -1 and "davo_track_begin" in err()      # push without begin
        assert L.davo_track_end(ctx) == -1 and L.davo_track_frames(ctx) == -1
        for bad in (0, -1, 4):
            assert L.davo_track_begin(ctx, bad, 0) == -1 and "lanes" in err()
        assert L.davo_track_begin(ctx, S, 2) == -1 and "policy" in err()
        assert L.davo_track_begin(ctx, S, 0) == 0
        assert L.davo_track_begin(ctx, S, 0) == -1 and "already" in err()                                      # begin twice
        # refused during a session
        assert L.davo_set_inflight(ctx, 2) == -1 and "tracking" in err()
        assert L.davo_set_feature_export(ctx, 1) == -1 and "tracking" in err()
        assert L.davo_set_heat_export(ctx, 1) == -1 and "tracking" in err()
        assert L.davo_set_label_format(ctx, 1) == -1
        win = lanes.windows(2)
        dwin = [e.alloc(a.nbytes).upload(a) for a in win]
        shifts = (ctypes.c_int * 6)()
        if cfg.needs_depth:
            assert L.davo_calibrate_depth(ctx, S, dwin[0].ptr, dwin[1].ptr, dwin[2].ptr, dwin[3].ptr, shifts) == -1 and "tracking" in err()
        else:
            assert L.davo_calibrate(ctx, S, dwin[0].ptr, dwin[1].ptr, dwin[2].ptr, shifts) == -1 and "tracking" in err()
        for k in range(3):                                   # pushes 0, 1: everything but flow2 and the poses is required
            if k == 1:
                continue
            q = list(p)
            q[k] = None
            assert L.davo_track_push(ctx, q[0], q[1], q[2], q[3], o, 0) == -1 and "null" in err()
        assert L.davo_track_push(ctx, p[0], None, p[2], p[3], None, 0) == 0
        assert L.davo_track_push(ctx, p[0], p[1], p[2], p[3], o, -1) == -1 and "hold" in err()
        assert L.davo_track_push(ctx, p[0], None, p[2], p[3], None, 0) == 0
        assert L.davo_track_frames(ctx) == 2
        for k in range(3):                                   # from the third push on flow2 and the poses too
            q = list(p)
            q[k] = None
            assert L.davo_track_push(ctx, q[0], q[1], q[2], q[3], o, 0) == -1 and "null" in err()
        assert L.davo_track_push(ctx, p[0], p[1], p[2], p[3], None, 0) == -1
        if cfg.needs_depth:                                  # a NULL depth pointer on a depth variant
            assert L.davo_track_push(ctx, p[0], p[1], p[2], None, o, 0) == -1
            assert "depth" in err() and "NULL" in err()
        d = [None if a is None else e.alloc(a.nbytes).upload(a) for a in lanes.push(3)]
        dp = [None if b is None else b.ptr for b in d]
        dpose = e.alloc(out.nbytes)
        assert L.davo_track_push_device(ctx, vp(dp[0].value + 4), dp[1], dp[2], dp[3], dpose.ptr, None) == -1 and "aligned" in err()      # misaligned
        assert L.davo_track_frames(ctx) == 2 and e.pending() == 0
        assert L.davo_track_push_device(ctx, dp[0], dp[1], dp[2], dp[3], dpose.ptr, None) == S
        assert L.davo_track_push(ctx, p[0], p[1], p[2], p[3], o, 0) == S
        assert L.davo_track_frames(ctx) == 4
        assert L.davo_track_end(ctx) == 0 and L.davo_track_end(ctx) == -1
        assert L.davo_set_inflight(ctx, 2) == 0              # legal again
        for b in dwin + [x for x in d if x is not None] + [dpose]:
            b.free()
        e._track_lanes = None
        # the Python layer
        with pytest.raises(davo_amd.DavoError):
            e.track_push(*lanes.push(3)[:3], out)
        with pytest.raises(ValueError):
            e.track_begin(S, "sometimes")
        e.track_begin(S)
        q = lanes.push(0)
        with pytest.raises(ValueError):
            e.track_push(q[0][:1], None, q[2], None, depth=q[3])
        if cfg.needs_depth:
            with pytest.raises(ValueError):
                e.track_push(q[0], None, q[2], None)
        e.close()                                            # davo_destroy frees a session left open


# ---- 10. device memory ------------------------------------------------------------------------------------------------------
def test_device_memory():
    """128x416 and 8 lanes so that every ring plane is more than one 2 MiB granule of the allocator"""
    cfg = parse_version(VARIANTS["se_depth_to_seg"])
    H, W, S = 128, 416, 8
    lanes = Lanes(cfg, S, PUSHES, H, W)
    pushes = [lanes.push(t) for t in range(PUSHES)]
    e = _engine(cfg, H, W, S)
    e.set_inflight(2)

    def cycle():
        e.track_begin(S, "trajectory")
        out = np.empty((S, 2, 6), np.float32)
        for p in pushes:
            e.track_push(p[0], p[1], p[2], out, depth=p[3])
        e.wait()
        inside = hip_free_bytes()
        e.track_end()
        return inside

    # a context that never begins allocates nothing for it: window work first, then a look
    win = lanes.windows(2)
    outs = [np.empty((S, 2, 6), np.float32) for _ in range(2)]
    for k in range(4):
        e.submit(*win[:3], outs[k % 2], depth=win[3])
    e.wait()
    before = hip_free_bytes()
    for k in range(4):
        e.submit(*win[:3], outs[k % 2], depth=win[3])
    e.wait()
    assert hip_free_bytes() == before
    inside = cycle()
    ring = 4 * S * H * W * (3 + 4 + 4)                      # four places of S frames, float32 label maps and depth planes
    after_first = hip_free_bytes()
    assert before - inside >= ring, (before, inside, ring)
    for _ in range(9):
        assert cycle() == inside
        assert hip_free_bytes() == after_first              # ten begin / 8 pushes / end cycles: where the first one left it
    assert after_first - inside >= ring                     # the ring goes with davo_track_end
    e.close()


# ---- 11. the Tracker and the CLI --------------------------------------------------------------------------------------------
def test_tracker_chains_what_stitch_trajectory_chains():
    from davo_amd import sequence as Sq
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, S, n = 36, 100, 3, 10
    lanes = Lanes(cfg, S, n, H, W, seed=6)
    ref, e = _engine(cfg, H, W), _engine(cfg, H, W)
    want = _want(ref, lanes, "trajectory", n)
    e.set_inflight(2)
    with davo_amd.Tracker(e, S) as tr:
        for t in range(n):
            p = lanes.push(t)
            tr.push(p[0], p[1], p[2], depth=p[3])
    assert len(tr.poses) == n - 2
    for s in range(S):
        stitched = Sq.stitch_trajectory(np.stack([want[t][s] for t in range(2, n)]))
        assert len(tr.trajectory(s)) == n and all(np.array_equal(a, b) for a, b in zip(tr.trajectory(s), stitched))
    ref.close()
    e.close()


@pytest.mark.parametrize("flags", [[], ["--labels", "u8", "--flow", "f16", "--flip"]], ids=["plain", "u8-f16-flip"])
def test_cli_online_writes_the_file_of_batch_1_trajectory(tmp_path, flags):
    """a 12-frame synthetic video as a dump in the reference's file layout (strips stored losslessly: consecutive windows must
    share their frames byte for byte, which JPEG strips of different windows need not)"""
    from PIL import Image
    from davo_amd import loader as L
    from davo_amd import run_kitti_pose as G
    H, W, n, seq = 32, 64, 12, 3
    img, flow, seg = davo_amd.windows_from_frames(*synth.make_frames(n, H, W))
    dump = str(tmp_path / "dump")
    os.makedirs(os.path.join(dump, "%.2d" % seq))
    for w in range(n - 2):
        jpg, flo, sg = L.window_paths(dump, seq, w + 1)
        Image.fromarray(img[w]).save(jpg, format="PNG")
        np.save(flo, flow[w])
        np.save(sg, seg[w])
    ckpt = str(tmp_path / "w.npz")
    np.savez(ckpt, **synth.make_weights(FLAGSHIP_VERSION))
    common = ["--test_seq", str(seq), "--concat_img_dir", dump, "--ckpt_file", ckpt, "--img_height", str(H), "--img_width", str(W),
              "--loader_procs", "0"] + flags
    files = {}
    for mode, extra in (("offline", ["--batch_size", "1", "--pairs", "trajectory"]), ("online", ["--online"])):
        out = str(tmp_path / mode)
        G.main(common + ["--output_dir", out] + extra)
        files[mode] = open(os.path.join(out, "%.2d-pred_kitti_pose.txt" % seq), "rb").read()
    assert files["online"] == files["offline"] and files["online"].count(b"\n") == n
