"""The frame layout on the host (include/davo_hip.h "Frame sequences"; davo_amd/frames.py): the ABI's new symbols, the
conversions to and from the window layout, the table of what a batch copies - from the function the library's copies use -
and the sequence driver, against a fake engine.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import davo_amd
from davo_amd import _lib, synth
from davo_amd import sequence as S
from davo_amd.version import ATT_SOURCE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("davo_forward_frames", "davo_submit_frames", "davo_forward_device_frames", "davo_frames_plan")


def test_new_symbols_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "davo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(davo_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_lib.build())
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name


@pytest.mark.parametrize("labels", ["f32", "u8"])
def test_round_trip_between_the_layouts(labels):
    H, W, n = 16, 20, 7
    frames, flow2, seg, depth = synth.make_frames(n, H, W, depth=True, labels=labels)
    assert frames.shape == (n, H, W, 3) and flow2.shape == (n - 2, 2, H, W, 2) and seg.shape == depth.shape == (n, H, W, 1)
    assert seg.dtype == (np.uint8 if labels == "u8" else np.float32)
    for a in (frames, seg, depth):                          # no two frames agree in any plane
        assert all(not np.array_equal(a[i], a[j]) for i in range(n) for j in range(i))
    assert not np.array_equal(flow2[:, 0], flow2[:, 1])
    img, flow, wseg, wdepth = davo_amd.windows_from_frames(frames, flow2, seg, depth)
    N = n - 2
    assert img.shape == (N, H, 3 * W, 3) and flow.shape == (N, 4, H, W, 2) and wseg.shape == wdepth.shape == (N, 3, H, W, 1)
    assert img.dtype == np.uint8 and wseg.dtype == seg.dtype and wdepth.dtype == np.float32
    for w in range(N):
        for k in range(3):
            assert np.array_equal(img[w, :, k * W:(k + 1) * W], frames[w + k])
            assert np.array_equal(wseg[w, k], seg[w + k]) and np.array_equal(wdepth[w, k], depth[w + k])
    assert np.array_equal(flow[:, :2], flow2) and not flow[:, 2:].any()
    back = davo_amd.frames_from_windows(img, flow, wseg, wdepth)
    for a, b in zip(back, (frames, flow2, seg, depth)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert len(davo_amd.windows_from_frames(frames, flow2, seg)) == 3
    assert len(davo_amd.frames_from_windows(img, flow, wseg)) == 3
    # make_inputs is untouched, and its windows are NOT consecutive windows of one sequence
    with pytest.raises(ValueError):
        davo_amd.frames_from_windows(*synth.make_inputs(2, H, W))


@pytest.mark.parametrize("what,window,plane", [("img", 1, 0), ("img", 3, 1), ("seg", 2, 2), ("depth", 0, 1)])
def test_one_pixel_of_disagreement_is_named(what, window, plane):
    H, W = 16, 16
    parts = list(davo_amd.windows_from_frames(*synth.make_frames(7, H, W, depth=True)))
    if what == "img":
        parts[0][window, 5, plane * W + 3, 1] ^= 1
    else:
        parts[{"seg": 2, "depth": 3}[what]][window, plane, 5, 3, 0] += 1.0
    with pytest.raises(ValueError) as err:
        davo_amd.frames_from_windows(*parts)
    # the frame is held by up to three windows: the first (window, plane) that differs from the frame array is named, and
    # it is the edited one or a neighbour that holds the same frame
    m = re.search(r"window (\d+), (\w+) plane (\d)", str(err.value))
    assert m and m.group(2) == what and int(m.group(1)) + int(m.group(3)) == window + plane, str(err.value)


H0, W0 = 128, 416
HW0 = H0 * W0


def test_link_bytes_per_window_at_the_flagship_shape():
    """The table of INTEGRATION.md, from davo_frames_plan - the function the host entry points' copies are driven by.  Per
    window of a long batch, both pairs, no depth: one frame (3 HW) + two flow planes [H,W,2] float32 (16 HW) + one label map
    (4 HW, or HW as bytes), against the window layout's strip (9 HW) + the same flow + two label maps (davo_submit's copy).
    The flow term is 16 HW = 851,968 B (638,976 B = 12 HW is the size of a window's three float32 label maps, not of two
    [H,W,2] float32 flow planes), so the frame rows are 1,224,704 B (-30 %) and 1,064,960 B (-26 %)."""
    windows = {"f32": 9 * HW0 + 16 * HW0 + 2 * 4 * HW0, "u8": 9 * HW0 + 16 * HW0 + 2 * HW0}
    assert windows == {"f32": 1757184, "u8": 1437696}
    want = {"f32": (159744, 851968, 212992), "u8": (159744, 851968, 53248)}
    for labels, terms in want.items():
        a = davo_amd.frames_plan(H0, W0, 32, "both", "se_flow", labels)["link_bytes"]
        b = davo_amd.frames_plan(H0, W0, 33, "both", "se_flow", labels)["link_bytes"]
        assert b - a == sum(terms), (labels, b - a)
        assert a - 32 * (b - a) == 2 * (terms[0] + terms[2])            # each batch additionally sends its two extra frames
        assert terms[0] == 3 * HW0 and terms[1] == 16 * HW0 and terms[2] == (4 if labels == "f32" else 1) * HW0
    assert sum(want["f32"]) == 1224704 and sum(want["u8"]) == 1064960
    assert round(100 * (1 - 1224704 / 1757184)) == 30 and round(100 * (1 - 1064960 / 1437696)) == 26
    # a depth source adds one float32 plane per window
    d = [davo_amd.frames_plan(H0, W0, n, "both", "se_depth_to_seg", "f32")["link_bytes"] for n in (32, 33)]
    assert d[1] - d[0] == sum(want["f32"]) + 4 * HW0


@pytest.mark.parametrize("N", [1, 2, 5])
def test_frame_ranges_of_the_selection_table(N):
    not_attended, attended = "se_flow", "se_rgb_to_seg"
    d_wo, d_with, d_split = "se_depth_wo_tgt_to_seg", "se_depth_to_seg", "se_flow_depthseg_sep"
    assert ATT_SOURCE[d_split] == 13

    def plan(pairs, att):
        return davo_amd.frames_plan(16, 16, N, pairs, att)

    for att in (not_attended, attended, d_wo, d_with, d_split):
        p = plan("both", att)
        assert p["frames"] == (0, N + 2) and p["flow"] == (0, 2) and p["seg"] == (0, N + 2)
        assert p["depth"] == ((0, N + 2) if att in (d_wo, d_with, d_split) else (0, 0))
    for att, tgt in ((not_attended, False), (attended, True), (d_wo, False), (d_with, True), (d_split, False)):
        p0, p1 = plan("src0", att), plan("src1", att)
        assert p0["frames"] == (0, N + 1) and p0["flow"] == (0, 1)
        assert p1["frames"] == (1, N + 2) and p1["flow"] == (1, 2)
        assert p0["seg"] == ((0, N + 1) if tgt else (0, N)) and p1["seg"] == ((1, N + 2) if tgt else (2, N + 2))
    for att in (d_wo, d_with):                                         # sources 11, 12: the target's plane and the source's
        assert plan("src0", att)["depth"] == (0, N + 1) and plan("src1", att)["depth"] == (1, N + 2)
    assert plan("src0", d_split)["depth"] == (0, N) and plan("src1", d_split)["depth"] == (2, N + 2)      # 13: the source's alone
    assert plan("src0", not_attended)["depth"] == (0, 0)
    # one pair of the flagship at 128x416: two frames' pixels less one, one flow plane, one label map
    p = [davo_amd.frames_plan(H0, W0, n, "src1", "se_flow")["link_bytes"] for n in (32, 33)]
    assert p[1] - p[0] == 3 * HW0 + 8 * HW0 + 4 * HW0
    L = _lib.lib()
    for bad in ((16, 16, 0, 3, 1, 0), (16, 16, 1, 0, 1, 0), (16, 16, 1, 4, 1, 0), (16, 16, 1, 3, 14, 0), (16, 16, 1, 3, 1, 2), (0, 16, 1, 3, 1, 0)):
        assert L.davo_frames_plan(*bad, None, None) < 0, bad
    with pytest.raises(ValueError):
        davo_amd.frames_plan(16, 16, 1, "all")


class _FakeEngine:
    """records its calls; poses say which window they are of"""

    def __init__(self):
        self.calls, self.pairs = [], "both"

    def set_pairs(self, pairs):
        self.calls.append(("set_pairs", pairs))
        self.pairs = pairs

    def forward_frames(self, frames, flow2, seg, depth=None):
        self.calls.append(("forward_frames", frames.shape[0], flow2.shape[0], int(frames[0, 0, 0, 0]), self.pairs, depth is not None))
        out = np.zeros((flow2.shape[0], 2, 6), np.float32)
        out[:, :, 3] = (int(frames[0, 0, 0, 0]) + np.arange(flow2.shape[0]))[:, None] + 1.0
        return out


class _FakeStream:
    def __init__(self):
        self.calls, self.drained, self.pending = [], 0, []

    def submit_frames(self, frames, flow2, seg, out, depth=None, pairs=None):
        self.calls.append(("submit_frames", frames.shape[0], flow2.shape[0], int(frames[0, 0, 0, 0]), pairs, depth is not None))
        assert out.shape == (flow2.shape[0], 2, 6) and out.flags.c_contiguous and out.dtype == np.float32
        self.pending.append((out, int(frames[0, 0, 0, 0])))

    def drain(self):
        self.drained += 1
        for out, lo in self.pending:                        # delivered late, into the caller's rows
            out[:, :, 3] = (lo + np.arange(out.shape[0]))[:, None] + 1.0
        self.pending = []


def _loader(n_frames, depth=False, log=None):
    def load(lo, hi):
        if log is not None:
            log.append((lo, hi))
        frames = np.zeros((hi - lo + 2, 16, 16, 3), np.uint8)
        frames[:, 0, 0, 0] = np.arange(lo, hi + 2)          # frame numbers, readable by the fakes
        parts = (frames, np.zeros((hi - lo, 2, 16, 16, 2), np.float32), np.zeros((hi - lo + 2, 16, 16, 1), np.float32))
        return parts + ((np.ones((hi - lo + 2, 16, 16, 1), np.float32),) if depth else ())
    assert n_frames >= 3
    return load


def test_run_frames_batches_tail_and_pairs():
    n_frames, B = 13, 4                                     # 11 windows: 4, 4 and a short batch of 3 - issued short, not padded
    log = []
    e = _FakeEngine()
    traj, poses = S.run_frames(e, _loader(n_frames, log=log), n_frames, B)
    assert log == [(0, 4), (4, 8), (8, 11)]
    assert e.calls == [("forward_frames", 6, 4, 0, "both", False), ("forward_frames", 6, 4, 4, "both", False), ("forward_frames", 5, 3, 8, "both", False)]
    assert poses.shape == (11, 2, 6) and np.array_equal(poses[:, 0, 3], np.arange(11) + 1.0) and len(traj) == n_frames
    want = S.stitch_trajectory(poses)
    assert all(np.array_equal(a, b) for a, b in zip(traj, want))
    # 'trajectory': the batch with window 0 runs both pairs, every other batch tgt->src1 alone; depth is passed along
    e = _FakeEngine()
    S.run_frames(e, _loader(n_frames, depth=True), n_frames, B, pairs="trajectory")
    assert e.calls == [("forward_frames", 6, 4, 0, "both", True), ("set_pairs", "src1"), ("forward_frames", 6, 4, 4, "src1", True),
                       ("forward_frames", 5, 3, 8, "src1", True)]
    # a stream: submitted with the selection, drained once, poses land in the returned array
    s = _FakeStream()
    traj, poses = S.run_frames(s, _loader(n_frames), n_frames, B, pairs="trajectory")
    assert s.calls == [("submit_frames", 6, 4, 0, "both", False), ("submit_frames", 6, 4, 4, "src1", False), ("submit_frames", 5, 3, 8, "src1", False)]
    assert s.drained == 1 and np.array_equal(poses[:, 1, 3], np.arange(11) + 1.0)
    s = _FakeStream()
    S.run_frames(s, _loader(n_frames), n_frames, B)
    assert [c[4] for c in s.calls] == [None, None, None]
    with pytest.raises(ValueError):
        S.run_frames(_FakeEngine(), _loader(n_frames), n_frames, B, pairs="src1")
    # a batch size that divides the windows: no short batch; fewer windows than a batch: one short batch
    e = _FakeEngine()
    S.run_frames(e, _loader(6), 6, 2)
    assert [c[1:3] for c in e.calls] == [(4, 2), (4, 2)]
    e = _FakeEngine()
    S.run_frames(e, _loader(3), 3, 4)
    assert [c[1:3] for c in e.calls] == [(3, 1)]


def test_engine_checks_refuse_before_the_library_is_asked():
    """shape and dtype checks of the frame entry points are _check_batch's kind: a ValueError, nothing converted silently"""
    from davo_amd.davo import Engine
    e = Engine.__new__(Engine)
    e.H, e.W, e.labels = 16, 16, "f32"
    frames, flow2, seg = synth.make_frames(4, 16, 16)
    assert e._check_frames(frames, flow2, e._frame_label_arg(seg)) == 2
    with pytest.raises(ValueError):
        e._check_frames(frames[:3], flow2, seg)             # N + 2 frames for N windows
    with pytest.raises(ValueError):
        e._check_frames(frames, flow2[:, :1], seg)
    with pytest.raises(ValueError):
        e._check_frames(frames, flow2, seg[:3])
    with pytest.raises(ValueError):
        e._frame_label_arg(davo_amd.labels_to_u8(seg))      # bytes to a float32 engine
    e.labels = "u8"
    with pytest.raises(ValueError):
        e._frame_label_arg(seg)
    assert e._frame_label_arg(davo_amd.labels_to_u8(seg)[..., 0]).shape == (4, 16, 16, 1)
    e._ctx = None                                           # (never created: nothing to destroy)
