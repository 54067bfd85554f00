"""The inputs the binary16-depth tests share (tests/test_f16_depth.py, tests/test_f16_depth_gpu.py): per depth source and shape
one seeded case - the float32 depth planes d, their rounded twin h = depth_to_f16(d), the widened halves depth_from_f16(h), and
weights under which the depth decides something:

* sources 11, 12 (the depth class tables): depth_source_ref.sensitive_weights, so that the tables depend on the depth mean;
* source 13 (the depth-split flow attention): the loaded depth_threshold sits BETWEEN a pixel's float32 depth and its rounded
  value - that pixel is near under one and far under the other - close to the median of the source planes, so both sides of the
  select are populated.

preconditions() states, on the float64 restatements alone, why a library that read anything but the halves' values could not
pass the GPU comparisons.  Nothing here touches the GPU."""
import collections

import numpy as np

from davo_amd import depth_from_f16, depth_to_f16, flow_from_f16, flow_to_f16, parse_version, synth

import depth_source_ref as D
import depthseg_attention_ref as R

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128"
VERSIONS = {
    11: BASE + "-segmask_all-se_depth_wo_tgt_to_seg-fc_tanh",
    12: BASE + "-segmask_all-se_depth_to_seg-fc_tanh",
    13: BASE + "-segmask_all-se_flow_on_depthseg_seplayers-abs_flow-fc_tanh",
}
SOURCES = (11, 12, 13)
# (H, W, B): the smallest context | W % 8 == 4: 8-byte mirror units, ragged tiles | W % 8 == 0 with three 16-byte units: the
# middle unit of an odd row | the remaining mirror row form (an even number of 16-byte units)
SHAPES = ((16, 16, 1), (36, 100, 3), (32, 24, 2), (64, 64, 2))
FRAME_CASES = ((1, 36, 100), (9, 36, 100))      # (N, H, W) of the frame-layout cases
COST_SHAPE = (36, 100, 3)                 # where the rounding's cost in the poses is recorded

Case = collections.namedtuple("Case", "source cfg img flow seg d h wide weights")
_CASES = {}


def place_threshold(d, wide, seg):
    """The float32 threshold for source 13: among the pixels of the source planes (file planes 0, 2) whose rounded depth differs
    from the float32 one and whose label is a class, the one closest to the planes' median; thr = the larger of its two values,
    so the smaller one is near (depth < thr, strict) and the larger one far."""
    src = [0, 2]
    dd, ww, ss = d[:, src, :, :, 0], wide[:, src, :, :, 0], np.asarray(seg, np.float32)[:, src, :, :, 0]
    ok = (dd != ww) & (ss >= 0) & (ss < 19)
    assert ok.any()
    med = np.float32(np.median(dd))
    flat = np.flatnonzero(ok.ravel())
    p = flat[np.argmin(np.abs(dd.ravel()[flat] - med))]
    thr = np.float32(max(dd.ravel()[p], ww.ravel()[p]))
    assert (dd.ravel()[p] < thr) != (ww.ravel()[p] < thr)
    return thr


def case(source, H, W, B, first_window=5):
    key = (source, H, W, B, first_window)
    if key not in _CASES:
        cfg = parse_version(VERSIONS[source])
        img, flow, seg = synth.make_inputs(B, H, W, first_window=first_window)
        d = synth.make_depth(B, H, W, first_window=first_window)
        h = synth.make_depth(B, H, W, first_window=first_window, fmt="f16")
        wide = depth_from_f16(h)
        weights = synth.make_weights(cfg)
        if source == 13:
            weights = R.with_mlps(weights, thr=place_threshold(d, wide, seg))
        else:
            weights = D.sensitive_weights(cfg, weights, d)
        for a in (img, flow, seg, d, h, wide):
            a.setflags(write=False)                           # shared among the tests: left unchanged
        _CASES[key] = Case(source, cfg, img, flow, seg, d, h, wide, weights)
    return _CASES[key]


def ref(source):
    return R if source == 13 else D


_FRAME_CASES = {}


def frames_case(source, N, H, W):
    """A frame-layout case: N + 2 synthetic frames (synth.make_frames; float32 labels and flow, float32 depth planes) and, as a
    Case, the N windows they expand to - so preconditions() and the restatements apply to exactly what the `_frames' entry points
    gather.  Weights as in case(), chosen on these windows.  -> (Case, (frames, flow2, seg, d, h) in the frame layout)"""
    from davo_amd import windows_from_frames
    key = (source, N, H, W)
    if key not in _FRAME_CASES:
        cfg = parse_version(VERSIONS[source])
        frames, flow2, seg, d = synth.make_frames(N + 2, H, W, depth=True)
        h = depth_to_f16(d)
        img, flow, wseg, wd = windows_from_frames(frames, flow2, seg, d)
        wh = windows_from_frames(frames, flow2, seg, h)[3]
        wide = depth_from_f16(wh)
        weights = synth.make_weights(cfg)
        if source == 13:
            weights = R.with_mlps(weights, thr=place_threshold(wd, wide, wseg))
        else:
            weights = D.sensitive_weights(cfg, weights, wd)
        for a in (frames, flow2, seg, d, h, img, flow, wseg, wd, wh, wide):
            a.setflags(write=False)
        _FRAME_CASES[key] = (Case(source, cfg, img, flow, wseg, wd, wh, wide, weights), (frames, flow2, seg, d, h))
    return _FRAME_CASES[key]


_POSES = {}


def reference_poses(c, conv, depth="wide", flow16=False):
    """float64 restatement's poses [B,2,6] on the case's widened halves (what both engines are given) or on d; flow16: on the
    flow rounded to binary16 and widened, what an engine with binary16 flow computes on.  Computed once per case."""
    key = (id(c), depth, flow16)
    if key not in _POSES:
        flow = flow_from_f16(flow_to_f16(c.flow)) if flow16 else c.flow
        _POSES[key] = ref(c.source).forward(c.cfg, c.img, flow, c.seg, getattr(c, depth), c.weights, conv=conv)
    return _POSES[key]


def reference_tables(c, depth="wide"):
    """-> the float64 tables the engine's att_table is compared with ([B,3,19]; source 13: (near, far))"""
    if c.source == 13:
        return R.class_tables(c.cfg, c.flow, c.weights)
    return D.class_tables(c.cfg, getattr(c, depth), c.weights)


def preconditions(c, conv):
    """What makes the GPU comparisons of this case meaningful, on the restatements alone; -> the largest pose change."""
    assert c.h.dtype == np.float16 and np.array_equal(c.h.view(np.uint16), depth_to_f16(c.d).view(np.uint16))
    moved = c.wide != c.d
    assert moved.mean() > 0.5, moved.mean()                    # the rounded depth differs from the float32 depth in most pixels
    if c.source == 13:
        thr = c.weights[R.THRESHOLD]
        near_d, near_w = R.near_mask(c.d, thr), R.near_mask(c.wide, thr)
        flipped = (near_d != near_w)[:, (0, 2)]
        assert flipped.any(), "no source pixel changes side under rounding"
        side = near_w[:, (0, 2)]
        assert side.any() and (~side).any()                   # both sides of the threshold are populated
    a, b = reference_poses(c, conv, "d"), reference_poses(c, conv, "wide")
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert not np.array_equal(np.asarray(a, np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64))
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())
