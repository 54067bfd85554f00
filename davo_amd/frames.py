"""The frame layout of a batch (include/davo_hip.h: "Frame sequences") on the host: conversion to and from the reference's
window layout, and the table of what a batch reads.

A sequence of N windows is N + 2 frames; window n is (src0, tgt, src1) = frames (n, n + 1, n + 2):

* ``frames`` u8  ``[N+2,H,W,3]``
* ``flow2``  f32 ``[N,2,H,W,2]``   (float16 for a binary16 engine, davo_amd.flow_to_f16: both conversions keep the dtype) planes (tgt->src0, tgt->src1) of window n - planes 0, 1 of the window layout's ``[B,4,H,W,2]``
* ``seg``        ``[N+2,H,W,1]``   float32 or uint8 (davo_amd.labels_to_u8)
* ``depth``  f32 ``[N+2,H,W,1]``   depth-source variants only (float16 for a binary16-depth engine, davo_amd.depth_to_f16: every conversion keeps the dtype)

The window layout is the reference's (``data_loader.py:537-557``, ``davo.py:978-1004``): strip ``[B,H,3W,3]`` src0|tgt|src1,
planes ``[B,3,H,W,1]`` in file order src0, tgt, src1.  ``Engine.forward_frames`` / ``submit_frames`` / ``forward_device_frames`` take
the frame layout as it is; the functions here are for callers and tests that need the other one."""
import ctypes

import numpy as np

from . import _lib
from .depth import DEPTH_FORMATS, check_depth_format
from .flow import FLOW_FORMATS, check_flow_format
from .labels import LABEL_FORMATS, check_label_format
from .version import att_source_id

PAIRS = {"src0": 1, "src1": 2, "both": 3}


def windows_from_frames(frames, flow2, seg, depth=None):
    """Frame layout -> the window-layout arrays ``(img, flow, seg)`` - ``(img, flow, seg, depth)`` when depth is given - that the
    window entry points take for the same N windows: byte for byte what the device gathers.  Flow planes 2, 3 are zero."""
    frames, flow2, seg = np.asarray(frames), np.asarray(flow2), np.asarray(seg)
    N = flow2.shape[0]
    if frames.ndim != 4 or frames.shape[0] != N + 2 or frames.shape[3] != 3:
        raise ValueError("frames shape %s: expected [N+2,H,W,3] for the %d windows of flow2" % (frames.shape, N))
    H, W = frames.shape[1:3]
    if flow2.shape != (N, 2, H, W, 2):
        raise ValueError("flow2 shape %s != %s" % (flow2.shape, (N, 2, H, W, 2)))
    seg = seg[..., None] if seg.ndim == 3 else seg
    if seg.shape != (N + 2, H, W, 1):
        raise ValueError("seg shape %s != %s" % (seg.shape, (N + 2, H, W, 1)))
    img = np.empty((N, H, 3 * W, 3), frames.dtype)
    for k in range(3):
        img[:, :, k * W:(k + 1) * W] = frames[k:k + N]
    flow = np.zeros((N, 4, H, W, 2), flow2.dtype)
    flow[:, :2] = flow2
    out = (img, flow, np.stack([seg[k:k + N] for k in range(3)], axis=1))
    if depth is not None:
        depth = np.asarray(depth)
        if depth.shape != (N + 2, H, W, 1):
            raise ValueError("depth shape %s != %s" % (depth.shape, (N + 2, H, W, 1)))
        out += (np.stack([depth[k:k + N] for k in range(3)], axis=1),)
    return out


def frames_from_windows(img, flow, seg, depth=None):
    """The inverse for CONSECUTIVE windows (window n + 1 starts one frame after window n): ``(frames, flow2, seg)`` -
    ``(frames, flow2, seg, depth)`` with depth.  Every frame but the first and the last is held by two or three windows;
    where they disagree a ValueError names the window and the plane (img / seg / depth, 0 src0, 1 tgt, 2 src1)."""
    img, flow, seg = np.asarray(img), np.asarray(flow), np.asarray(seg)
    B, H, W3 = img.shape[:3]
    W = W3 // 3
    if img.shape != (B, H, 3 * W, 3) or flow.shape != (B, 4, H, W, 2):
        raise ValueError("img %s / flow %s are not [B,H,3W,3] / [B,4,H,W,2]" % (img.shape, flow.shape))
    seg = seg[..., None] if seg.ndim == 4 else seg
    planes = {"img": np.stack([img[:, :, k * W:(k + 1) * W] for k in range(3)], axis=1), "seg": seg}
    if depth is not None:
        planes["depth"] = np.asarray(depth)
    out = {}
    for name, p in planes.items():
        if p.shape[:4] != (B, 3, H, W):
            raise ValueError("%s shape %s is not [B,3,H,W,...] of the %d windows of img" % (name, p.shape, B))
        f = np.concatenate([p[:, 0], p[-1, 1:]])                   # src0 of every window, then the last window's tgt and src1
        for n in range(B):
            for k in range(3):
                if not np.array_equal(p[n, k], f[n + k], equal_nan=p.dtype.kind == "f"):
                    raise ValueError("window %d, %s plane %d does not hold frame %d as its neighbours do: the windows are not "
                                     "consecutive windows of one sequence" % (n, name, k, n + k))
        out[name] = f
    res = (out["img"], np.ascontiguousarray(flow[:, :2]), out["seg"])
    return res + ((out["depth"],) if depth is not None else ())


def flip_windows(img, flow, seg, depth=None):
    """The left-right mirror of a window-layout batch as ``Engine.set_flip`` applies it on the device (include/davo_hip.h:
    davo_set_flip) - the training loader's rule (data_loader.py:142-169): every frame mirrored inside its own third of the strip,
    every flow plane, label map and depth plane mirrored on its own; no value changes (the horizontal flow component is not
    negated), plane and frame order stay.  -> new C-contiguous ``(img, flow, seg)`` - ``(img, flow, seg, depth)`` with depth - of
    the dtypes and shapes given ([B,H,3W,3]; [B,4,H,W,2]; [B,3,H,W,1] or [B,3,H,W])."""
    img, flow, seg = np.asarray(img), np.asarray(flow), np.asarray(seg)
    if img.ndim != 4 or img.shape[3] != 3 or img.shape[2] % 3:
        raise ValueError("img shape %s is not [B,H,3W,3]" % (img.shape,))
    B, H, W3 = img.shape[:3]
    W = W3 // 3
    if flow.shape != (B, 4, H, W, 2):
        raise ValueError("flow shape %s != %s" % (flow.shape, (B, 4, H, W, 2)))

    def planes(a, name):
        if a.shape[:4] != (B, 3, H, W) or a.shape[4:] not in ((), (1,)):
            raise ValueError("%s shape %s is not [B,3,H,W,1]" % (name, a.shape))
        return np.ascontiguousarray(a[:, :, :, ::-1])

    out = (np.ascontiguousarray(img.reshape(B, H, 3, W, 3)[:, :, :, ::-1]).reshape(B, H, W3, 3),
           np.ascontiguousarray(flow[:, :, :, ::-1]), planes(seg, "seg"))
    return out if depth is None else out + (planes(np.asarray(depth), "depth"),)


def flip_frames(frames, flow2, seg, depth=None):
    """flip_windows' rule on the frame layout: every frame, flow plane, label map and depth plane mirrored left-right on its own
    (frames [N+2,H,W,3], flow2 [N,2,H,W,2], seg and depth [N+2,H,W,1] or [N+2,H,W]); dtypes and shapes are kept.
    ``windows_from_frames(*flip_frames(...))`` is ``flip_windows(*windows_from_frames(...))``."""
    frames, flow2, seg = np.asarray(frames), np.asarray(flow2), np.asarray(seg)
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError("frames shape %s is not [N+2,H,W,3]" % (frames.shape,))
    if flow2.ndim != 5 or flow2.shape[1:] != (2,) + frames.shape[1:3] + (2,):
        raise ValueError("flow2 shape %s is not [N,2,H,W,2] of the frames %s" % (flow2.shape, frames.shape))

    def planes(a, name):
        if a.shape[:3] != frames.shape[:3] or a.shape[3:] not in ((), (1,)):
            raise ValueError("%s shape %s is not [N+2,H,W,1] of the frames %s" % (name, a.shape, frames.shape))
        return np.ascontiguousarray(a[:, :, ::-1])

    out = (np.ascontiguousarray(frames[:, :, ::-1]), np.ascontiguousarray(flow2[:, :, :, ::-1]), planes(seg, "seg"))
    return out if depth is None else out + (planes(np.asarray(depth), "depth"),)


def track_pushes(frames, flow2, seg, depth=None):
    """A frame sequence as a tracking session takes it (include/davo_hip.h "Online tracking"; Engine.track_push, Tracker.push):
    one tuple per frame, ``(frame [1,H,W,3], flow2 [1,2,H,W,2] or None, seg [1,H,W,1], depth [1,H,W,1] or None)`` - push t carries
    frame t, the flow pair of window t - 2 (None for the first two frames, which complete no window), label map t and depth plane
    t.  The arrays are views of the arguments (lanes = 1; stack the tuples of S sequences along axis 0 for S lanes)."""
    frames, flow2, seg = np.asarray(frames), np.asarray(flow2), np.asarray(seg)
    N = flow2.shape[0]
    if frames.ndim != 4 or frames.shape[0] != N + 2 or frames.shape[3] != 3:
        raise ValueError("frames shape %s: expected [N+2,H,W,3] for the %d windows of flow2" % (frames.shape, N))
    seg = seg[..., None] if seg.ndim == 3 else seg
    if seg.shape[0] != N + 2 or (depth is not None and np.asarray(depth).shape[0] != N + 2):
        raise ValueError("seg / depth hold another number of frames than frames' %d" % (N + 2))
    depth = None if depth is None else np.asarray(depth)
    return [(frames[t:t + 1], flow2[t - 2:t - 1] if t >= 2 else None, seg[t:t + 1], None if depth is None else depth[t:t + 1])
            for t in range(N + 2)]


def track_pushes_from_windows(img, flow, seg, depth=None):
    """track_pushes of a batch of CONSECUTIVE windows (frames_from_windows, which names the window and the plane where they are
    not): B windows -> B + 2 pushes.  ``windows_from_frames`` of the pushes' arrays put back together is the batch again."""
    return track_pushes(*frames_from_windows(img, flow, seg, depth))


def track_plan(H, W, lanes=1, pairs="src1", att_source="se_flow", labels="f32", flow="f32", depth="f32"):
    """Bytes one push of a tracking session copies across the link (include/davo_hip.h: davo_track_plan; no GPU needed): per lane a
    frame, a label map, a depth plane where ``att_source`` reads depth, and the flow planes of ``pairs``."""
    if pairs not in PAIRS:
        raise ValueError("pairs must be 'both', 'src0' or 'src1', got %r" % (pairs,))
    att = att_source_id(att_source) if isinstance(att_source, str) else int(att_source)
    nbytes = ctypes.c_longlong(0)
    rc = _lib.lib().davo_track_plan(int(H), int(W), int(lanes), PAIRS[pairs], att, LABEL_FORMATS[check_label_format(labels)],
                                    FLOW_FORMATS[check_flow_format(flow)], DEPTH_FORMATS[check_depth_format(depth)], ctypes.byref(nbytes))
    if rc != 0:
        raise ValueError("davo_track_plan(%r) refused its arguments" % ((H, W, lanes, pairs, att_source, labels, flow, depth),))
    return nbytes.value


def track_ring(inflight, t):
    """The ring rule of a tracking session as the library applies it (include/davo_hip.h: davo_track_ring; no GPU needed), for push
    ``t`` of a session begun with ``inflight`` slots: ``{'R', 'upload': place, 'read': (3 places, -1 for t < 2), 'upload_after':
    (3 pushes whose gather the upload waits for, -1 = none), 'gather_after': (2 pushes whose upload the gather waits for)}``."""
    places, after = (ctypes.c_int * 4)(), (ctypes.c_longlong * 5)()
    R = _lib.lib().davo_track_ring(int(inflight), int(t), places, after)
    if R < 0:
        raise ValueError("davo_track_ring(%r, %r) refused its arguments" % (inflight, t))
    return {"R": R, "upload": places[0], "read": tuple(places[1:4]), "upload_after": tuple(after[0:3]), "gather_after": tuple(after[3:5])}


def frames_plan(H, W, N, pairs="both", att_source="se_flow", labels="f32", flow="f32", depth="f32"):
    """What a frame-layout batch of N windows reads (include/davo_hip.h: davo_frames_plan - the function the library's copies and
    its gather kernel are driven by; no GPU needed): ``{'frames', 'seg', 'depth', 'flow': (lo, hi), 'link_bytes': int}`` - frame
    ranges of the pixels, the label maps and the depth planes ((0, 0) where the source reads no depth), the flow planes, and the
    bytes the host entry points send.  ``att_source``: a name of davo_amd.version.ATT_SOURCE / POOLED_ATT_SOURCE or its number.  ``flow``: "f32", or
    "f16" for a binary16 engine (davo_frames_plan_fmt): half the flow's bytes in 'link_bytes', the same ranges.  ``depth``: "f32",
    or "f16" for a binary16-depth engine (davo_frames_plan_fmt2): half the depth planes' bytes, the same ranges."""
    if pairs not in PAIRS:
        raise ValueError("pairs must be 'both', 'src0' or 'src1', got %r" % (pairs,))
    att = att_source_id(att_source) if isinstance(att_source, str) else int(att_source)
    r = (ctypes.c_int * 8)()
    nbytes = ctypes.c_longlong(0)
    lab = LABEL_FORMATS[check_label_format(labels)]
    if check_depth_format(depth) != "f32":
        rc = _lib.lib().davo_frames_plan_fmt2(int(H), int(W), int(N), PAIRS[pairs], att, lab, FLOW_FORMATS[check_flow_format(flow)],
                                              DEPTH_FORMATS[depth], r, ctypes.byref(nbytes))
    elif check_flow_format(flow) == "f32" and att <= 13:         # (davo_frames_plan keeps the range it was published with, 0..13)
        rc = _lib.lib().davo_frames_plan(int(H), int(W), int(N), PAIRS[pairs], att, lab, r, ctypes.byref(nbytes))
    else:
        rc = _lib.lib().davo_frames_plan_fmt(int(H), int(W), int(N), PAIRS[pairs], att, lab, FLOW_FORMATS[flow], r, ctypes.byref(nbytes))
    if rc != 0:
        raise ValueError("davo_frames_plan(%r) refused its arguments" % ((H, W, N, pairs, att_source, labels, flow) + (() if depth == "f32" else (depth,)),))
    return {"frames": (r[0], r[1]), "seg": (r[2], r[3]), "depth": (r[4], r[5]), "flow": (r[6], r[7]), "link_bytes": nbytes.value}
