"""Host side of the pose path: the reference's ``DAVO`` call surface over libdavo_hip.so.

Mirrors ``DAVO.__init__`` (reference davo.py:31-33), ``setup_inference`` (davo.py:1533-1551)
and ``inference`` (davo.py:1553-1569).  The TF reference takes tensors of a tf.data iterator
and pulls the next batch inside ``sess.run``; here the inputs are numpy arrays, or an iterator
yielding ``(img_u8, flow, seg)`` batches (``(img_u8, flow, seg, depth)`` for a depth-source variant), pulled once per ``inference`` call.  Weights enter
through ``load_weights`` — the stand-in for ``tf.train.Saver(...).restore``
(test_kitti_pose.py:129-131) — keyed by the TF variable names.
"""
import collections
import ctypes

import numpy as np

from . import _lib
from .labels import LABEL_DTYPES, LABEL_FORMATS, check_label_format, labels_to_u8  # noqa: F401
from .flow import FLOW_DTYPES, FLOW_FORMATS, check_flow_format, flow_from_f16, flow_to_f16  # noqa: F401
from .depth import DEPTH_DTYPES, DEPTH_FORMATS, check_depth_format, depth_from_f16, depth_to_f16  # noqa: F401
from .frames import flip_windows
from .version import NUM_SEG_CLASSES, att_source_id, parse_version, weight_shapes


DEPTH_THRESHOLD = "pose_exp_net/se_flow/depth_threshold"      # the rank-0 variable of `-se_flow_on_depthseg_seplayers'


class DavoError(RuntimeError):
    pass


class DavoRangeError(DavoError):
    """f16x3: a layer's activations left the fp16-pair storage range (include/davo_hip.h: DAVO_ERR_RANGE).
    Only raised with ``set_option("auto_range", 0)``: by default the library re-issues such a batch itself
    (re-calibrated, or on its float32 kernels), as the reference's float32 graph never fails on a finite network."""


_PY_ERR = {-1: ValueError, -2: DavoError, -3: DavoError, -4: MemoryError, -5: DavoRangeError}


class _PinnedBlock:
    """hipHostMalloc'd block; freed when the last numpy view of it goes away."""

    def __init__(self, device, nbytes):
        p = ctypes.c_void_p()
        if _lib.lib().davo_host_alloc(int(device), int(nbytes), ctypes.byref(p)) != 0:
            raise DavoError("davo_host_alloc(%d bytes) failed on device %d" % (nbytes, device))
        self.ptr, self.nbytes = p, int(nbytes)

    def __del__(self):
        if getattr(self, "ptr", None):
            _lib.lib().davo_host_free(self.ptr)
            self.ptr = None


def pinned_empty(shape, dtype, device=0):
    """numpy array over page-locked host memory (include/davo_hip.h: davo_host_alloc): buffers filled by the
    loader and handed to DAVO.inference / Engine.forward copy at the PCIe DMA rate."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    blk = _PinnedBlock(device, max(n, 1))
    buf = (ctypes.c_uint8 * blk.nbytes).from_address(blk.ptr.value)
    buf._owner = blk                                   # the ctypes object is the array's base; it keeps the block alive
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


def pin_array(arr, device=0):
    """Page-lock the memory of a C-contiguous numpy array in place (include/davo_hip.h: davo_host_register)."""
    if not arr.flags.c_contiguous:
        raise ValueError("only a C-contiguous array can be page-locked in place")
    if _lib.lib().davo_host_register(int(device), ctypes.c_void_p(arr.ctypes.data), arr.nbytes) != 0:
        raise DavoError("davo_host_register(%d bytes) failed on device %d" % (arr.nbytes, device))


def unpin_array(arr):
    if _lib.lib().davo_host_unregister(ctypes.c_void_p(arr.ctypes.data)) != 0:
        raise DavoError("davo_host_unregister failed")


def _is_ready(a, dtype):
    """a C-contiguous numpy array of that dtype: it goes to the library as it is"""
    return isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous


def _ptr(a):
    """an argument as the library takes it: a numpy array's or a DeviceBuffer's address, anything else as it is"""
    return a.ctypes.data if isinstance(a, np.ndarray) else getattr(a, "ptr", a)


class DeviceBuffer:
    """A hipMalloc'd buffer owned through a context (bench / multi-GPU shards keep inputs in HBM)."""

    def __init__(self, engine, nbytes):
        self.engine, self.nbytes = engine, int(nbytes)
        self.dtype = None                                  # of the array uploaded last (Engine.forward_device checks the label maps' against its format)
        p = ctypes.c_void_p()
        engine._check(_lib.lib().davo_device_malloc(engine._ctx, self.nbytes, ctypes.byref(p)))
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.dtype = arr.dtype
        self.engine._check(_lib.lib().davo_memcpy_h2d(self.engine._ctx, self.ptr, arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes))
        return self

    def download(self, shape, dtype=np.float32):
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        self.engine._check(_lib.lib().davo_memcpy_d2h(self.engine._ctx, out.ctypes.data_as(ctypes.c_void_p), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            _lib.lib().davo_device_free(self.engine._ctx, self.ptr)
            self.ptr = None


class Engine:
    """Thin object wrapper of one ``davo_ctx`` (one GPU, one host thread)."""

    def __init__(self, cfg, img_height, img_width, max_batch, device=0, labels="f32", flow="f32", depth="f32"):
        """``labels``: the format of every label map this engine takes - "f32" (the reference's float32 [B,3,H,W,1], the default)
        or "u8" (uint8 class ids, a quarter of the bytes; include/davo_hip.h: davo_set_label_format, davo_amd.labels_to_u8).
        ``flow``: the format of every flow array - "f32" (the default) or "f16" (IEEE binary16 in the same layout, half the
        bytes; include/davo_hip.h: davo_set_flow_format, davo_amd.flow_to_f16).
        ``depth``: the format of every depth array - "f32" (the default) or "f16" (IEEE binary16 in the same layout, half the
        bytes; include/davo_hip.h: davo_set_depth_format, davo_amd.depth_to_f16).  A variant that reads no depth accepts it."""
        check_label_format(labels)
        check_flow_format(flow)
        check_depth_format(depth)
        self.cfg, self.H, self.W, self.max_batch, self.device = cfg, img_height, img_width, max_batch, device
        self.labels = "f32"
        self.flow = "f32"
        self.depth = "f32"
        self._L = _lib.lib()
        self._ctx = ctypes.c_void_p()
        self.host_chunk = 8                       # davo_set_option "host_chunk" as last set through set_option (its default)
        v = _lib.DavoVariant(*cfg.as_c_ints())
        rc = self._L.davo_create(ctypes.byref(self._ctx), device, img_height, img_width, max_batch, ctypes.byref(v))
        if rc != 0:
            msg = self._L.davo_last_error(self._ctx).decode() if self._ctx else "davo_create failed"
            if self._ctx:
                self._L.davo_destroy(self._ctx)
                self._ctx = ctypes.c_void_p()
            raise _PY_ERR.get(rc, DavoError)(msg)
        if cfg.posenn_se != "none":               # `-se_insert': before any weight is loaded (include/davo_hip.h)
            try:
                self._check(self._L.davo_set_posenn_se(self._ctx, {"insert": 1}[cfg.posenn_se]))
            except Exception:
                self.close()
                raise
        if cfg.posenn == "triplet":               # `-dilatedPoseNN' without `-sharedNN': likewise before any weight (davo_set_posenn_topology)
            try:
                self._check(self._L.davo_set_posenn_topology(self._ctx, _lib.POSENN_TRIPLET))
            except Exception:
                self.close()
                raise
        if cfg.heads == "coupled":                # `-sharedNN-dilatedCouplePoseNN': likewise before any weight (davo_set_posenn_heads)
            try:
                self._check(self._L.davo_set_posenn_heads(self._ctx, _lib.POSENN_HEADS_COUPLED))
            except Exception:
                self.close()
                raise
        try:
            for attr, value in (("labels", labels), ("flow", flow), ("depth", depth)):
                if value != "f32":
                    self._set_format(attr, value)
        except Exception:
            self.close()
            raise

    # the engine attribute of each plane kind -> (the C setter, its values, the name check)
    _FORMATS = {"labels": ("davo_set_label_format", LABEL_FORMATS, check_label_format),
                "flow": ("davo_set_flow_format", FLOW_FORMATS, check_flow_format),
                "depth": ("davo_set_depth_format", DEPTH_FORMATS, check_depth_format)}

    def _set_format(self, attr, value):
        """The three format setters' one body (include/davo_hip.h: davo_set_label_format / _flow_format / _depth_format): before
        the first call that takes inputs, ValueError afterwards.  From then on every array of that kind must have the format's
        dtype; nothing is converted silently."""
        setter, values, check = self._FORMATS[attr]
        self._check(getattr(self._L, setter)(self._ctx, values[check(value)]))
        setattr(self, attr, value)

    def set_label_format(self, labels):
        """Select the label format, "f32" or "u8" (see _set_format)."""
        self._set_format("labels", labels)

    def set_flow_format(self, flow):
        """Select the flow format, "f32" or "f16" (see _set_format)."""
        self._set_format("flow", flow)

    def set_depth_format(self, depth):
        """Select the depth format, "f32" or "f16" (see _set_format)."""
        self._set_format("depth", depth)

    def _f16_arg(self, a, noun):
        """An array of the plane kind ``noun`` ("flow" | "depth") as the entry points take it: C-contiguous, of the engine's format
        of that kind.  A float16 array handed to a float32 engine, or anything but float16 to a binary16 engine, is a ValueError."""
        is_f16 = np.asarray(a).dtype == np.float16
        if getattr(self, noun) == "f16":
            if not is_f16:
                raise ValueError("this engine takes float16 %s (%s='f16'), got dtype %s: convert with davo_amd.%s_to_f16" % (noun, noun, np.asarray(a).dtype, noun))
            return np.ascontiguousarray(a)
        if is_f16:
            raise ValueError("this engine takes float32 %s (%s='f32'), got float16: create it with %s='f16'" % (noun, noun, noun))
        return np.ascontiguousarray(a, np.float32)

    def _label_arg(self, seg):
        """The label maps of a batch as the entry points take them: C-contiguous [B,3,H,W,1] of the engine's format.  A byte
        array handed to a float32 engine, or anything but bytes to a byte engine, is a ValueError."""
        is_u8 = np.asarray(seg).dtype == np.uint8
        if self.labels == "u8":
            if not is_u8:
                raise ValueError("this engine takes uint8 label maps (labels='u8'), got dtype %s: convert with davo_amd.labels_to_u8" % np.asarray(seg).dtype)
            seg = np.ascontiguousarray(seg)
            return seg[..., None] if seg.ndim == 4 else seg
        if is_u8:
            raise ValueError("this engine takes float32 label maps (labels='f32'), got uint8: create it with labels='u8'")
        return np.ascontiguousarray(seg, np.float32)

    def _check(self, rc):
        if rc != 0:
            raise _PY_ERR.get(rc, DavoError)(self._L.davo_last_error(self._ctx).decode())

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.davo_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    __del__ = close

    def load_weights(self, weights):
        want = weight_shapes(self.cfg)
        for name in want:
            if name not in weights:
                raise KeyError("checkpoint has no variable `%s'" % name)
        for name in want:
            a = np.asarray(weights[name], np.float32)
            a = a.copy() if a.shape == () else np.ascontiguousarray(a)      # (np.ascontiguousarray would make a rank-0 variable [1])
            shape = (ctypes.c_int64 * a.ndim)(*a.shape)
            self._check(self._L.davo_load_weight(self._ctx, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), shape, a.ndim))

    def _depth_arg(self, depth, shape, names, strict=None):
        """The depth planes of a batch as the entry points take them (of the engine's depth format and of ``shape``: [B,3,H,W,1]
        in file order src0, tgt, src1, davo.py:991-996, or the frame layout's [N+2,H,W,1]), or None for a variant that reads none
        (a depth array handed to such a variant is ignored, as the reference ignores its depth input there).  A float16 array
        handed to a float32 engine, or anything but float16 to a binary16 engine, is a ValueError (_f16_arg).  ``strict``: see _contiguous."""
        if not self.cfg.needs_depth:
            return None
        if strict and not _is_ready(depth, DEPTH_DTYPES[self.depth]):
            raise ValueError("%s(hold > 0) needs a C-contiguous %s depth array (a converted copy would not outlive the call)"
                             % (strict, DEPTH_DTYPES[self.depth]))
        if depth is None:
            raise ValueError("%s and depth inputs are all required for version `%s'" % (names, self.cfg.version))
        depth = self._f16_arg(depth, "depth")
        if depth.shape != shape:
            raise ValueError("depth shape %s != %s" % (depth.shape, shape))
        return depth

    def _contiguous(self, pixels, flow, seg, seg_ndim, label_arg, strict):
        """A batch's uint8, float32 and label arrays as they are where they can go to the library so, else converted
        (``label_arg`` for the label maps) - or, ``strict`` (the name of a ``hold > 0`` submit), refused: a converted copy
        would not outlive the call."""
        if not (_is_ready(pixels, np.uint8) and _is_ready(flow, FLOW_DTYPES[self.flow]) and _is_ready(seg, LABEL_DTYPES[self.labels]) and seg.ndim == seg_ndim):
            if strict:
                raise ValueError("%s(hold > 0) needs C-contiguous uint8 / %s / %s arrays (a converted copy would not outlive the call)"
                                 % (strict, FLOW_DTYPES[self.flow], LABEL_DTYPES[self.labels]))
            pixels, flow, seg = np.ascontiguousarray(pixels, np.uint8), self._f16_arg(flow, "flow"), label_arg(seg)
        return pixels, flow, seg

    def _window_batch(self, img, flow, seg, depth, strict=None, calibration=False):
        """A window-layout batch as the caller handed it -> (img, flow, seg), depth or None, B: checked and C-contiguous."""
        inputs = self._contiguous(img, flow, seg, 5, self._label_arg, strict)
        B = self._check_batch(*inputs, calibration=calibration)
        return inputs, self._depth_arg(depth, (B, 3, self.H, self.W, 1), "image, flow, seglabel", strict), B

    def _frame_batch(self, frames, flow2, seg, depth, strict=None):
        """A frame-layout batch as the caller handed it -> (frames, flow2, seg), depth or None, N: checked and C-contiguous."""
        inputs = self._contiguous(frames, flow2, seg, 4, self._frame_label_arg, strict)
        N = self._check_frames(*inputs)
        return inputs, self._depth_arg(depth, (N + 2, self.H, self.W, 1), "frames, flow2, seg", strict), N

    def _call(self, name, n, inputs, depth, *tail, depth_slot=False):
        """``name``(ctx, n, *inputs[, depth], *tail), checked.  An entry point either has a depth slot whatever the variant
        (``depth_slot``: the `_frames', feature and heat calls; None = NULL) or comes in a plain and a `_depth' form, chosen here
        by ``depth``.  numpy arrays and DeviceBuffers go as their pointers, everything else as it is."""
        if depth_slot or depth is not None:
            inputs, name = tuple(inputs) + (depth,), name if depth_slot else name + "_depth"
        self._check(getattr(self._L, name)(self._ctx, int(n), *map(_ptr, inputs), *map(_ptr, tail)))

    def forward(self, img, flow, seg, depth=None):
        inputs, depth, B = self._window_batch(img, flow, seg, depth)
        out = np.empty((B, 2, 6), np.float32)
        self._call("davo_forward", B, inputs, depth, out)
        return out

    FEATURE_OUTPUTS = ("att_19", "attention", "masked_image", "image", "feat_rot", "feat_trans")

    def set_feature_export(self, on=True):
        """Allocate (or free) the workspace of forward_features (include/davo_hip.h: davo_set_feature_export); off by default."""
        self._check(self._L.davo_set_feature_export(self._ctx, int(bool(on))))

    HEAT_OUTPUTS = ("heat_rot", "heat_trans", "max_rot", "max_trans")

    def set_heat_export(self, on=True):
        """Allocate (or free) the workspace of forward_features' heat outputs (include/davo_hip.h: davo_set_heat_export); off by
        default, independent of set_feature_export."""
        self._check(self._L.davo_set_heat_export(self._ctx, int(bool(on))))

    def forward_features(self, img, flow, seg, depth=None, want=FEATURE_OUTPUTS):
        """forward() plus the tensors of the reference's mode='feature' fetches from the same forward (include/davo_hip.h:
        davo_forward_features; needs set_feature_export() and the 'both' pair selection).  -> {'pose': [B,2,6]} and, for each
        name in ``want``: 'att_19' [3,B,19], 'attention' [3,B,H,W], 'masked_image' and 'image' [3,B,H,W,3] - frames in the
        order tgt, src0, src1 - 'feat_rot' and 'feat_trans' [B,H,W,cnv6_out]; all float32.  An output that is not wanted is
        neither computed nor copied.
        ``want`` may also name HEAT_OUTPUTS (davo_forward_heat; needs set_heat_export()): 'heat_rot' / 'heat_trans' [B,H,W], the
        channel sum of feat_rot / feat_trans reduced on the device, and 'max_rot' / 'max_trans' [B], their maxima."""
        unknown = [w for w in want if w not in self.FEATURE_OUTPUTS and w not in self.HEAT_OUTPUTS]
        if unknown:
            raise ValueError("unknown feature output(s) %s: choose from %s" % (unknown, list(self.FEATURE_OUTPUTS)))
        inputs, depth, B = self._window_batch(img, flow, seg, depth)
        H, W, c6 = self.H, self.W, self.cfg.cnv6_out
        shapes = {"att_19": (3, B, 19), "attention": (3, B, H, W), "masked_image": (3, B, H, W, 3), "image": (3, B, H, W, 3),
                  "feat_rot": (B, H, W, c6), "feat_trans": (B, H, W, c6),
                  "heat_rot": (B, H, W), "heat_trans": (B, H, W), "max_rot": (B,), "max_trans": (B,)}
        res = {"pose": np.empty((B, 2, 6), np.float32)}
        for name in self.FEATURE_OUTPUTS + self.HEAT_OUTPUTS:
            if name in want:
                res[name] = np.empty(shapes[name], np.float32)
        out = _lib.DavoFeatureOut(*[res[n].ctypes.data if n in res else None for n in self.FEATURE_OUTPUTS])
        if any(n in res for n in self.HEAT_OUTPUTS):
            heat = _lib.DavoHeatOut(*[res[n].ctypes.data if n in res else None for n in self.HEAT_OUTPUTS])
            self._call("davo_forward_heat", B, inputs, depth, res["pose"], ctypes.byref(out), ctypes.byref(heat), depth_slot=True)
        else:
            self._call("davo_forward_features", B, inputs, depth, res["pose"], ctypes.byref(out), depth_slot=True)
        return res

    def _check_batch(self, img, flow, seg, calibration=False):
        B = img.shape[0]
        want = ((B, self.H, 3 * self.W, 3), (B, 4, self.H, self.W, 2), (B, 3, self.H, self.W, 1))
        got = (img.shape, flow.shape, seg.shape)
        if got != want:
            if calibration:
                raise ValueError("calibration batch shapes %s %s %s do not match the engine" % got)
            raise ValueError(next("%s shape %s != %s" % t for t in zip(("img", "flow", "seg"), got, want) if t[1] != t[2]))
        return B

    def submit(self, img, flow, seg, out, hold=0, depth=None):
        """Streaming form of forward (include/davo_hip.h: davo_submit): issue the batch and return; ``out`` - a C-contiguous
        float32 [B,2,6] array the caller keeps alive - receives the poses when the batch is delivered (a later submit, wait()
        or synchronize()).  On return the input arrays of the batch submitted ``hold`` calls ago may be overwritten.
        ``depth``: the depth planes of a depth-source variant (davo_submit_depth), held like the other inputs."""
        inputs, depth, B = self._window_batch(img, flow, seg, depth, strict="submit" if hold else None)
        self._check_out(out, B)
        self._call("davo_submit", B, inputs, depth, out, int(hold))

    @staticmethod
    def _check_out(out, B):
        if not (_is_ready(out, np.float32) and out.shape == (B, 2, 6)):
            raise ValueError("out must be a C-contiguous float32 array of shape (%d, 2, 6)" % B)

    # ---- frame layout (include/davo_hip.h "Frame sequences"; davo_amd/frames.py) -------------------------------------
    def _frame_label_arg(self, seg):
        """The label maps of a frame-layout batch: C-contiguous [N+2,H,W,1] of the engine's format.  As _label_arg: a byte array
        handed to a float32 engine, or anything but bytes to a byte engine, is a ValueError; nothing is converted silently."""
        dt = np.asarray(seg).dtype
        if self.labels == "u8" and dt != np.uint8:
            raise ValueError("this engine takes uint8 label maps (labels='u8'), got dtype %s: convert with davo_amd.labels_to_u8" % dt)
        if self.labels != "u8" and dt == np.uint8:
            raise ValueError("this engine takes float32 label maps (labels='f32'), got uint8: create it with labels='u8'")
        seg = np.ascontiguousarray(seg, LABEL_DTYPES[self.labels])
        return seg[..., None] if seg.ndim == 3 else seg

    def _check_frames(self, frames, flow2, seg):
        N = flow2.shape[0]
        if frames.shape != (N + 2, self.H, self.W, 3):
            raise ValueError("frames shape %s != %s" % (frames.shape, (N + 2, self.H, self.W, 3)))
        if flow2.shape != (N, 2, self.H, self.W, 2):
            raise ValueError("flow2 shape %s != %s" % (flow2.shape, (N, 2, self.H, self.W, 2)))
        if seg.shape != (N + 2, self.H, self.W, 1):
            raise ValueError("seg shape %s != %s" % (seg.shape, (N + 2, self.H, self.W, 1)))
        return N

    def forward_frames(self, frames, flow2, seg, depth=None):
        """forward() on the frame layout (include/davo_hip.h: davo_forward_frames): ``frames`` u8 [N+2,H,W,3], ``flow2`` f32
        [N,2,H,W,2], ``seg`` [N+2,H,W,1] in the engine's label format, ``depth`` f32 [N+2,H,W,1] for a depth-source variant;
        window n is frames (n, n+1, n+2).  -> [N,2,6], the bits of forward() on davo_amd.windows_from_frames of the same arrays."""
        inputs, depth, N = self._frame_batch(frames, flow2, seg, depth)
        out = np.empty((N, 2, 6), np.float32)
        self._call("davo_forward_frames", N, inputs, depth, out, depth_slot=True)
        return out

    def submit_frames(self, frames, flow2, seg, out, hold=0, depth=None):
        """submit() on the frame layout (include/davo_hip.h: davo_submit_frames; shapes as forward_frames).  ``out`` [N,2,6] and
        ``hold`` as submit's; window and frame submits count alike."""
        inputs, depth, N = self._frame_batch(frames, flow2, seg, depth, strict="submit_frames" if hold else None)
        self._check_out(out, N)
        self._call("davo_submit_frames", N, inputs, depth, out, int(hold), depth_slot=True)

    def forward_device_frames(self, N, d_frames, d_flow2, d_seg, d_pose, timed=False, depth=None):
        """forward_device() on the frame layout (include/davo_hip.h: davo_forward_device_frames): DeviceBuffers of frames
        [N+2,H,W,3], flow2 [N,2,H,W,2], label maps [N+2,H,W,1] and - a depth-source variant - ``depth`` [N+2,H,W,1].  The timed
        form's milliseconds include the gather."""
        return self._call_device("davo_forward_device_frames", N, (d_frames, d_flow2, d_seg), depth, d_pose, timed, "frames, flow2, seg", depth_slot=True)

    def _call_device(self, name, n, bufs, depth, d_pose, timed, names, depth_slot=False):
        """The device entry points' checks and call: the label maps' DeviceBuffer holds the engine's format (where it knows), a
        depth-source variant gets its depth planes (any other ignores them).  -> milliseconds of the timed form, else None."""
        d_flow, d_seg = bufs[1], bufs[2]
        if getattr(d_flow, "dtype", None) is not None and (d_flow.dtype == np.float16) != (self.flow == "f16"):
            raise ValueError("d_flow holds %s flow, this engine takes flow='%s'" % (d_flow.dtype, self.flow))
        if getattr(d_seg, "dtype", None) is not None and (d_seg.dtype == np.uint8) != (self.labels == "u8"):
            raise ValueError("d_seg holds %s label maps, this engine takes labels='%s'" % (d_seg.dtype, self.labels))
        if self.cfg.needs_depth and depth is None:
            raise ValueError("%s and depth inputs are all required for version `%s'" % (names, self.cfg.version))
        if self.cfg.needs_depth and getattr(depth, "dtype", None) is not None and (depth.dtype == np.float16) != (self.depth == "f16"):
            raise ValueError("depth holds %s depth planes, this engine takes depth='%s'" % (depth.dtype, self.depth))
        ms = ctypes.c_float(0.0)
        self._call(name, n, bufs, depth if depth_slot or self.cfg.needs_depth else None, d_pose, ctypes.byref(ms) if timed else None, depth_slot=depth_slot)
        return ms.value if timed else None

    # ---- online tracking (include/davo_hip.h "Online tracking"; davo_amd/track.py: Tracker) --------------------------
    TRACK_POLICIES = {"trajectory": _lib.TRACK_TRAJECTORY, "as_set": _lib.TRACK_AS_SET}

    def track_begin(self, lanes=1, policy="trajectory"):
        """Open a tracking session of ``lanes`` video streams in lockstep (davo_track_begin).  ``policy``: "trajectory" - the
        first window both pairs, then tgt->src1 alone - or "as_set" - whatever set_pairs holds at each push."""
        if policy not in self.TRACK_POLICIES:
            raise ValueError("policy must be 'trajectory' or 'as_set', got %r" % (policy,))
        self._check(self._L.davo_track_begin(self._ctx, int(lanes), self.TRACK_POLICIES[policy]))
        self._track_lanes, self._track_held = int(lanes), collections.deque()

    def _track_issued(self, rc):
        if rc < 0:
            self._check(rc)
        return rc

    def track_push(self, frames, flow2, seg, out, hold=0, depth=None):
        """One new frame per lane (davo_track_push): ``frames`` u8 [S,H,W,3], ``flow2`` [S,2,H,W,2] the flow planes (tgt->src0,
        tgt->src1) of the window the frame completes, ``seg`` [S,H,W,1], ``depth`` [S,H,W,1] for a depth-source variant, in the
        engine's formats; ``out`` [S,2,6] and ``hold`` as submit's.  The first two pushes of a session read neither ``flow2`` nor
        ``out`` (None is fine).  -> windows issued: S, or 0 for those two.  The engine keeps ``out`` and - with ``hold`` - the
        inputs referenced until the push has been delivered."""
        S = getattr(self, "_track_lanes", None)
        if S is None:
            raise DavoError("track_push: no tracking session is open: call track_begin first")
        warm = self.track_frames() < 2
        if warm and flow2 is None:
            flow2 = np.zeros((S, 2, self.H, self.W, 2), FLOW_DTYPES[self.flow])
        strict = "track_push" if hold and not warm else None
        frames, flow2, seg = self._contiguous(frames, flow2, seg, 4, self._frame_label_arg, strict)
        want = ((S, self.H, self.W, 3), (S, 2, self.H, self.W, 2), (S, self.H, self.W, 1))
        for name, a, w in zip(("frames", "flow2", "seg"), (frames, flow2, seg), want):
            if a.shape != w:
                raise ValueError("%s shape %s != %s" % (name, a.shape, w))
        depth = self._depth_arg(depth, (S, self.H, self.W, 1), "frames, flow2, seg", strict)
        if not warm:
            self._check_out(out, S)
        n = self._track_issued(self._L.davo_track_push(self._ctx, _ptr(frames), _ptr(flow2), _ptr(seg), _ptr(depth), _ptr(out) if not warm else None, int(hold)))
        if n:
            self._track_held.append((out, (frames, flow2, seg, depth) if hold else None))
            while len(self._track_held) > max(self.pending(), int(hold) + 1):
                self._track_held.popleft()
        return n

    def track_push_device(self, d_frames, d_flow2, d_seg, d_pose, timed=False, depth=None):
        """track_push from DeviceBuffers (davo_track_push_device; 16-byte aligned, never written).  -> (windows issued,
        milliseconds of the timed form or None)."""
        ms = ctypes.c_float(0.0)
        n = self._track_issued(self._L.davo_track_push_device(self._ctx, _ptr(d_frames), _ptr(d_flow2), _ptr(d_seg), _ptr(depth) if self.cfg.needs_depth else None,
                                                              _ptr(d_pose), ctypes.byref(ms) if timed else None))
        return n, (ms.value if timed else None)

    def track_frames(self):
        """Frames pushed per lane in the open session (davo_track_frames)."""
        return self._track_issued(self._L.davo_track_frames(self._ctx))

    def track_end(self):
        """Deliver what is pending and free the session's ring (davo_track_end)."""
        self._check(self._L.davo_track_end(self._ctx))
        self._track_lanes, self._track_held = None, collections.deque()

    def wait(self, leave_pending=0):
        """Deliver submitted batches until at most ``leave_pending`` are outstanding (include/davo_hip.h: davo_wait)."""
        self._check(self._L.davo_wait(self._ctx, int(leave_pending)))

    def pending(self):
        return self._L.davo_pending(self._ctx)

    LAYERS = ("cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6")

    def calibrate(self, img, flow, seg, depth=None):
        """Choose the power-of-two storage scales of the f16x3 activations from a sample batch
        (include/davo_hip.h: davo_calibrate; davo_calibrate_depth for a depth-source variant).  -> {layer: log2 scale}."""
        inputs, depth, B = self._window_batch(img, flow, seg, depth, calibration=True)
        bufs = [self.alloc(a.nbytes).upload(a) for a in inputs + (() if depth is None else (depth,))]
        shifts = (ctypes.c_int * 6)()
        try:
            self._call("davo_calibrate", B, bufs[:3], bufs[3] if depth is not None else None, shifts)
        finally:
            for b in bufs:
                b.free()
        return dict(zip(self.LAYERS, list(shifts)))

    def activation_range(self, reset=False):
        """-> ({layer: largest |activation| stored since the last reset}, {layer: log2 storage scale})."""
        mx, sh = (ctypes.c_float * 6)(), (ctypes.c_int * 6)()
        self._check(self._L.davo_activation_range(self._ctx, mx, sh, int(bool(reset))))
        return dict(zip(self.LAYERS, list(mx))), dict(zip(self.LAYERS, list(sh)))

    def range_stats(self):
        """{'recalibrations', 'f32_batches', 'reissued'}: what the f16x3 range recovery has done so far
        (include/davo_hip.h: davo_range_stats)."""
        a, b, c = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_longlong(0)
        self._check(self._L.davo_range_stats(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return {"recalibrations": a.value, "f32_batches": b.value, "reissued": c.value}

    def range_report(self):
        """What the range management last did, in words ('' if nothing): the verdict behind a re-calibration or a float32
        batch, or the weight tensor whose per-input-channel spread keeps the network on the float32 kernels."""
        return (self._L.davo_range_report(self._ctx) or b"").decode()

    def set_activation_shifts(self, shifts=None):
        """Install storage scales from an earlier calibrate() (dict or sequence of 6 ints; None = none)."""
        if shifts is None:
            self._check(self._L.davo_set_activation_shifts(self._ctx, None))
            return
        vals = [shifts[k] for k in self.LAYERS] if isinstance(shifts, dict) else list(shifts)
        self._check(self._L.davo_set_activation_shifts(self._ctx, (ctypes.c_int * 6)(*vals)))

    def reset_range_state(self):
        """Back to a new engine's range state: no storage scales, zeroed range records and counters, an empty range_report
        (include/davo_hip.h: davo_reset_range_state).  Between independent jobs on one engine - the sequences of one
        run_kitti_pose launch - so that a job computes what it would on an engine of its own.  range_stats() keeps counting."""
        self._check(self._L.davo_reset_range_state(self._ctx))

    def forward_device(self, B, d_img, d_flow, d_seg, d_pose, timed=False, depth=None):
        """``depth``: the DeviceBuffer of the depth planes, required by a depth-source variant (davo_forward_device_depth)."""
        return self._call_device("davo_forward_device", B, (d_img, d_flow, d_seg), depth, d_pose, timed, "image, flow, seglabel")

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def synchronize(self):
        self._check(self._L.davo_synchronize(self._ctx))

    def set_option(self, key, value):
        """'auto_range' (default 1), 'fuse_pose' (default 1), 'fuse_pack' (default 0), 'host_chunk' (default 8), ...:
        see include/davo_hip.h."""
        self._check(self._L.davo_set_option(self._ctx, key.encode(), int(value)))
        if key == "host_chunk":
            self.host_chunk = int(value)

    def get_option(self, key):
        """The value the engine holds for ``key``, as set_option stored it (include/davo_hip.h: davo_get_option)."""
        v = ctypes.c_int()
        rc = self._L.davo_get_option(self._ctx, key.encode(), ctypes.byref(v))
        if rc != 0:
            raise _PY_ERR.get(rc, DavoError)("option `%s' cannot be read back: unknown, or kept per layer (\"force_tile\")" % key)
        return v.value

    def set_inflight(self, n):
        """Batches kept in flight by forward_device (1..4): n streams + n workspaces, rotated per call."""
        self._check(self._L.davo_set_inflight(self._ctx, int(n)))

    PAIRS = {"src0": 1, "src1": 2, "both": 3}

    def set_pairs(self, pairs):
        """Which of a window's two pairs the batches issued from now on run (include/davo_hip.h: davo_set_pairs): 'both'
        (default), 'src0' (tgt->src0 only) or 'src1' (tgt->src1 only - all that a trajectory needs of every window but a
        sequence's first, test_kitti_pose.py:143-145).  Outputs stay [B,2,6]; the row that was not selected is exactly zero.
        Batches in flight, and their range-recovery re-issues, keep the selection they were issued with."""
        if pairs not in self.PAIRS:
            raise ValueError("pairs must be 'both', 'src0' or 'src1', got %r" % (pairs,))
        self._check(self._L.davo_set_pairs(self._ctx, self.PAIRS[pairs]))

    @property
    def pairs(self):
        v = self._L.davo_get_pairs(self._ctx)
        for name, code in self.PAIRS.items():
            if code == v:
                return name
        raise DavoError("davo_get_pairs returned %d" % v)

    def set_flip(self, on):
        """Mirror the inputs of the batches issued from now on left-right, on the device (include/davo_hip.h: davo_set_flip): the
        engine then computes on X what it computes with flip off on ``davo_amd.flip_windows(X)`` (``flip_frames`` for the frame
        layout), bit for bit.  Off by default; may be switched between batches at any time, batches in flight keep theirs."""
        if on not in (0, 1, False, True):
            raise ValueError("flip must be True or False, got %r" % (on,))
        self._check(self._L.davo_set_flip(self._ctx, int(on)))

    @property
    def flip(self):
        return bool(self._L.davo_get_flip(self._ctx))

    def set_impl(self, impl):
        self._check(self._L.davo_set_impl(self._ctx, {"mfma": 0, "direct": 1}.get(impl, impl)))

    def set_precision(self, precision):
        """'f16x3' (default: split-fp16 MFMA, float32-grade) or 'f32' (FP32 MFMA, bit-exact fmaf chains)."""
        self._check(self._L.davo_set_precision(self._ctx, {"f32": 0, "f16x3": 1}.get(precision, precision)))

    def profile(self, on):
        """0/False off, 1/True every kernel, 2 only the dominant kernel (main cnv6 launch)."""
        self._check(self._L.davo_profile_enable(self._ctx, int(on)))

    def profile_reset(self):
        self._check(self._L.davo_profile_reset(self._ctx))

    def profile_entries(self):
        out, i = {}, 0
        name = ctypes.create_string_buffer(64)
        n, ms = ctypes.c_int(0), ctypes.c_double(0.0)
        while self._L.davo_profile_entry(self._ctx, i, name, 64, ctypes.byref(n), ctypes.byref(ms)) == 0:
            out[name.value.decode()] = (n.value, ms.value)
            i += 1
        return out

    def profile_samples(self, name, cap=8192):
        """(durations_ms, periods_ms) of every bracketed launch of `name` since the last profile_reset, in issue order
        (include/davo_hip.h: davo_profile_samples); period = start of the previous bracketed launch to this one's start."""
        out = []
        for which in (0, 1):
            buf = (ctypes.c_float * cap)()
            n = self._L.davo_profile_samples(self._ctx, name.encode(), which, buf, cap)
            if n < 0:
                self._check(n)
            out.append(np.array(buf[:min(n, cap)], np.float32))
        return out[0], out[1]

    def last_plan(self, layer):
        """[(mtiles, BN), ...] of the launches the last forward used for conv layer 0..6."""
        out = []
        for k in (0, 1):
            m, bn = ctypes.c_int(0), ctypes.c_int(0)
            self._check(self._L.davo_last_plan(self._ctx, layer, k, ctypes.byref(m), ctypes.byref(bn)))
            if m.value:
                out.append((m.value, bn.value))
        return out

    def last_split(self, layer):
        """Split-K parts of conv layer 0..6's launch in the last forward (1: a single chain over K)."""
        s = ctypes.c_int(0)
        self._check(self._L.davo_last_split(self._ctx, layer, ctypes.byref(s)))
        return s.value

    def debug_read(self, tensor, shape):
        out = np.empty(shape, np.float32)
        self._check(self._L.davo_debug_read(self._ctx, tensor.encode(), out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), out.size))
        return out


def conv2d_same(x, w, b, stride=1, rate=1, relu=True, device=0, precision="f32"):
    """slim.conv2d(padding='SAME') through the MFMA implicit-GEMM kernel (test hook)."""
    x = np.ascontiguousarray(x, np.float32); w = np.ascontiguousarray(w, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    N, H, W, Cin = x.shape
    k, k2, ci, Cout = w.shape
    if k != k2 or ci != Cin:
        raise ValueError("weights %s do not fit input %s" % (w.shape, x.shape))
    y = np.empty((N, -(-H // stride), -(-W // stride), Cout), np.float32)
    err = ctypes.create_string_buffer(256)
    fp = ctypes.POINTER(ctypes.c_float)
    rc = _lib.lib().davo_conv2d_same(device, x.ctypes.data_as(fp), N, H, W, Cin, w.ctypes.data_as(fp), k, Cout,
                                     b.ctypes.data_as(fp), stride, rate, int(relu),
                                     {"f32": 0, "f16x3": 1}[precision], y.ctypes.data_as(fp), err, 256)
    if rc != 0:
        raise _PY_ERR.get(rc, DavoError)(err.value.decode())
    return y


def seg_one_hot(seg):
    """The reference's seg_19 (davo.py:1115: tf.one_hot(tf.cast(seg, int32), 19)) of label maps [..., 1] -> [..., 19] float32, by
    the rules the kernels' class gather follows: the cast truncates toward zero, and a label outside [0, 19) after it - or NaN or
    infinite, where the cast is platform-defined - selects no class: a zero row.  Byte label maps (uint8 [..., 1] or without the
    trailing axis) follow the same rule: a byte's value as a float selects the class the byte selects on the device."""
    seg = np.asarray(seg)
    seg = (seg if seg.dtype == np.uint8 and seg.ndim == 4 else seg[..., 0]).astype(np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(seg) & (seg > -1.0) & (seg < 19.0)
    idx = np.where(ok, seg, 0.0).astype(np.int32)
    return ((idx[..., None] == np.arange(19, dtype=np.int32)) & ok[..., None]).astype(np.float32)


def host_maps(cfg, img, seg, tables, depth=None, tables_far=None, thr=None):
    """The four map outputs of Engine.forward_features - 'att_19' [3,B,19], 'attention' [3,B,H,W], 'masked_image' and 'image'
    [3,B,H,W,3], frames tgt, src0, src1 - rebuilt on the host from a batch's inputs and the class tables its forward computed
    (Engine.debug_read("att_table"), [B,3,19]), in the kernels' float32 expressions (csrc/feature_export.h: feature_maps), so to
    the bit what the device exports.  DAVO's features='heat' mode uses it: the device-side maps live in the full export's
    workspace, which that mode never allocates.
    The depth-split flow attention (`-se_flow_on_depthseg_seplayers') also takes the batch's depth planes, the far tables
    (debug_read("att_table_far")) and the loaded threshold: a source pixel's weight comes from ``tables`` where
    float32(depth) < thr, else from ``tables_far`` (a NaN depth is far); 'att_19' is absent there - no single table was applied."""
    split = cfg.att_source == "se_flow_depthseg_sep"
    if split and (depth is None or tables_far is None or thr is None):
        raise ValueError("version `%s' needs depth, tables_far and thr" % cfg.version)
    img = np.asarray(img, np.uint8)
    seg = np.asarray(seg)
    seg = (seg[..., None] if seg.dtype == np.uint8 and seg.ndim == 4 else seg).astype(np.float32)      # bytes: the same class as floats
    tables = np.asarray(tables, np.float32)
    B, H, W3, _ = img.shape
    W = W3 // 3
    unit = (img.astype(np.float32) * np.float32(1.0 / 255.0)) * np.float32(2.0) - np.float32(1.0)      # davo.py:1521-1522
    a19 = np.ones((3, B, NUM_SEG_CLASSES), np.float32)
    att = np.ones((3, B, H, W), np.float32)
    image = np.empty((3, B, H, W, 3), np.float32)
    for f, plane in enumerate((1, 0, 2)):                      # (tgt, src0, src1) -> strip slot / label plane src0, tgt, src1
        image[f] = unit[:, :, plane * W:(plane + 1) * W]
        if cfg.tgt_attended if f == 0 else att_source_id(cfg.att_source) != 0:       # else the reference's tf.ones_like override
            a19[f] = tables[:, f]
            lab = seg[:, plane, :, :, 0]
            with np.errstate(invalid="ignore"):
                ok = np.isfinite(lab) & (lab > -1.0) & (lab < float(NUM_SEG_CLASSES))
            idx = np.where(ok, lab, 0.0).astype(np.int64).reshape(B, -1)
            looked = np.take_along_axis(a19[f], idx, axis=1).reshape(B, H, W)
            if split:
                far = np.take_along_axis(np.asarray(tables_far, np.float32)[:, f], idx, axis=1).reshape(B, H, W)
                with np.errstate(invalid="ignore"):
                    near = np.asarray(depth, np.float32)[:, plane, :, :, 0] < np.float32(thr)
                looked = np.where(near, looked, far)
            att[f] = np.where(ok, looked, np.float32(0.0))
    masked = image * att[..., None] if cfg.mask_rgb else image.copy()
    out = {"att_19": a19, "attention": att, "masked_image": masked, "image": image}
    if split:
        del out["att_19"]
    return out


class DAVO(object):
    """Drop-in for the reference class on the inference path (reference davo.py:30)."""

    def __init__(self, version=None, att_19=None, device=0, flip=False):
        """``flip``: mirror every batch left-right on the device (Engine.set_flip; include/davo_hip.h: davo_set_flip) - for a
        flip-trained checkpoint or the mirrored sequences (poses-flip); ``setup_inference(..., flip=...)`` overrides it."""
        self.version = version          # davo.py:32
        self.att_19 = att_19            # davo.py:33 (unused on the pose path)
        self.device = device
        self.engine = None
        self._weights = None
        self._feature_mode = False
        self._features = 'full'
        self._labels = "f32"
        self._flow = "f32"
        self._depth = "f32"
        self._flip = bool(flip)

    def use_f16_flow(self):
        """Opt in to binary16 flow (include/davo_hip.h: davo_set_flow_format): ``input_flow``, ``inference(inputs=...)`` and
        iterator inputs then carry float16 [B,4,H,W,2] (davo_amd.flow_to_f16 of the float32 flow) and float32 flow is refused.
        Before ``setup_inference`` - which also picks the format up by itself from a float16 ``input_flow``.  Returns self."""
        if self.engine is not None:
            raise DavoError("use_f16_flow() must be called before setup_inference")
        self._flow = "f16"
        return self

    def use_f16_depth(self):
        """Opt in to binary16 depth planes (include/davo_hip.h: davo_set_depth_format): ``input_depth``, ``inference(inputs=...)``
        and iterator inputs then carry float16 [B,3,H,W,1] (davo_amd.depth_to_f16 of the float32 planes) and float32 depth is
        refused.  Before ``setup_inference`` - which also picks the format up by itself from a float16 ``input_depth``.  A
        variant that reads no depth accepts the call.  Returns self."""
        if self.engine is not None:
            raise DavoError("use_f16_depth() must be called before setup_inference")
        self._depth = "f16"
        return self

    def use_u8_labels(self):
        """Opt in to byte label maps (include/davo_hip.h: davo_set_label_format): ``input_seglabel``, ``inference(inputs=...)`` and
        iterator inputs then carry uint8 [B,3,H,W,1] or [B,3,H,W] class ids (davo_amd.labels_to_u8 of the float maps) and float
        maps are refused.  Before ``setup_inference``.  Returns self."""
        if self.engine is not None:
            raise DavoError("use_u8_labels() must be called before setup_inference")
        self._labels = "u8"
        return self

    def enable_feature_mode(self, features='full'):
        """Opt in to ``inference(mode='feature')``: allocates the library's export workspace - now if ``setup_inference`` has
        run, else when it does.  Returns self.
        features='full' (include/davo_hip.h: davo_set_feature_export): 'features' holds the two resized cnv6 maps.
        features='heat' (davo_set_heat_export alone; the maps' workspace is never allocated): 'features' holds what
        generate_feature_map.py:204-265 reduces the maps to, computed on the device - see ``inference``."""
        if features not in ('full', 'heat'):
            raise ValueError("features must be 'full' or 'heat', got %r" % (features,))
        self._feature_mode = True
        self._features = features
        if self.engine is not None:
            self._switch_exports()
        return self

    def _switch_exports(self):
        if self._features == 'heat':
            self.engine.set_heat_export(True)
        else:
            self.engine.set_feature_export(True)

    def setup_inference(self, img_height, img_width, mode, seq_length=3, batch_size=1,
                        input_img_uint8=None, input_pose=None, input_flow=None, input_depth=None,
                        input_seglabel=None, flip=None):
        """davo.py:1533-1551.  ``input_*`` are numpy arrays ([B,H,3W,3] u8, [B,4,H,W,2] f32,
        [B,3,H,W,1] f32) or ``input_img_uint8`` is an iterator yielding (img, flow, seg) - (img, flow, seg, depth)
        for a depth-source variant; ``input_depth`` ([B,3,H,W,1] f32, file order src0, tgt, src1: davo.py:991-996) is
        kept for such a variant and ignored otherwise, ``input_pose`` is accepted and ignored, like the reference does.
        ``flip``: True / False mirrors the inputs on the device or not (Engine.set_flip); None keeps the constructor's choice.
        Every output of ``inference`` is then what a flip-off DAVO returns on ``davo_amd.flip_windows`` of the same inputs."""
        self.img_height, self.img_width, self.mode, self.batch_size = img_height, img_width, mode, batch_size
        if self.mode != 'davo':
            return                                        # davo.py:1548: other modes do nothing
        if seq_length != 3:
            raise ValueError("seq_length %d: the pose path is built for 3-frame windows" % seq_length)
        self.seq_length, self.num_source = seq_length, seq_length - 1
        assert self.version is not None                   # davo.py:959
        self.cfg = parse_version(self.version)
        if isinstance(input_flow, np.ndarray) and input_flow.dtype == np.float16:
            self._flow = "f16"                             # a float16 ``input_flow`` selects the binary16 flow format
        if isinstance(input_depth, np.ndarray) and input_depth.dtype == np.float16:
            self._depth = "f16"                            # a float16 ``input_depth`` selects the binary16 depth format
        self.engine = Engine(self.cfg, img_height, img_width, batch_size, self.device, labels=self._labels, flow=self._flow, depth=self._depth)
        if self._weights is not None:
            self.engine.load_weights(self._weights)
        if flip is not None:
            self._flip = bool(flip)
        if self._flip:
            self.engine.set_flip(True)
        if self._feature_mode:
            self._switch_exports()
        self._ahead = []                                   # iterator inputs: batches submitted and not returned yet
        if input_img_uint8 is not None and not isinstance(input_img_uint8, np.ndarray) and input_flow is None:
            self._inputs = iter(input_img_uint8)
            # the counterpart of the tf.data iterator the reference's graph pulls from (data_loader.py:321-324, prefetch): batches
            # go through the library's streaming entry point, so while inference() call n waits for its poses, batch n+1 is
            # already copied and running (two in flight on the GPU)
            self.engine.set_inflight(2)
        else:
            self._inputs = (input_img_uint8, input_flow, input_seglabel) + ((input_depth,) if self.cfg.needs_depth else ())

    def load_weights(self, weights):
        """Stand-in for tf.train.Saver(tf.trainable_variables()).restore (test_kitti_pose.py:129-131)."""
        self._weights = weights
        if self.engine is not None:
            self.engine.load_weights(weights)

    def calibrate(self, inputs):
        """Range-calibrate the f16x3 arithmetic on a sample batch (img, flow, seg[, depth]); see Engine.calibrate.  Optional:
        ``inference`` re-calibrates by itself on the first batch that leaves the range (the reference's float32
        graph has no counterpart and never fails, davo.py:1553-1569); calling it up front only saves that re-issue."""
        if self.engine is None:
            raise DavoError("setup_inference(..., mode='davo') has not been called")
        return self.engine.calibrate(*inputs)

    def inference(self, sess=None, mode='pose', inputs=None):
        """davo.py:1553-1569.  ``sess`` is accepted and ignored.
        mode='pose' -> {'pose': float32 [B,2,6]}.
        mode='feature' (after ``enable_feature_mode()``) -> the reference's dict, float32 throughout, lists in the frame order
        tgt, src0, src1:
          'pose'      [B,2,6], bit for bit mode='pose';
          'masks'     {'attention': 3 x [B,H,W,1], the maps multiplied in (after the tf.ones_like overrides);
                       'image': 3 x [B,H,W,3], the frames' rgb after masking (the plain rgb where the version masks none);
                       'att_19': 3 x [B,1,1,19], att_19[f][b,0,0,c] = the value frame f's map takes on class c - an empty list
                       for `-se_flow_on_depthseg_seplayers', where a pixel's weight comes from one of two tables by its depth
                       and the reference sets no att_19s (davo.py:1470)};
          'features'  {'rot', 'trans'}: [B,H,W,cnv6_out], resize_bilinear of the tgt->src1 call's cnv6 heads; after
                      ``enable_feature_mode(features='heat')`` instead {'rot_sum', 'trans_sum'}: [B,H,W], the maps' sum over
                      the channels; {'rot_avg', 'trans_avg'}: [B,H,W] = sum * (1 / cnv6_out), exact; {'rot_max', 'trans_max'}:
                      [B], the maps' maxima (generate_feature_map.py:249-263 draws these);
          'images'    3 x [B,H,W,3] preprocessed, unmasked;
          'seg_19'    3 x [B,H,W,19] one-hot label maps (built on the host, seg_one_hot).
        Deviations from the reference: 'att_19' is defined for every variant, and a frame whose map the reference overrides
        with ones reports 19 ones (the reference keeps an se() output there that nothing multiplies in and
        generate_feature_map.py never reads); 'flows' and 'segs' - colourings of the caller's own inputs - are not built, the
        keys are absent.  With iterator inputs a 'feature' call first waits for what 'pose' calls have in flight, then takes
        the iterator's next batch synchronously."""
        if mode == 'feature' and not self._feature_mode:
            raise NotImplementedError("mode `feature' is an opt-in: call enable_feature_mode() on this DAVO first (davo.py:1557-1569)")
        if mode not in ('pose', 'feature'):
            raise NotImplementedError("mode `%s': only 'pose' and 'feature' are built (davo.py:1555-1569)" % mode)
        if self.engine is None:
            raise DavoError("setup_inference(..., mode='davo') has not been called")
        if mode == 'feature':
            return self._inference_feature(inputs)
        if inputs is None and not isinstance(self._inputs, tuple):
            return {'pose': self._next_from_iterator()}
        img, flow, seg, depth = self._split(inputs if inputs is not None else self._inputs)
        if img is None or flow is None or seg is None:
            raise ValueError("image, flow and seglabel inputs are all required for version `%s'" % self.version)
        return {'pose': self.engine.forward(img, flow, seg, depth)}

    def _inference_feature(self, inputs):
        if inputs is None and not isinstance(self._inputs, tuple):
            self.engine.wait(0)                                # batches 'pose' calls submitted ahead: delivered into _ahead, in order
            inputs = next(self._inputs, None)
            if inputs is None:
                raise StopIteration("the input iterator is exhausted")
        img, flow, seg, depth = self._split(inputs if inputs is not None else self._inputs)
        if img is None or flow is None or seg is None:
            raise ValueError("image, flow and seglabel inputs are all required for version `%s'" % self.version)
        heat = self._features == 'heat'
        if self._flip:                                         # the parts rebuilt on the host (seg_19, the heat mode's maps) see what the device saw
            host_in = flip_windows(img, flow, seg, depth)
            seg_seen, depth_seen, img_seen = host_in[2], (host_in[3] if depth is not None else None), host_in[0]
        else:
            seg_seen, depth_seen, img_seen = seg, depth, img
        # the depth-split flow attention has no att_19 (include/davo_hip.h): the library is asked for the other members only
        split = self.cfg.att_source == "se_flow_depthseg_sep"
        want = tuple(n for n in Engine.FEATURE_OUTPUTS if not (split and n == "att_19"))
        r = self._forward_heat(img, flow, seg, depth, (img_seen, seg_seen, depth_seen)) if heat else self.engine.forward_features(img, flow, seg, depth, want=want)
        if heat:
            inv = np.float32(1.0 / self.cfg.cnv6_out)          # a power of two: the mean is exact
            features = {'rot_sum': r['heat_rot'], 'trans_sum': r['heat_trans'], 'rot_avg': r['heat_rot'] * inv,
                        'trans_avg': r['heat_trans'] * inv, 'rot_max': r['max_rot'], 'trans_max': r['max_trans']}
        else:
            features = {'rot': r['feat_rot'], 'trans': r['feat_trans']}
        one_hot = seg_one_hot(seg_seen)                         # [B,3,H,W,19], file order src0, tgt, src1 (davo.py:998-1004)
        return {'pose': r['pose'],
                'masks': {'attention': [r['attention'][f][..., None] for f in range(3)],
                          'image': [r['masked_image'][f] for f in range(3)],
                          'att_19': [] if split else [r['att_19'][f][:, None, None, :] for f in range(3)]},
                'features': features,
                'images': [r['image'][f] for f in range(3)],
                'seg_19': [one_hot[:, plane] for plane in (1, 0, 2)]}

    def _forward_heat(self, img, flow, seg, depth, seen):
        """Engine.forward_features' dict with the heat outputs in place of the two feature maps.  The device delivers the poses,
        planes and maxima (davo_forward_heat); the four maps are rebuilt by ``host_maps`` from the class tables of the forward,
        which the context holds for one sub-batch: a batch that davo_forward would split (2 x host_chunk windows or more) is
        issued here as those sub-batches, one call each - the same forwards, so the same poses (a range recovery then re-issues
        a sub-batch, not the batch).  ``seen``: (img, seg, depth) as the device read them - mirrored with flip on."""
        e = self.engine
        seen = [None if a is None else np.asarray(a) for a in seen]
        img, flow, seg = np.asarray(img), np.asarray(flow), np.asarray(seg)
        depth = None if depth is None else np.asarray(depth)
        B = img.shape[0]
        step = e.host_chunk if e.host_chunk > 0 and B >= 2 * e.host_chunk else B
        parts = []
        for b0 in range(0, B, step):
            part = [None if a is None else a[b0:b0 + step] for a in (img, flow, seg, depth)]
            r = e.forward_features(*part, want=Engine.HEAT_OUTPUTS)
            s_img, s_seg, s_depth = [None if a is None else a[b0:b0 + step] for a in seen]
            tab_shape = (len(part[0]), 3, NUM_SEG_CLASSES)
            if self.cfg.att_source == "se_flow_depthseg_sep":
                r.update(host_maps(self.cfg, s_img, s_seg, e.debug_read("att_table", tab_shape), depth=s_depth,
                                   tables_far=e.debug_read("att_table_far", tab_shape), thr=self._weights[DEPTH_THRESHOLD]))
            else:
                r.update(host_maps(self.cfg, s_img, s_seg, e.debug_read("att_table", tab_shape)))
            parts.append(r)
        if len(parts) == 1:
            return parts[0]
        frame_major = ("att_19", "attention", "masked_image", "image")      # (no att_19 for the depth-split flow attention)
        return {k: np.concatenate([p[k] for p in parts], axis=1 if k in frame_major else 0) for k in parts[0]}

    def _split(self, inputs):
        """(img, flow, seg) or, for a depth-source variant, (img, flow, seg, depth) -> the four, depth None without it."""
        inputs = tuple(inputs)
        if self.cfg.needs_depth:
            if len(inputs) != 4 or inputs[3] is None:
                raise ValueError("image, flow, seglabel and depth inputs are all required for version `%s'" % self.version)
            return inputs
        img, flow, seg = inputs[:3] if len(inputs) == 4 else inputs      # a fourth array is ignored like the reference's depth input
        return img, flow, seg, None

    def _next_from_iterator(self):
        """Poses of the iterator's next batch; the batch after it is submitted before this one is waited for.  A batch the
        iterator yields must stay valid until the iterator is asked for the next one (davo_amd.loader's contract)."""
        while len(self._ahead) < 2:
            item = next(self._inputs, None)
            if item is None:
                break
            img, flow, seg, depth = self._split(item)
            out = np.empty((np.shape(img)[0], 2, 6), np.float32)
            self.engine.submit(img, flow, seg, out, depth=depth)       # hold = 0: the batch is copied when this returns
            self._ahead.append(out)
        if not self._ahead:
            raise StopIteration("the input iterator is exhausted")      # tf.errors.OutOfRangeError's counterpart
        out = self._ahead.pop(0)
        self.engine.wait(len(self._ahead))
        return out
