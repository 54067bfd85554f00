"""The pooled flow-attention variants' window geometry (att_source 14..17) as the library plans it: ``davo_pool_plan`` of
include/davo_hip.h, pure host logic - no context, no device."""
import ctypes

import numpy as np

from . import _lib
from .version import att_source_id


def pool_plan(H, W, att_source):
    """-> (rects int32 [n,4], inv_div float32 [n]): per cell of the SE descriptor of an H x W frame, in descriptor order, rows
    [y0, y1) and columns [x0, x1) cut to the real image (zeros for a cell wholly in padding) and the reciprocal divisor of its
    mean.  ``att_source``: a name of davo_amd.version.ATT_SOURCE / POOLED_ATT_SOURCE or its number; n = 0 for a source that does not pool."""
    att = att_source_id(att_source) if isinstance(att_source, str) else int(att_source)
    L = _lib.lib()
    n = ctypes.c_int(0)
    if L.davo_pool_plan(H, W, att, ctypes.byref(n), None, None) != 0:
        raise ValueError("davo_pool_plan(%r) refused its arguments" % ((H, W, att_source),))
    rects = np.zeros((n.value, 4), np.int32)
    inv = np.zeros((n.value,), np.float32)
    if n.value:
        rc = L.davo_pool_plan(H, W, att, ctypes.byref(n), rects.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                              inv.ctypes.data_as(ctypes.POINTER(ctypes.c_float)))
        assert rc == 0 and n.value == rects.shape[0]
    return rects, inv
