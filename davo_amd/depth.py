"""The depth formats of the library (include/davo_hip.h: davo_set_depth_format) and the one host-side definition of the rule that
turns float32 depth planes into IEEE binary16.  numpy only: loader workers import it without loading the HIP library.

The depth planes are a monocular network's estimate (monodepth2), good to a few percent; binary16 keeps 11 significant bits (a
rounding error of at most 2^-12 relative; at the depth-split attention's 15 m default threshold a half is 2^-7 m wide).  The
kernels widen every half exactly (csrc/input_decode.h: widen_fetch4), so a binary16 engine on ``h`` computes the bits of a float32
engine on ``depth_from_f16(h)``.  The rounding rule is the flow's (davo_amd/flow.py: to_f16)."""
import numpy as np

from .flow import F16_MAX, from_f16, to_f16  # noqa: F401

DEPTH_FORMATS = {"f32": 0, "f16": 1}  # DAVO_DEPTH_F32, DAVO_DEPTH_F16
DEPTH_DTYPES = {"f32": np.dtype(np.float32), "f16": np.dtype(np.float16)}


def check_depth_format(depth):
    if depth not in DEPTH_FORMATS:
        raise ValueError("depth must be 'f32' or 'f16', got %r" % (depth,))
    return depth


def depth_to_f16(depth):
    """float32 depth -> binary16, same shape: round to nearest even; a finite value beyond +-65504 becomes +-65504 (binary16
    would round 65520 and more to infinity: a finite depth stays finite); NaN stays NaN, an infinity stays that infinity, a
    zero keeps its sign, and what is too small for a normal half becomes a subnormal or a signed zero by the same rounding."""
    return to_f16(depth)


def depth_from_f16(depth_f16):
    """The widening twin: binary16 -> the float32 of the same value, exact for every half (NaN stays NaN).  What the kernels of
    a binary16 engine compute on, and what a float32 engine must be given to compute the same bits."""
    return from_f16(depth_f16, "depth_from_f16")
