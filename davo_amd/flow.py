"""The flow formats of the library (include/davo_hip.h: davo_set_flow_format) and the one host-side definition of the rule that
turns float32 optical flow into IEEE binary16.  numpy only: loader workers import it without loading the HIP library.

The flow is what FlowNet2 estimates, to about a pixel; binary16 keeps 11 significant bits (a rounding error of at most 2^-12
relative: under 0.004 px at 15 px).  The kernels widen every half exactly (csrc/input_decode.h: flow_fetch4, widen_fetch4), so a binary16
engine on ``h`` computes the bits of a float32 engine on ``flow_from_f16(h)``."""
import numpy as np

FLOW_FORMATS = {"f32": 0, "f16": 1}  # DAVO_FLOW_F32, DAVO_FLOW_F16
FLOW_DTYPES = {"f32": np.dtype(np.float32), "f16": np.dtype(np.float16)}
F16_MAX = np.float32(65504.0)        # the largest finite binary16


def check_flow_format(flow):
    if flow not in FLOW_FORMATS:
        raise ValueError("flow must be 'f32' or 'f16', got %r" % (flow,))
    return flow


def to_f16(x):
    """The one float32 -> binary16 rule of the inputs (flow_to_f16 here, depth_to_f16 in davo_amd/depth.py), same shape: round to
    nearest even, finite values clipped to +-65504, NaN, infinities and the sign of zero kept."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        clipped = np.where(np.isinf(x), x, np.clip(x, -F16_MAX, F16_MAX))      # (np.clip keeps NaN)
        return clipped.astype(np.float16)


def from_f16(h, name="from_f16"):
    """The widening twin of to_f16: binary16 -> the float32 of the same value, exact for every half.  ``name``: the caller's
    name for the error text."""
    h = np.asarray(h)
    if h.dtype != np.float16:
        raise ValueError("%s takes a float16 array, got %s" % (name, h.dtype))
    return h.astype(np.float32)


def flow_to_f16(flow):
    """float32 flow -> binary16, same shape: round to nearest even; a finite value beyond +-65504 becomes +-65504 (binary16
    would round 65520 and more to infinity: a finite flow stays finite); NaN stays NaN, an infinity stays that infinity, a
    zero keeps its sign, and what is too small for a normal half becomes a subnormal or a signed zero by the same rounding."""
    return to_f16(flow)


def flow_from_f16(flow_f16):
    """The widening twin: binary16 -> the float32 of the same value, exact for every half (NaN stays NaN).  What the kernels of
    a binary16 engine compute on, and what a float32 engine must be given to compute the same bits."""
    return from_f16(flow_f16, "flow_from_f16")
