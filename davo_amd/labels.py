"""The label formats of the library (include/davo_hip.h: davo_set_label_format) and the one host-side definition of the rule
that turns the reference's float32 label maps into bytes.  numpy only: loader workers import it without loading the HIP library.

A label map is a class id per pixel; the network and the exports read no more of it than "class 0..18, or none" (the kernels'
att_lookup, csrc/input_decode.h).  The reference's preprocessing stores it as float32 (data_loader.py:313-317); DeepLab writes
bytes."""
import numpy as np

NUM_CLASSES = 19
NO_CLASS = 255                       # what labels_to_u8 writes for "no class"; on the device every byte >= 19 means it
LABEL_FORMATS = {"f32": 0, "u8": 1}  # DAVO_LABELS_F32, DAVO_LABELS_U8
LABEL_DTYPES = {"f32": np.dtype(np.float32), "u8": np.dtype(np.uint8)}


def check_label_format(labels):
    if labels not in LABEL_FORMATS:
        raise ValueError("labels must be 'f32' or 'u8', got %r" % (labels,))
    return labels


def labels_to_u8(seg_f32):
    """att_lookup's rule folded into a byte: a finite value in (-1, 19) becomes its truncation toward zero (-0.5 -> 0,
    18.9 -> 18); everything else - NaN, +-inf, <= -1, >= 19 - becomes 255.  The class a byte L selects on the device (row L
    when L < 19, none otherwise) is then the class the float selects, for every float: the conversion loses nothing the
    network or the exports compute.  Same shape as the input, dtype uint8."""
    seg = np.asarray(seg_f32, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (seg > np.float32(-1.0)) & (seg < np.float32(NUM_CLASSES))      # false for NaN; no infinity passes both
    return np.where(ok, np.trunc(np.where(ok, seg, np.float32(0.0))), np.float32(NO_CLASS)).astype(np.uint8)
