"""Float64 restatement of the feature export (include/davo_hip.h: davo_forward_features), what DAVO.inference(sess,
mode='feature') returns beside the poses (reference davo.py:1553-1569).  Imported by tests/test_feature_export.py (its own
properties, CPU) and tests/test_feature_export_gpu.py (the library against it); the library never calls it.

Frames are in the order tgt, src0, src1; the label maps and depth planes come in file order src0, tgt, src1 (davo.py:998-1004),
the strip as src0 | tgt | src1 (data_loader.py:537-557)."""
import numpy as np

from davo_amd.version import ATT_SOURCE, NUM_SEG_CLASSES

FILE_PLANE = (1, 0, 2)          # frame (tgt, src0, src1) -> plane of seg / depth, slot of the strip


# ---- the resize: TF 1.13 resize_bilinear, align_corners=False, no half-pixel centres, at scale 1/4 ------------------------------
def _axis(n_in):
    """For the 4 n_in outputs of one axis: lo, hi = min(lo + 1, n_in - 1), lerp = (out & 3) / 4 (in = out / 4 exactly)."""
    out = np.arange(4 * n_in)
    lo = out >> 2
    return lo, np.minimum(lo + 1, n_in - 1), (out & 3) / 4.0


def resize_x4(x):
    """[N,h,w,C] -> [N,4h,4w,C] float64 in TF's order per value: top = tl + (tr - tl) xl, bot = bl + (br - bl) xl,
    out = top + (bot - top) yl."""
    x = np.asarray(x, np.float64)
    ylo, yhi, yl = _axis(x.shape[1])
    xlo, xhi, xl = _axis(x.shape[2])
    xl = xl[None, None, :, None]
    rows_t, rows_b = x[:, ylo], x[:, yhi]
    top = rows_t[:, :, xlo] + (rows_t[:, :, xhi] - rows_t[:, :, xlo]) * xl
    bot = rows_b[:, :, xlo] + (rows_b[:, :, xhi] - rows_b[:, :, xlo]) * xl
    return top + (bot - top) * yl[None, :, None, None]


def resize_matrix(n_in):
    """[4 n_in, n_in]: the same weights as one matrix per axis (row o: 1 - lerp on lo, lerp on hi)."""
    lo, hi, l = _axis(n_in)
    m = np.zeros((4 * n_in, n_in))
    np.add.at(m, (np.arange(4 * n_in), lo), 1.0 - l)
    np.add.at(m, (np.arange(4 * n_in), hi), l)
    return m


def resize_x4_separable(x):
    x = np.asarray(x, np.float64)
    return np.einsum("yi,nijc,xj->nyxc", resize_matrix(x.shape[1]), x, resize_matrix(x.shape[2]))


def corner_max(x):
    """[N,4h,4w,C]: max(|tl|, |tr|, |bl|, |br|) of every output element - what the resize's float32 error is relative to."""
    a = np.abs(np.asarray(x, np.float64))
    ylo, yhi, _ = _axis(a.shape[1])
    xlo, xhi, _ = _axis(a.shape[2])
    t, b = a[:, ylo], a[:, yhi]
    return np.maximum(np.maximum(t[:, :, xlo], t[:, :, xhi]), np.maximum(b[:, :, xlo], b[:, :, xhi]))


def features(cnv6, c6):
    """cnv6 [2B,h,w,2 c6] of a both-pairs forward -> (rot, trans) [B,4h,4w,c6]: the second PoseNN call (pair image 2b + 1),
    rotation = channels [0, c6), translation = [c6, 2 c6) (davo.py:1457,1463-1465)."""
    second = np.asarray(cnv6)[1::2]
    return resize_x4(second[..., :c6]), resize_x4(second[..., c6:2 * c6])


# ---- the maps -----------------------------------------------------------------------------------------------------
def looked_up(cfg, frame):
    """Does the forward gather frame's map from a class table?  Otherwise the reference overrides it with tf.ones_like
    (davo.py:1387,1394,1218): every frame under -no_segmask, the target unless the variant attends it."""
    return cfg.tgt_attended if frame == 0 else ATT_SOURCE[cfg.att_source] != 0


def att_19(cfg, tables):
    """tables [B,3,19] (what the forward computed; rows of overridden frames are ignored) -> [3,B,19]."""
    tables = np.asarray(tables)
    out = np.ones((3,) + tables.shape[:1] + (NUM_SEG_CLASSES,), tables.dtype)
    for f in range(3):
        if looked_up(cfg, f):
            out[f] = tables[:, f]
    return out


def class_index(seg):
    """seg [...] float -> (int class, valid): the cast truncates toward zero; NaN, inf and anything outside [0, 19) after
    the cast is no class (one_hot of an out-of-range id is a zero row, davo.py:1115)."""
    seg = np.asarray(seg, np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(seg) & (seg > -1.0) & (seg < float(NUM_SEG_CLASSES))
    return np.where(ok, seg, 0.0).astype(np.int64), ok


def attention(cfg, a19, seg):
    """a19 [3,B,19], seg [B,3,H,W,1] -> [3,B,H,W]: the gather through int(seg), 0 on labels that are no class; 1 on every
    pixel of an overridden frame, ignore labels included.  Keeps a19's dtype (bit-exact gathers of float32 rows)."""
    B, _, H, W, _ = seg.shape
    out = np.ones((3, B, H, W), a19.dtype)
    for f in range(3):
        if looked_up(cfg, f):
            idx, ok = class_index(seg[:, FILE_PLANE[f], :, :, 0])
            out[f] = np.where(ok, np.take_along_axis(a19[f], idx.reshape(B, -1), axis=1).reshape(B, H, W), 0)
    return out


def images(img_u8):
    """[B,H,3W,3] u8 -> [3,B,H,W,3] float64: (u8 * (1/255)) * 2 - 1 (davo.py:967-971,1519-1522)."""
    B, H, W3, _ = img_u8.shape
    W = W3 // 3
    x = (img_u8.astype(np.float64) * (1.0 / 255.0)) * 2.0 - 1.0
    return np.stack([x[:, :, s * W:(s + 1) * W] for s in FILE_PLANE])


def masked_images(cfg, imgs, att):
    """imgs [3,B,H,W,3], att [3,B,H,W] -> rgb_k * att_k where the version masks rgb (davo.py:1419-1421,1447-1449), else imgs."""
    return imgs * att[..., None] if cfg.mask_rgb else imgs.copy()


def seg_19(seg):
    """seg [B,3,H,W,1] -> list of 3 (tgt, src0, src1) one-hot [B,H,W,19] float32."""
    out = []
    for f in range(3):
        idx, ok = class_index(seg[:, FILE_PLANE[f], :, :, 0])
        out.append(((idx[..., None] == np.arange(NUM_SEG_CLASSES)) & ok[..., None]).astype(np.float32))
    return out
