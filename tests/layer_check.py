"""Per-launch check of a forward against float64: every conv layer's output is compared with a float64 convolution of the
GPU's OWN decoded input to that layer (Engine.debug_read), so each launch of a plan is judged alone and errors do not pile
up through the network.  Imported by the tests like helpers.py; the checker only, the library never calls it.

Two bars per layer:
  (a) max|got - ref| <= REL_MAX * max|ref|                       (test_conv_kernel_vs_oracle's bar);
  (b) |got - ref| <= TAU[precision][layer] * (conv(|x|, |w|) + |b|) + floor   element-wise, scaled by each output's L1
      mass: catches errors in small outputs (border pixels, values next to the ReLU, quiet channels) that (a) scales away.
      docs/F16X3_NUMERICS.md bounds the f16x3 product error at ~3 * 2^-22 of the L1 mass, plus the float32 accumulation,
      plus the pair format's absolute grid: `lo' rounds onto the fp16 subnormal grid, <= 2^-25 in stored units, once for
      the stored output and once for the split bias.  So floor = STORE_FLOOR * 2^-shift in f16x3 (shift: the layer's log2
      storage scale) and 0 in float32.  An output that is its bias alone (a 7x7 window of fully masked input) shows it:
      5.3e-4 off by 1.2e-8, 2.3e-5 of its L1 mass.
      Bar (a) takes the same floor only where asked (a_floor=True: the storage-scale edge sets of
      tests/test_scaled_layers_gpu.py).  With the layer's stored maximum in the guard's lowest binade [GUARD_FLOOR,
      2 GUARD_FLOOR), that floor is STORE_FLOOR * 2^-shift <= STORE_FLOOR / GUARD_FLOOR = 2^-18 of max|ref| in rounding
      alone, beside REL_MAX = 5e-6 (2^-17.6) for everything else: so (a) becomes max|got - ref| <= REL_MAX * max|ref| + floor.
The network's inputs: `packed' against the oracle's packing and `att_table' against its class tables, at 2e-6.  The pose:
0.01 * mean(pred(cnv7)) in float64 from the GPU's cnv7 when it is stored, else from cnv7(GPU cnv6) (fused pose head)."""
import json
import os

import numpy as np

from davo_amd.version import ATT_SOURCE, NUM_SEG_CLASSES
from oracle import davo_oracle as O

import class_table_ref as R

REL_MAX = 5e-6                  # bar (a)
TABLE_TOL = 2e-6                # att_table, absolute (the entries are sigmoids in (0, 1))
PACKED_TOL = 2e-6               # packed: absolute, relative to the tensor's max where that is above 1 (flow channels)
POSE_REL = 2e-6                 # poses vs float64 from the GPU's last stored activation, relative to max|pose|
TAU_CAP = 2.0 ** -16
STORE_FLOOR = 2.0 ** -24        # f16x3: two roundings onto the fp16 subnormal grid of the stored units (see above)
# Bar (b), per precision and layer: the smallest power of two at least 4x the worst ratio (|err| - floor) / L1 mass measured
# on an MI355X over every case of tests/test_plan_layers_gpu.py (in brackets), and at most TAU_CAP.
TAU = {
    "f16x3": {"cnv1": 2.0 ** -18,   # 5.6e-7
              "cnv2": 2.0 ** -19,   # 3.7e-7
              "cnv3": 2.0 ** -19,   # 3.2e-7
              "cnv4": 2.0 ** -19,   # 3.7e-7
              "cnv5": 2.0 ** -19,   # 3.6e-7
              "cnv6": 2.0 ** -19,   # 3.6e-7
              "cnv7": 2.0 ** -19},  # 3.2e-7
    "f32": {"cnv1": 2.0 ** -18,     # 8.7e-7
            "cnv2": 2.0 ** -18,     # 4.8e-7
            "cnv3": 2.0 ** -19,     # 3.9e-7
            "cnv4": 2.0 ** -19,     # 3.6e-7
            "cnv5": 2.0 ** -19,     # 4.2e-7
            "cnv6": 2.0 ** -19,     # 3.7e-7
            "cnv7": 2.0 ** -19},    # 4.6e-7
}

# The f16x3 range guard's window on a layer's stored maximum: [GUARD_FLOOR, GUARD_CEIL).  GUARD_FLOOR must equal the
# "too small" threshold of range_value_fails in davo_amd/csrc/params.h (tests/test_storage_scale_emulation.py derives it,
# tests/test_scaled_layers_gpu.py shows the library trips exactly there).
GUARD_FLOOR_LOG2 = -6
GUARD_FLOOR = 2.0 ** GUARD_FLOOR_LOG2
GUARD_CEIL = 65504.0
CEIL_BINADE_LOG2 = 15           # the highest binade below GUARD_CEIL: [2^15, 65504)
EDGE_BAND = 2.0 ** -10          # edge_shifts keeps a stored maximum this far (relative) inside the window
STORED = ("cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6")     # the layers with a storage scale and a range record

# the packed tensor of the MFMA path drops the target's flow channels 3, 4 (always zero): 10 -> 8 channels
PACK8 = [0, 1, 2, 5, 6, 7, 8, 9]

# worst bar-(b) ratio seen in this process per (precision, layer): tests report it
WORST = {}
_REPORTS = {}                   # module -> its worst ratios, of the modules that finished in this process


def report_worst_ratios(module):
    """The body of a module-scoped autouse fixture (tests/test_plan_layers_gpu.py, tests/test_cnv6_widths_gpu.py): the worst
    bar-(b) ratio per precision and layer over that module alone, printed, and written as JSON {module: {"precision/layer":
    ratio}} where DAVO_LAYER_RATIOS names a file (how TAU above was measured).  A module that finishes later in the same
    run adds its own entry and leaves the others' as they were."""
    WORST.clear()
    yield
    worst = {"%s/%s" % k: v for k, v in sorted(WORST.items())}
    print("worst |err| / L1 mass (%s):" % module, json.dumps(worst))
    _REPORTS[module] = worst
    path = os.environ.get("DAVO_LAYER_RATIOS")
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(_REPORTS, f, indent=1, sort_keys=True)


def conv64(x, w, b, stride, rate, relu=True):
    return O.conv2d_same(np.asarray(x, np.float64), np.asarray(w, np.float64), np.asarray(b, np.float64), stride, rate, relu)


def l1_mass(x, w, b, stride, rate):
    """conv(|x|, |w|) + |b|: what one output's float error is proportional to."""
    return O.conv2d_same(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)),
                         np.abs(np.asarray(b, np.float64)), stride, rate, relu=False)


def out_size(n, stride):
    return -(-n // stride)


def shapes(cfg, H, W):
    """{tensor: per-pair-image shape} of what debug_read returns."""
    H1, W1 = out_size(H, 2), out_size(W, 2)
    H2, W2 = out_size(H1, 2), out_size(W1, 2)
    return {"packed": (H, W, 8), "cnv1": (H1, W1, 16), "cnv2": (H2, W2, 32), "cnv3": (H2, W2, 64), "cnv4": (H2, W2, 128),
            "cnv5": (H2, W2, 256), "cnv6": (H2, W2, 2 * cfg.cnv6_out), "cnv7": (out_size(H2, 2), out_size(W2, 2), 512)}


def layers(cfg, weights):
    """[(name, input, stride, rate, [(w, b, input channel slice, output channel slice)])] of cnv1..cnv7 as the library
    stores them: cnv6 = rotation | translation on the same cnv5, cnv7 = the two heads on their halves of cnv6."""
    assert cfg.cin_per_frame == 5, "the 8-channel packed layout drops the target's two flow channels"
    g = lambda n: (weights["pose_exp_net/%s/weights" % n], weights["pose_exp_net/%s/biases" % n])
    w1, b1 = g("cnv1")
    out = [("cnv1", "packed", 2, 1, [(w1[:, :, PACK8], b1, slice(None), slice(None))])]
    for name, prev, stride, rate in (("cnv2", "cnv1", 2, 1), ("cnv3", "cnv2", 1, 2), ("cnv4", "cnv3", 1, 4), ("cnv5", "cnv4", 1, 8)):
        w, b = g(name)
        out.append((name, prev, stride, rate, [(w, b, slice(None), slice(None))]))
    c6 = cfg.cnv6_out
    heads = [g("pose/%s/cnv6" % h) for h in ("rotation", "translation")]
    out.append(("cnv6", "cnv5", 1, 2, [(w, b, slice(None), slice(k * c6, (k + 1) * c6)) for k, (w, b) in enumerate(heads)]))
    heads = [g("pose/%s/cnv7" % h) for h in ("rotation", "translation")]
    out.append(("cnv7", "cnv6", 2, 1, [(w, b, slice(k * c6, (k + 1) * c6), slice(k * 256, (k + 1) * 256))
                                      for k, (w, b) in enumerate(heads)]))
    return out


def layer_ratios(got, ref, mass, floor=0.0, a_floor=False):
    """-> (bar (a) ratio max|got - ref| / max|ref| (max|got - ref| - floor with a_floor), bar (b) ratio
    max (|got - ref| - floor) / mass, index of the worst (b) element)."""
    d = np.abs(np.asarray(got, np.float64) - ref)
    a = float(max(d.max() - (floor if a_floor else 0.0), 0.0) / max(np.abs(ref).max(), 1e-30))
    r = np.maximum(d - floor, 0.0) / np.maximum(mass, 1e-300)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return a, float(r[i]), i


def check_layer(name, got, x, groups, stride, rate, tau, what="", floor=0.0, a_floor=False):
    """got [N,Ho,Wo,C] against the float64 conv of x [N,H,W,Cin] under both bars; -> (ratio a, ratio b)."""
    ref = np.empty(got.shape)
    mass = np.empty(got.shape)
    for w, b, cin, cout in groups:
        ref[..., cout] = conv64(x[..., cin], w, b, stride, rate)
        mass[..., cout] = l1_mass(x[..., cin], w, b, stride, rate)
    a, rb, i = layer_ratios(got, ref, mass, floor, a_floor)
    assert a <= REL_MAX, "%s %s: bar (a) max|err| = %.3g of max|ref| > %.1g" % (what, name, a, REL_MAX)
    assert rb <= tau, "%s %s: bar (b) |err| = %.3g of the L1 mass at %s (got %.9g, ref %.9g, mass %.3g, floor %.3g) > tau %.3g" % (
        what, name, rb, i, got[i], ref[i], mass[i], floor, tau)
    return a, rb


def pose_from_cnv7(c7, weights):
    """[N,h,w,512] -> [N,6]: pred 1x1 of each head, spatial mean, x 0.01 (nets/posenn.py:240-250), float64."""
    outs = []
    for k, head in enumerate(("rotation", "translation")):
        p = "pose_exp_net/pose/%s/" % head
        pred = conv64(c7[..., 256 * k:256 * (k + 1)], weights[p + "pred/weights"], weights[p + "pred/biases"], 1, 1, relu=False)
        outs.append(pred.mean(axis=(1, 2)))
    return 0.01 * np.concatenate(outs, -1)


def pose_from_cnv6(c6, cfg, weights):
    _, _, _, _, groups = layers(cfg, weights)[6]
    c7 = np.empty(c6.shape[:1] + (out_size(c6.shape[1], 2), out_size(c6.shape[2], 2), 512))
    for w, b, cin, cout in groups:
        c7[..., cout] = conv64(c6[..., cin], w, b, 2, 1)
    return pose_from_cnv7(c7, weights)


def check_pose(got, want, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want).max()
    scale = np.abs(want).max()
    assert err <= POSE_REL * scale, "%s pose: max|err| %.3g > %.1g * max|ref| (%.3g)" % (what, err, POSE_REL, scale)
    return err / scale


# ---- the network's inputs ----------------------------------------------------------------------------------------
def class_table(cfg):
    """att_source 4..10: the tables come from per-frame descriptors (tests/class_table_ref.py)."""
    return ATT_SOURCE[cfg.att_source] >= 4


def ref_tables(cfg, img, flow, seg, weights):
    """[B,3,19] float64 tables, and which of the three frames' rows the library fills (the others are implied ones)."""
    if class_table(cfg):
        tab = R.class_tables(cfg, img, flow, seg, weights)
    else:
        tab = O.attention_tables(cfg, flow, weights, np.float64)
    rows = [] if cfg.att_source == "ones" else [0, 1, 2] if cfg.tgt_attended else [1, 2]
    return tab, rows


def ref_packed(cfg, img, flow, seg, weights):
    """[2B,H,W,8] float64 packed inputs of the MFMA path."""
    p = R.pack(cfg, img, flow, seg, weights) if class_table(cfg) else O.pack_inputs(cfg, img, flow, seg, weights)
    B, _, H, W, C = p.shape
    return p.reshape(2 * B, H, W, C)[..., PACK8]


def check_table(got, want, rows, what=""):
    if not rows:
        return 0.0
    err = float(np.abs(np.asarray(got, np.float64)[:, rows] - want[:, rows]).max())
    assert err <= TABLE_TOL, "%s att_table: max|err| %.3g > %.1g" % (what, err, TABLE_TOL)
    return err


def check_packed(got, want, what=""):
    err = float(np.abs(np.asarray(got, np.float64) - want).max())
    bar = PACKED_TOL * max(1.0, float(np.abs(want).max()))
    assert err <= bar, "%s packed: max|err| %.3g > %.3g" % (what, err, bar)
    return err


# ---- a whole forward -----------------------------------------------------------------------------------------------
def forward(e, img, flow, seg):
    """e.forward with the checker's preconditions: a batch above 8 runs as ONE step (host_chunk 0; debug_read then holds
    the whole batch), and the batch was not re-issued (a re-issued batch's tensors come from the other arithmetic or other
    storage scales)."""
    B = img.shape[0]
    if B > 8:
        e.set_option("host_chunk", 0)
    before = e.range_stats()
    got = e.forward(img, flow, seg)
    after = e.range_stats()
    assert after["f32_batches"] == before["f32_batches"] and after["reissued"] == before["reissued"], (before, after, e.range_report())
    return got


def plan_images(e, cfg, B, H, W, ends=2):
    """Pair images a subset check must hold: the first `ends' and the last `ends', and those holding the first and last
    row of every launch of the last forward's plan (last_plan: launch 0 covers rows [0, 128 m0), launch 1 the rest)."""
    NB = 2 * B
    sh = shapes(cfg, H, W)
    keep = set(range(ends)) | set(range(NB - ends, NB))
    for li, name in enumerate(("cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6", "cnv7")):
        per = sh[name][0] * sh[name][1]
        row = 0
        for m, _ in e.last_plan(li):
            for r in (row, min(row + 128 * m, NB * per) - 1):
                keep.add(min(r // per, NB - 1))
            row = min(row + 128 * m, NB * per)
    return sorted(i for i in keep if 0 <= i < NB)


FULL_IMAGES = 64                # pair images checked in full (B <= 32); above that, plan_images


def check_forward(e, cfg, weights, img, flow, seg, poses, precision, images=None, what="", stop_after=None, chunk=8,
                  a_floor=False, checked=None):
    """Check the last forward of engine `e` (run through forward() above) layer by layer.  images: pair-image indices to
    check (None = all up to FULL_IMAGES pair images, else "plan" = plan_images, "bounds" = plan_images with one image at
    each end).  stop_after: last tensor to check ("packed", "cnv1", ...).
    a_floor: bar (a) takes the storage floor too (module docstring).  checked: a dict kept across calls on the same inputs
    and images: a layer whose tensor AND input are bit-identical to the ones checked before is not convolved again.
    -> {layer: (ratio a, ratio b)}; the worst (b) ratios also go to WORST."""
    B, H, W3, _ = img.shape
    W = W3 // 3
    NB = 2 * B
    sh = shapes(cfg, H, W)
    stats = {}
    want_tab, rows = ref_tables(cfg, img, flow, seg, weights)
    stats["att_table"] = check_table(e.debug_read("att_table", (B, 3, NUM_SEG_CLASSES)), want_tab, rows, what)
    if images is None:
        images = list(range(NB)) if NB <= FULL_IMAGES else "plan"
    if isinstance(images, str) and images == "plan":
        images = plan_images(e, cfg, B, H, W)
    elif isinstance(images, str) and images == "bounds":
        images = plan_images(e, cfg, B, H, W, ends=1)
    images = np.asarray(images)
    trip = sorted(set(int(i) // 2 for i in images))
    want_p = ref_packed(cfg, img[trip], flow[trip], seg[trip], weights)
    pos = {b: k for k, b in enumerate(trip)}
    want_p = want_p[[2 * pos[int(i) // 2] + int(i) % 2 for i in images]]
    acts = {"packed": e.debug_read("packed", (NB,) + sh["packed"])[images]}
    stats["packed"] = check_packed(acts["packed"], want_p, what)
    if stop_after == "packed":
        return stats
    shifts = e.activation_range()[1] if precision == "f16x3" else {}
    fused = True
    for name, prev, stride, rate, groups in layers(cfg, weights):
        floor = STORE_FLOOR * 2.0 ** -shifts.get(name, 0) if precision == "f16x3" else 0.0
        try:
            acts[name] = e.debug_read(name, (NB,) + sh[name])[images]
        except Exception:
            if name != "cnv7":
                raise
            break                                   # the pose head ran fused: cnv7 was never stored
        if name == "cnv7":
            fused = False
        seen = checked.get(name) if checked is not None else None
        if seen is not None and np.array_equal(seen[0], acts[name]) and np.array_equal(seen[1], acts[prev]) and seen[2] == floor:
            worst = seen[3]
        else:
            worst = (0.0, 0.0)
            for c0 in range(0, len(images), chunk):
                s = slice(c0, c0 + chunk)
                a, b = check_layer(name, acts[name][s], acts[prev][s], groups, stride, rate, TAU[precision][name], what, floor,
                                   a_floor)
                worst = (max(worst[0], a), max(worst[1], b))
            if checked is not None:
                checked[name] = (acts[name], acts[prev], floor, worst)
        stats[name] = worst
        key = (precision, name)
        WORST[key] = max(WORST.get(key, 0.0), worst[1])
        del acts[prev]
        if stop_after == name:
            return stats
    got = np.asarray(poses, np.float64).reshape(NB, 6)[images]
    if fused:
        want = np.concatenate([pose_from_cnv6(acts["cnv6"][c0:c0 + chunk], cfg, weights) for c0 in range(0, len(images), chunk)])
        stats["pose(fused)"] = check_pose(got, want, what + " fused head")
    else:
        stats["pose"] = check_pose(got, pose_from_cnv7(acts["cnv7"], weights), what + " pose head")
    return stats


# ---- storage scales at the edges of the range guard's window (f16x3) ---------------------------------------------------
def binade_shift(vmax, lo_log2):
    """The power-of-two storage shift that puts a layer's largest |activation| vmax into [2^lo_log2, 2^(lo_log2 + 1))."""
    return int(lo_log2 - np.floor(np.log2(float(vmax))))


def edge_shifts(maxima, where):
    """Per-layer storage shifts at the edges of the guard's window.  maxima: {layer: largest |activation|, unscaled}
    (Engine.activation_range()[0] of a run at any scales); where: "floor", "ceiling", or {layer: "floor" | "ceiling" |
    None (shift 0)}.  "floor": the stored maximum in [GUARD_FLOOR, 2 GUARD_FLOOR); "ceiling": in [2^15, GUARD_CEIL (1 - 2^-10)).
    A maximum in the guard band (within EDGE_BAND of the window's edge: a rounding away from tripping the guard) steps one
    binade inwards - down at the ceiling, up at the floor.  -> {layer: shift}."""
    out = {}
    for k, m in maxima.items():
        w = where if isinstance(where, str) else where.get(k)
        if w is None:
            out[k] = 0
            continue
        assert m > 0, (k, m)
        if w == "floor":
            s = binade_shift(m, GUARD_FLOOR_LOG2)
            if m * 2.0 ** s < GUARD_FLOOR * (1.0 + EDGE_BAND):
                s += 1
        elif w == "ceiling":
            s = binade_shift(m, CEIL_BINADE_LOG2)
            if m * 2.0 ** s >= GUARD_CEIL * (1.0 - EDGE_BAND):
                s -= 1
        else:
            raise ValueError(w)
        out[k] = s
    return out


def pair_store(x, shift=0, flush_lo=False, clamp=GUARD_CEIL):
    """What an f16x3 epilogue stores, decoded: x' = min(f32(x 2^shift), clamp), hi = fp16(x'), lo = fp16(x' - hi),
    -> (hi + lo) 2^-shift in float64.  numpy's float16 keeps subnormals; flush_lo: lo halves below the smallest normal fp16
    are stored as 0 (a kernel that flushes denormals)."""
    xs = np.minimum(np.asarray(x, np.float64) * 2.0 ** shift, clamp).astype(np.float32)
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    if flush_lo:
        lo = np.where(np.abs(lo) < np.float16(2.0 ** -14), np.float16(0), lo)
    return (hi.astype(np.float64) + lo.astype(np.float64)) * 2.0 ** -shift


RECORD_REL = 2.0 ** -22         # the range record against max|debug_read|: the pair rounding, relative ...
RECORD_ABS = 2.0 ** -25         # ... plus the subnormal grid of lo, in stored units


def range_record_forward(e, img, flow, seg, shifts=None):
    """One forward(), with the range record started afresh: shifts installed (None = none; the next host call then
    starts from a zeroed record) and the host's maxima reset.  -> (poses, record {layer: max |stored|, unscaled})."""
    e.set_activation_shifts(shifts)
    e.activation_range(reset=True)
    poses = forward(e, img, flow, seg)
    return poses, e.activation_range()[0]


def check_range_record(e, cfg, B, H, W, record, what=""):
    """The range record of the last forward against what its kernels stored: record[layer] == max |debug_read(layer)| over
    the whole batch, within the pair rounding (RECORD_REL * max + RECORD_ABS * 2^-shift).  Catches an epilogue that skips
    range_note, notes before out_scale or notes rows outside the tensor.  -> {layer: (row of the maximum in the layer's
    GEMM, [(first row, rows) of each launch of last_plan])}."""
    sh = shapes(cfg, H, W)
    shifts = e.activation_range()[1]
    where = {}
    for li, name in enumerate(STORED):
        t = e.debug_read(name, (2 * B,) + sh[name])
        a = np.abs(t.reshape(-1, t.shape[-1])).max(axis=1)
        row = int(np.argmax(a))
        m = float(a[row])
        bar = RECORD_REL * m + RECORD_ABS * 2.0 ** -shifts[name]
        assert abs(record[name] - m) <= bar, "%s %s: range record %.9g, stored maximum %.9g (shift %d)" % (
            what, name, record[name], m, shifts[name])
        launches, r0 = [], 0
        for mt, _ in e.last_plan(li):
            n = min(128 * mt, a.size - r0)
            launches.append((r0, n))
            r0 += n
        where[name] = (row, launches)
    return where

