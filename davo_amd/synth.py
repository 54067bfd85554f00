"""Synthetic inputs and weights for the pose path.

No KITTI dump, FlowNet2/DeepLab output or checkpoint exists offline, so tests and
``bench.py`` run on synthetic tensors of the reference's shapes and statistics:

* ``img``  u8  ``[B,H,3W,3]``   uniform{0..255}; strip order src0|tgt|src1
  (reference ``data_loader.py:537-557``, ``data/preprocess.py:61-66``)
* ``flow`` f32 ``[B,4,H,W,2]``  ~ (0.32140523, 15.384229) — the dataset statistics the
  reference hard-codes (``davo.py:1090``)
* ``seg``  f32 ``[B,3,H,W,1]``  Cityscapes train ids 0..18 in 8x8 blocks, 3 % of blocks 255
  (ignore id, ``utils/seg_utils/labels.py:64-70``)
* ``depth`` f32 ``[B,3,H,W,1]`` (``make_depth``, depth-source variants only) smooth positive fields in (1, 80)

The PRNG is splitmix64 and every float is produced by integer arithmetic plus IEEE
add/mul/sqrt only (the "normal" is an Irwin-Hall sum of four uniforms), so the same
seed gives bit-identical tensors on every host — the GPU box regenerates the inputs
that the committed golden outputs under tests/golden/ were computed from.
Seed 8964 is the reference's own (``train.py:34``).
"""
import math

import numpy as np

from .version import parse_version, weight_shapes, NUM_SEG_CLASSES

SEED = 8964
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)
_GAMMA = 0x9E3779B97F4A7C15


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def splitmix64(seed, stream, n):
    """n 64-bit outputs of the splitmix64 sequence whose state starts at
    mix(seed, stream); counter-based, so it vectorises."""
    with np.errstate(over="ignore"):
        base = _mix(np.uint64(seed) * np.uint64(0x2545F4914F6CDD1D) + np.uint64(stream) * np.uint64(_GAMMA))
        idx = np.arange(1, n + 1, dtype=np.uint64)
        return _mix(base + idx * np.uint64(_GAMMA))


def uniform01(seed, stream, n):
    """float64 in [0,1) with 53 random bits."""
    return (splitmix64(seed, stream, n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def normalish(seed, stream, n):
    """zero-mean unit-variance Irwin-Hall(4) variate; add/mul only."""
    u = uniform01(seed, stream, 4 * n).reshape(4, n)
    s = (u[0] + u[1]) + (u[2] + u[3])
    return (s - 2.0) * 1.7320508075688772          # sqrt(12/4)


def _stream(name):
    """stable 32-bit stream id from a tensor name (FNV-1a)."""
    h = 0x811C9DC5
    for ch in name.encode():
        h = ((h ^ ch) * 0x01000193) & 0xFFFFFFFF
    return h


def make_inputs(B, H=128, W=416, seed=SEED, first_window=0, labels="f32", flow="f32"):
    """Synthetic batch of B triplets; window w of a sequence is reproducible on its own
    (``first_window`` offsets the per-window streams), which is what lets ranks generate
    just their shard.  ``labels`` = "u8": the label maps are the byte twin of the float ones
    (``davo_amd.labels_to_u8``), uint8 [B,3,H,W,1].  ``flow`` = "f16": the flow is the rounded twin of the float32 draw
    (``davo_amd.flow_to_f16``), float16 [B,4,H,W,2]."""
    from .flow import check_flow_format, flow_to_f16
    from .labels import check_label_format, labels_to_u8
    check_label_format(labels)
    flow_fmt = check_flow_format(flow)
    img = np.empty((B, H, 3 * W, 3), np.uint8)
    flow = np.empty((B, 4, H, W, 2), np.float32)
    seg = np.empty((B, 3, H, W, 1), np.float32)
    hb, wb = (H + 7) // 8, (W + 7) // 8
    for b in range(B):
        w = first_window + b
        r = splitmix64(seed, _stream("img") + 7919 * w, (H * 3 * W * 3 + 7) // 8)
        img[b] = r.view(np.uint8)[: H * 3 * W * 3].reshape(H, 3 * W, 3)
        f = normalish(seed, _stream("flow") + 7919 * w, 4 * H * W * 2)
        flow[b] = (f * 15.384229 + 0.32140523).astype(np.float32).reshape(4, H, W, 2)
        r = splitmix64(seed, _stream("seg") + 7919 * w, 3 * hb * wb)
        ids = (r % np.uint64(NUM_SEG_CLASSES)).astype(np.float32)
        ign = ((r >> np.uint64(32)) % np.uint64(100)) < np.uint64(3)
        ids[ign] = 255.0
        blk = ids.reshape(3, hb, wb)
        seg[b, :, :, :, 0] = np.repeat(np.repeat(blk, 8, axis=1), 8, axis=2)[:, :H, :W]
    return img, (flow_to_f16(flow) if flow_fmt == "f16" else flow), (labels_to_u8(seg) if labels == "u8" else seg)


def make_depth(B, H=128, W=416, seed=SEED, first_window=0, fmt="f32"):
    """Synthetic depth planes f32 ``[B,3,H,W,1]`` (file order src0, tgt, src1; reference ``davo.py:991-996``,
    ``test_kitti_pose.py:48``) in a monodepth2-like range: per plane a smooth field - a coarse 5x9 grid of depths, log-uniform
    in [1.5, 60], interpolated bilinearly, times a per-pixel ripple of +-5 % - so every value lies strictly inside (1, 80).
    Reproducible per window like ``make_inputs`` (streams of their own: the other planes do not move); integer arithmetic plus
    IEEE add/mul only after the grid's exponentiation, which is float64 ``np.exp2`` of 45 values per plane.  ``fmt`` = "f16": the
    rounded twin of the float32 draw (``davo_amd.depth_to_f16``), float16 [B,3,H,W,1]."""
    from .depth import check_depth_format, depth_to_f16
    check_depth_format(fmt)
    depth = np.empty((B, 3, H, W, 1), np.float32)
    gh, gw = 5, 9
    ys = np.linspace(0.0, gh - 1.0, H)
    xs = np.linspace(0.0, gw - 1.0, W)
    y0 = np.minimum(ys.astype(np.int64), gh - 2)
    x0 = np.minimum(xs.astype(np.int64), gw - 2)
    fy = (ys - y0)[:, None]
    fx = (xs - x0)[None, :]
    for b in range(B):
        w = first_window + b
        u = uniform01(seed, _stream("depth") + 7919 * w, 3 * gh * gw).reshape(3, gh, gw)
        grid = 1.5 * np.exp2(u * math.log2(60.0 / 1.5))
        rip = uniform01(seed, _stream("depth_ripple") + 7919 * w, 3 * H * W).reshape(3, H, W)
        for p in range(3):
            g = grid[p]
            top = g[y0][:, x0] * (1.0 - fx) + g[y0][:, x0 + 1] * fx
            bot = g[y0 + 1][:, x0] * (1.0 - fx) + g[y0 + 1][:, x0 + 1] * fx
            depth[b, p, :, :, 0] = ((top * (1.0 - fy) + bot * fy) * (0.95 + 0.1 * rip[p])).astype(np.float32)
    return depth_to_f16(depth) if fmt == "f16" else depth


def make_frames(n_frames, H=128, W=416, seed=SEED, depth=False, labels="f32", flow="f32"):
    """A synthetic sequence in the frame layout (davo_amd/frames.py): ``(frames, flow2, seg)`` - ``(frames, flow2, seg, depth)`` with
    ``depth`` - for the n_frames - 2 windows of n_frames frames: frames u8 [n,H,W,3], flow2 f32 [n-2,2,H,W,2] (per window, the
    statistics of ``make_inputs``), seg [n,H,W,1] (8x8 blocks of train ids, 3 % ignore; uint8 with labels="u8"), depth f32
    [n,H,W,1] (the fields of ``make_depth``).  Every frame and every window draws from streams of its own, so no two frames agree
    in any plane, and consecutive windows share their frames by construction - which ``make_inputs``' windows, drawn one by one,
    do not.  ``flow`` = "f16": flow2 is float16, ``davo_amd.flow_to_f16`` of the float32 draw.  ``depth`` = "f16" (instead of
    True): the depth planes are float16, ``davo_amd.depth_to_f16`` of the float32 draw."""
    from .flow import check_flow_format, flow_to_f16
    from .labels import check_label_format, labels_to_u8
    check_label_format(labels)
    check_flow_format(flow)
    if n_frames < 3:
        raise ValueError("a sequence needs at least 3 frames, got %d" % n_frames)
    frames = np.empty((n_frames, H, W, 3), np.uint8)
    seg = np.empty((n_frames, H, W, 1), np.float32)
    flow2 = np.empty((n_frames - 2, 2, H, W, 2), np.float32)
    hb, wb = (H + 7) // 8, (W + 7) // 8
    for f in range(n_frames):
        r = splitmix64(seed, _stream("frame_img") + 7919 * f, (H * W * 3 + 7) // 8)
        frames[f] = r.view(np.uint8)[: H * W * 3].reshape(H, W, 3)
        r = splitmix64(seed, _stream("frame_seg") + 7919 * f, hb * wb)
        ids = (r % np.uint64(NUM_SEG_CLASSES)).astype(np.float32)
        ids[((r >> np.uint64(32)) % np.uint64(100)) < np.uint64(3)] = 255.0
        seg[f, :, :, 0] = np.repeat(np.repeat(ids.reshape(hb, wb), 8, axis=0), 8, axis=1)[:H, :W]
    for w in range(n_frames - 2):
        v = normalish(seed, _stream("frame_flow") + 7919 * w, 2 * H * W * 2)
        flow2[w] = (v * 15.384229 + 0.32140523).astype(np.float32).reshape(2, H, W, 2)
    out = (frames, flow_to_f16(flow2) if flow == "f16" else flow2, labels_to_u8(seg) if labels == "u8" else seg)
    if depth:
        planes = make_depth((n_frames + 2) // 3, H, W, seed=seed, first_window=1000003,      # three planes per draw, all different
                            fmt="f16" if depth == "f16" else "f32")
        out += (np.ascontiguousarray(planes.reshape(-1, H, W, 1)[:n_frames]),)
    return out


def make_weights(version_or_cfg, seed=SEED):
    """dict TF-name -> float32 array (HWIO conv kernels, [in,out] dense kernels).

    conv ~ U(+-sqrt(6/fan_in)) (He-uniform keeps activations O(1) through eight ReLU
    layers, so the 6-DoF outputs are large enough for the 1e-4 absolute bar to bite),
    conv biases U(+-0.05), SE kernels variance-scaling as nets/attention_module.py:60,
    SE biases U(+-0.5) (every SE scope: se_flow, se_flow_near, se_flow_far, se_seg, se_rgb, se_segflow, se_depth - each
    tensor on a stream of its own, named after it), static seg weights stddev 0.05 as nets/posenn.py:387-388, the depth
    threshold of `-se_flow_on_depthseg_seplayers' N(cfg.depth_thres_init, 0.1), its initialiser (davo.py:1136-1141)."""
    cfg = parse_version(version_or_cfg) if isinstance(version_or_cfg, str) else version_or_cfg
    out = {}
    for name, shape in weight_shapes(cfg).items():
        n = int(np.prod(shape))
        st = _stream(name)
        if name.endswith("/weights"):
            fan_in = shape[0] * shape[1] * shape[2]
            a = (uniform01(seed, st, n) * 2.0 - 1.0) * math.sqrt(6.0 / fan_in)
            if "/pred/" in name:
                a = a * 16.0        # lifts the 6-DoF outputs to O(0.1), the scale of real KITTI motion
        elif name.endswith("/biases"):
            a = (uniform01(seed, st, n) * 2.0 - 1.0) * 0.05
        elif name.endswith("/kernel"):
            a = normalish(seed, st, n) * math.sqrt(2.0 / shape[0])
        elif name.endswith("/bias"):
            a = (uniform01(seed, st, n) * 2.0 - 1.0) * 0.5
        elif name.endswith("seg_channel_weight/weight"):
            a = normalish(seed, st, n) * 0.05
        elif name.endswith("/depth_threshold"):             # davo.py:1136-1141: random_normal(mean = the version's number, stddev 0.1)
            a = cfg.depth_thres_init + normalish(seed, st, n) * 0.1
        else:
            raise KeyError(name)
        out[name] = a.astype(np.float32).reshape(shape)
    return out
