"""The rows tests/test_forward_plan.py (csrc/plan.h: decide_forward through davo_decide_forward, no GPU), tests/test_forward_plan_gpu.py
(a live engine) and tools/record_forward_launches.py (the recorder of tests/golden/forward_launches.json) share: an explicit table of
forwards, one per rule of the launch sequence, and `observe', which runs a row on an engine and reads back what it launched."""
import collections
import ctypes
import os
import re

from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION, _lib

import coupled_cases as CC
import f16_depth_cases as FD
import feature_attention_cases as FA
import pooled_flow_ref as PF
import three_frame_cases as K3

# one variant per kind of attention front, then the PoseNN forms
FLOW = FLAGSHIP_VERSION
CLASS = FD.BASE + "-segmask_all-se_rgb_to_seg-fc_tanh"
DEPTH = FD.VERSIONS[12]
SPLIT = FD.VERSIONS[13]
POOLED = PF.version("se_spp21_flow")
TRIPLET = K3.FLAGSHIP3
COUPLED = CC.FLAGSHIP_C
INSERT = FA.PUBLISHED
VERSIONS = {"flow": FLOW, "class": CLASS, "depth": DEPTH, "split": SPLIT, "pooled": POOLED, "triplet": TRIPLET, "coupled": COUPLED,
            "insert": INSERT}
FRONT_OF = {"flow": "flow", "class": "class", "depth": "depth", "split": "split", "pooled": "pooled", "triplet": "flow",
            "coupled": "flow", "insert": "none"}

BIG, SMALL = (128, 416), (36, 100)      # cnv7's map: 16 x 52 = 832 pixels; 5 x 13 = 65, under the fused head's 128

Row = collections.namedtuple("Row", "variant H W B precision impl pairs options entry")


def _r(variant, shape, B, precision, impl=0, pairs="both", entry="host", **options):
    return Row(variant, shape[0], shape[1], B, precision, impl, pairs, options, entry)


# entry "host" = Engine.forward (f16x3: the call's last kernel mirrors the range record, nothing zeroes it); "device" =
# Engine.forward_device (f16x3: a ticketed batch - its first kernel zeroes the record's per-batch word, its last keeps the inputs)
ROWS = [
    # the flagship over the fold boundary (FOLD_EXCITE_MAX_BATCH = 2) and on the small map, both precisions
    _r("flow", BIG, 1, "f16x3"), _r("flow", BIG, 2, "f16x3"), _r("flow", BIG, 3, "f16x3"), _r("flow", SMALL, 2, "f16x3"),
    _r("flow", BIG, 1, "f32"), _r("flow", BIG, 2, "f32"), _r("flow", BIG, 3, "f32"), _r("flow", SMALL, 2, "f32"),
    # every other front kind on both sides of the boundary, both precisions
    _r("class", BIG, 2, "f16x3"), _r("class", BIG, 3, "f16x3"), _r("class", BIG, 2, "f32"), _r("class", BIG, 3, "f32"),
    _r("depth", BIG, 2, "f16x3"), _r("depth", BIG, 3, "f16x3"), _r("depth", BIG, 2, "f32"), _r("depth", BIG, 3, "f32"),
    _r("split", BIG, 2, "f16x3"), _r("split", BIG, 3, "f16x3"), _r("split", BIG, 2, "f32"), _r("split", BIG, 3, "f32"),
    _r("pooled", BIG, 2, "f16x3"), _r("pooled", BIG, 3, "f16x3"), _r("pooled", BIG, 2, "f32"), _r("pooled", BIG, 3, "f32"),
    # the three-frame PoseNN, the coupled heads, feature attention
    _r("triplet", BIG, 2, "f16x3"), _r("triplet", SMALL, 2, "f16x3"), _r("triplet", BIG, 2, "f32"),
    _r("coupled", BIG, 2, "f16x3"), _r("coupled", SMALL, 2, "f16x3"), _r("coupled", BIG, 2, "f32"),
    _r("insert", BIG, 2, "f16x3"), _r("insert", SMALL, 2, "f16x3"), _r("insert", BIG, 2, "f32"),
    # impl 1, the direct convolution: its group loop over the heads
    _r("flow", SMALL, 2, "f32", impl=1), _r("coupled", SMALL, 2, "f32", impl=1), _r("insert", SMALL, 2, "f32", impl=1),
    # one pair per window
    _r("flow", BIG, 2, "f16x3", pairs="src0"), _r("class", BIG, 2, "f16x3", pairs="src0"), _r("flow", BIG, 3, "f32", pairs="src0"),
    # fold_tails: nothing folded under the boundary, both tails and the excitation alone above it, the split front's folded form
    _r("flow", BIG, 1, "f16x3", fold_tails=0), _r("flow", BIG, 3, "f16x3", fold_tails=1), _r("flow", BIG, 3, "f16x3", fold_tails=2),
    _r("flow", SMALL, 2, "f16x3", fold_tails=1), _r("flow", BIG, 3, "f32", fold_tails=1), _r("split", BIG, 3, "f16x3", fold_tails=1),
    _r("class", BIG, 2, "f16x3", fold_tails=0), _r("pooled", BIG, 2, "f16x3", fold_tails=1),
    # mask + pack fused into cnv1 (never on the split front, the three-frame PoseNN or float32)
    _r("flow", BIG, 2, "f16x3", fuse_pack=1), _r("split", BIG, 2, "f16x3", fuse_pack=1), _r("triplet", BIG, 2, "f16x3", fuse_pack=1),
    _r("flow", BIG, 2, "f32", fuse_pack=1),
    # the two-pass head by choice
    _r("flow", BIG, 2, "f16x3", fuse_pose=0), _r("flow", BIG, 2, "f32", fuse_pose=0), _r("coupled", BIG, 2, "f16x3", fuse_pose=0),
    # cnv1..cnv3 off their patch kernels
    _r("flow", BIG, 2, "f16x3", patch_cnv2=0), _r("flow", BIG, 2, "f16x3", patch_cnv3=0), _r("flow", BIG, 2, "f32", patch_f32=0),
    _r("triplet", BIG, 2, "f16x3", patch_cnv1_t=0), _r("flow", BIG, 2, "f16x3", split_k=0, force_tile=0),
    # ticketed batches: the snapshot rides in pose_from_tiles; a two-pass head and a pose tail in cnv7 leave it a launch of its own
    _r("flow", BIG, 2, "f16x3", entry="device"), _r("flow", SMALL, 2, "f16x3", entry="device"),
    _r("flow", BIG, 2, "f16x3", entry="device", fold_tails=1), _r("triplet", BIG, 2, "f16x3", entry="device"),
    _r("flow", BIG, 2, "f32", entry="device"),
]


def row_id(r):
    tail = "".join("-%s%d" % kv for kv in sorted(r.options.items()))
    return "%s-%dx%d-B%d-%s%s%s%s%s" % (r.variant, r.H, r.W, r.B, r.precision, "-impl1" if r.impl else "",
                                       "" if r.pairs == "both" else "-" + r.pairs, "" if r.entry == "host" else "-" + r.entry, tail)


assert len({row_id(r) for r in ROWS}) == len(ROWS)

# ---- davo_decide_forward (include/davo_hip.h) ------------------------------------------------------------------------------
_HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "davo_hip.h")
_LABELS = []


def labels():
    """DAVO_FORWARD_LABELS as the header has it (read at the first use: the recorder needs none)."""
    if not _LABELS:
        with open(_HEADER) as f:
            _LABELS.extend(re.findall(r'"([a-z0-9_]+)"', re.search(r"#define DAVO_FORWARD_LABELS (\{[^}]*\})", f.read()).group(1)))
    return _LABELS


UNPROFILED = {"range_guard_snapshot"}                       # a launch without a profile entry
CALL = ("H", "W", "B", "pairs", "mode", "att_source", "cnv6_out", "cin_per_frame", "topology", "heads", "posenn_se")
MODES = {"f16x3": 0, "f32": 1, "direct": 2}
PLAN_DEFAULTS = dict(fold_tails=-1, fuse_pack=-1, fuse_pose=1, patch_cnv1_t=1, patch_cnv2=1, patch_cnv3=1, patch_f32=1, force_tile=-1,
                     zero_record=0, want_snapshot=0)      # in the header's order
HEAD = ("NB", "front", "squeeze", "fold_excite", "excite", "excite_far", "reset_at", "pack", "pack_ld", "packed_ld", "packed_valid", "se5",
        "head", "cols", "heads", "snapshot_launch", "cnv7_valid")
LAYER = ("runner", "label", "x_buf", "x_ch", "Hin", "Win", "y_ld", "Hout", "Wout", "y_f32", "fuse_pose", "pose_tail", "pose_six", "plan_code",
         "ngroups", "cin", "cout", "x_coff0", "x_coff1", "y_coff0", "y_coff1")
FRONTS = ("flow", "split", "class", "depth", "pooled")
PACK_NONE, PACK_PAIR, PACK_TRIPLET = range(3)
RUN_PATCH, RUN_PATCH_FUSED, RUN_PATCH_CNV1T, RUN_IGEMM_H3, RUN_IGEMM_F32, RUN_DIRECT = range(6)
BUF_PACKED, BUF_SE = -1, -2
HEAD_TAIL, HEAD_TILES, HEAD_TWO_PASS = range(3)


def decide_forward(call, **options):
    """davo_decide_forward on a dict of CALL's keys -> the record as a dict ("layers": seven dicts of LAYER's keys, "launches": the
    labels in issue order), or the negative status of a refusal."""
    assert set(call) == set(CALL) and set(options) <= set(PLAN_DEFAULTS), (call, options)
    opts = dict(PLAN_DEFAULTS, **options)
    c = (ctypes.c_int * len(CALL))(*[int(call[k]) for k in CALL])
    o = (ctypes.c_int * len(opts))(*[int(opts[k]) for k in PLAN_DEFAULTS])
    out = (ctypes.c_int * 256)()
    n = _lib.lib().davo_decide_forward(c, o, len(opts), out, 256)
    if n < 0:
        return n
    at = len(HEAD) + 7 * len(LAYER)
    assert n == at + 1 + out[at] <= 256, (n, at, out[at])
    p = dict(zip(HEAD, out[:len(HEAD)]))
    p["layers"] = [dict(zip(LAYER, out[len(HEAD) + i * len(LAYER):len(HEAD) + (i + 1) * len(LAYER)])) for i in range(7)]
    p["launches"] = [labels()[k] for k in out[at + 1:n]]
    return p


def call_of(cfg, H, W, B, mode, pairs="both"):
    cin_per_frame, cnv6_out, _, _, _, att_source = cfg.as_c_ints()[:6]
    return dict(H=H, W=W, B=B, pairs=Engine.PAIRS[pairs], mode=MODES[mode], att_source=att_source, cnv6_out=cnv6_out,
                cin_per_frame=cin_per_frame, topology=int(cfg.posenn == "triplet"), heads=int(cfg.heads == "coupled"),
                posenn_se=int(cfg.posenn_se != "none"))


def mode_of(r):
    return "direct" if r.impl else r.precision


def plan_of(r, **more):
    """The plan of a row as its engine's forward decides it: every f16x3 batch of an entry point wants the range guard's snapshot,
    a ticketed one (the device entry) has its record zeroed."""
    ticketed = mode_of(r) == "f16x3"
    options = {k: v for k, v in r.options.items() if k in PLAN_DEFAULTS}
    options.update(want_snapshot=int(ticketed), zero_record=int(ticketed and r.entry == "device"))
    options.update(more)
    return decide_forward(call_of(parse_version(VERSIONS[r.variant]), r.H, r.W, r.B, mode_of(r), r.pairs), **options)


_CASES = {}


def case(r):
    """(cfg, weights, (img, flow, seg), depth or None) of a row, built once per (variant, shape, batch) and left unchanged."""
    key = (r.variant, r.H, r.W, r.B)
    if key not in _CASES:
        cfg = parse_version(VERSIONS[r.variant])
        inputs = synth.make_inputs(r.B, r.H, r.W, first_window=7)
        depth = synth.make_depth(r.B, r.H, r.W, first_window=7) if cfg.needs_depth else None
        _CASES[key] = (cfg, synth.make_weights(cfg), inputs, depth)
    return _CASES[key]


def observe(r):
    """One forward of a row on a new engine, profiled -> {"launches": {profile label: launches}, "last_plan": [[[M tiles, tile], ...]
    per layer], "last_split": [parts per layer]}.  The engine calls are Engine.profile, profile_entries, last_plan and last_split."""
    cfg, weights, inputs, depth = case(r)
    e = Engine(cfg, r.H, r.W, r.B)
    try:
        e.load_weights(weights)
        e.set_precision(r.precision)
        e.set_impl(r.impl)
        e.set_pairs(r.pairs)
        for k, v in r.options.items():
            e.set_option(k, v)
        e.profile(1)
        if r.entry == "host":
            e.forward(*inputs, depth=depth)
        else:
            bufs = [e.alloc(a.nbytes).upload(a) for a in inputs + ((depth,) if depth is not None else ())]
            pose = e.alloc(r.B * 12 * 4)
            e.forward_device(r.B, bufs[0], bufs[1], bufs[2], pose, depth=bufs[3] if depth is not None else None)
            e.synchronize()
            for b in bufs + [pose]:
                b.free()
        stats = e.range_stats()
        assert stats["reissued"] == 0 and stats["recalibrations"] == 0 and stats["f32_batches"] == 0, (row_id(r), stats, e.range_report())
        return {"launches": {k: n for k, (n, _) in e.profile_entries().items()},
                "last_plan": [[list(t) for t in e.last_plan(li)] for li in range(7)],
                "last_split": [e.last_split(li) for li in range(7)]}
    finally:
        e.close()
