"""The launch decisions of the conv layers (csrc/plan.h: decide_layer_h3, decide_layer_f32) through davo_decide_layer, on the CPU:
structural properties of every decision, and tests/golden/layer_decisions.json - what the build before the decisions were split
from their issuers reported through Engine.last_plan, Engine.last_split and the profile's launch counts on an MI355X - row by row."""
import ctypes
import json
import os

import pytest

from davo_amd import _lib

import cnv6_width_cases as CW
import forward_plan_cases as FP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layer_decisions.json")

# include/davo_hip.h: davo_decide_layer's options, step record and tail
OPTIONS = ("wave128", "skip_order", "merge_order", "pad_classes", "merge_rem_f32", "share_taps", "merge_rem", "merge_cnv4", "tile_208x128",
           "deep_ring", "split_k", "fold_fixup", "f32_n16", "f32_n256", "ncu", "dev_cus", "cu_partition", "user_stream", "max_batch",
           "shift_in", "shift_out", "force_tile", "pose_tail", "posenn_se", "triplet", "coupled")
DEFAULTS = dict(wave128=2, skip_order=1, merge_order=-1, pad_classes=6, merge_rem_f32=1, share_taps=1, merge_rem=1, merge_cnv4=0,
                tile_208x128=0, deep_ring=1, split_k=1, fold_fixup=0, f32_n16=1, f32_n256=0, ncu=256, dev_cus=256, cu_partition=0,
                user_stream=0, max_batch=1, shift_in=0, shift_out=0, force_tile=-1, pose_tail=0, posenn_se=0, triplet=0, coupled=0)
STEP = ("family", "tile", "row0", "m_end", "mtile0", "ntiles_n", "gx", "gy", "n_main", "n_rem", "order", "deep", "rem_label",
        "rem_mtile0", "rem_ntiles_n", "order_kind", "family_ok", "nchunks")
TAIL = ("code0", "code1", "split", "fold_if_xcd", "pad_classes", "pose_bm", "pose_mt", "pose_ntn", "pose_floats", "splitk_floats",
        "nchunks_h", "cpb")
H3, H3S, H3W, H3W64, H3W128, H3_MAINREM, H3_SPLITK, F32, F32_N256, F32_MAINREM = range(10)
TILE_BM = {0: 128, 1: 256, 2: 256, 3: 128, 4: 128, 5: 256, 6: 208, 8: 208}
TILE_BN = {0: 32, 1: 64, 2: 128, 3: 256, 4: 128, 5: 256, 6: 256, 8: 128}
LAYER_COUT = lambda width: (16, 32, 64, 128, 256, 2 * width, 256)
# options of the Engine that choose between the patch kernels and these decisions for cnv1..cnv3, or touch neither
NOT_DECISION_OPTIONS = {"fuse_pack", "patch_cnv2", "patch_cnv3", "patch_f32"}


def half(n, times):
    for _ in range(times):
        n = (n + 1) // 2
    return n


def layer_rows(li, H, W, NB):
    """Output rows of conv layer li's GEMM: cnv1, cnv2 and cnv7 have stride 2."""
    k = 1 if li == 0 else 3 if li == 6 else 2
    return NB * half(H, k) * half(W, k)


def decide(precision, li, H, W, NB, width=128, fuse_pose=0, **options):
    assert set(options) <= set(OPTIONS), options
    opts = dict(DEFAULTS, **options)
    arr = (ctypes.c_int * len(OPTIONS))(*[int(opts[k]) for k in OPTIONS])
    out = (ctypes.c_int * 64)()
    n = _lib.lib().davo_decide_layer(1 if precision == "f16x3" else 0, li, H, W, NB, width, int(fuse_pose), arr, len(OPTIONS), out, 64)
    assert n > 0, (n, precision, li, H, W, NB, width, fuse_pose, options)
    steps = [dict(zip(STEP, out[1 + i * len(STEP):1 + (i + 1) * len(STEP)])) for i in range(out[0])]
    assert n == 1 + out[0] * len(STEP) + len(TAIL) <= 64
    d = dict(zip(TAIL, out[n - len(TAIL):n]))
    d["steps"] = steps
    return d


def fuses(precision, li, H, W, B, fuse_pose, width=128):
    """Whether the forward fuses the pose head into this layer's launch, as davo_decide_forward reports it for cnv7 of the flagship."""
    cfg = FP.parse_version(FP.FLOW.replace("-cnv6_128", "-cnv6_%d" % width))
    return bool(FP.decide_forward(FP.call_of(cfg, H, W, B, precision), fuse_pose=fuse_pose)["layers"][li]["fuse_pose"])


def check_structure(d, precision, li, H, W, NB, what, width=128):
    M = layer_rows(li, H, W, NB)
    steps = d["steps"]
    assert 1 <= len(steps) <= 2, what
    assert not steps[0]["rem_label"], what                             # a `.rem' step never comes first
    at = 0
    for s in steps:                                                    # the steps' row ranges partition [0, M)
        assert s["row0"] == at and s["m_end"] > at, (what, s)
        at = s["m_end"]
        assert s["family_ok"] == 1, (what, s)
        rows = s["m_end"] - s["row0"]
        if s["family"] == H3_MAINREM:                                  # 256-row main tiles, then 128-row remainder tiles
            assert s["row0"] == 0 and s["n_main"] * 256 == s["rem_mtile0"] * 128 and s["gx"] == s["n_main"] + s["n_rem"], (what, s)
            assert s["n_rem"] == -(-(s["m_end"] - s["n_main"] * 256) // 128) * s["rem_ntiles_n"], (what, s)
        elif s["family"] == F32_MAINREM:
            assert s["n_main"] == (s["rem_mtile0"] - s["mtile0"]) * s["ntiles_n"] and s["n_rem"] == -(-(s["m_end"] - s["rem_mtile0"] * 128) // 128) * s["rem_ntiles_n"], (what, s)
        elif s["family"] in (F32, F32_N256):
            assert s["mtile0"] * 128 == s["row0"] and s["gx"] == -(-rows // 128) * s["ntiles_n"], (what, s)
        else:
            bm = 256 if s["family"] in (H3W, H3W64, H3W128) else TILE_BM[s["tile"]]
            assert s["mtile0"] * bm == s["row0"] and s["gx"] == -(-rows // bm) * s["ntiles_n"], (what, s)
    assert at == M, (what, at, M)
    # the plan codes decode to the steps' tiles; a merged grid reports one launch over the layer: mark 7 (f16x3) or its main tile's columns
    codes = [c for c in (d["code0"], d["code1"]) if c]
    assert len(codes) == len(steps) and d["code0"], (what, d)
    for c, s in zip(codes, steps):
        want = 7 if s["family"] == H3_MAINREM else 128 if s["family"] == F32_MAINREM else s["tile"]
        assert c % 1000 == want and c // 1000 == -(-(s["m_end"] - s["row0"]) // 128), (what, c, s)
    if precision == "f16x3" and steps[0]["family"] == H3_SPLITK:       # whole channel blocks and whole filter rows per part
        s = steps[0]
        assert d["split"] in (2, 4) and s["gy"] == d["split"] and s["nchunks"] * d["split"] == d["nchunks_h"], (what, d)
        assert s["nchunks"] % d["cpb"] == 0 and s["nchunks"] % 3 == 0 and d["splitk_floats"] == M * d["split"] * LAYER_COUT(width)[li], (what, d)
    else:
        assert d["split"] == 1 and d["splitk_floats"] == 0 and not d["fold_if_xcd"], (what, d)


def decided_layers(row):
    """Layers of a recorded forward that went through the decisions: cnv4..cnv7, and cnv1..cnv3 where their patch kernel is off
    (f16x3 cnv1 has no switch in the product build; a forced tile that fits takes cnv2 / cnv3 off their patch kernels too)."""
    o = row["options"]
    cout = LAYER_COUT(row["width"])
    if row["precision"] == "f32":
        return list(range(7)) if o.get("patch_f32", 1) == 0 else [3, 4, 5, 6]
    ft = o.get("force_tile", -1)
    forced = lambda li: ft >= 0 and cout[li] >= TILE_BN[ft]
    return [li for li in (1, 2) if o.get("patch_cnv%d" % (li + 1), 1) == 0 or forced(li)] + [3, 4, 5, 6]


with open(GOLDEN) as f:
    ROWS = json.load(f)["rows"]


def test_the_option_positions_and_defaults_are_the_library_table():
    """OPTIONS[:14] and their DEFAULTS, as typed out above, are rows 0..13 of the library's option table (davo_option_info)."""
    assert _lib.option_table()[:14] == [(k, DEFAULTS[k]) for k in OPTIONS[:14]]


def test_pad_classes_default_leaves_cnv4_on_the_natural_order():
    """A new context sorts cnv5 and cnv6 by padding class, not cnv4 (mask 6), and that is what the hook decides with no options; mask
    7 takes cnv4 along.  B = 32 at 128x416 has class tables for all three layers (test_pad_classes_gpu.py)."""
    assert [decide("f32", li, 128, 416, 64)["pad_classes"] for li in (3, 4, 5)] == [0, 1, 1]
    assert decide("f32", 3, 128, 416, 64, pad_classes=7)["pad_classes"] == 1


def row_id(r):
    return "%s-%s-cnv6_%d-%dx%d-B%d-fuse_pose%d" % (r["group"], r["precision"], r["width"], r["H"], r["W"], r["B"], r["fuse_pose"])


def test_table_covers_the_cases():
    """The recorded table holds the default shapes and every option row of test_plan_layers_gpu.py in both pose-head forms, the cnv6
    width cases, and the batch sizes forward.hip's comments name as plan boundaries."""
    import test_plan_layers_gpu as TP
    have = {(r["group"], r["precision"], r["width"], r["H"], r["W"], r["B"], r["fuse_pose"]) for r in ROWS}
    for prec in TP.PRECISIONS:
        for H, W, B in TP.DEFAULT_PLANS:
            assert all(("default", prec, 128, H, W, B, fp) in have for fp in (0, 1))
        for H, W, Bs in ((128, 416, (1, 2, 4, 24, 40)), (256, 832, (6, 8))):
            assert all(("boundary", prec, 128, H, W, B, 1) in have for B in Bs)
        for width in CW.WIDTHS:
            for H, W, B in [c[:3] for c in CW.CASES[width] + CW.SPLIT_K_CASES[width]]:
                assert all(("cnv6_width", prec, width, H, W, B, fp) in have for fp in (0, 1))
    for prec, table in (("f16x3", TP.F16X3_OPTIONS), ("f32", TP.F32_OPTIONS)):
        for name, B, H, W, options, _ in table:
            rows = [r for r in ROWS if r["group"] == "option:" + name and r["precision"] == prec]
            assert sorted(r["fuse_pose"] for r in rows) == [0, 1] and all(r["options"] == options and (r["H"], r["W"], r["B"]) == (H, W, B) for r in rows), name


@pytest.mark.parametrize("row", ROWS, ids=row_id)
def test_recorded_row(row):
    """The hook reproduces the recorded last_plan, last_split and launch counts of every layer that is decided here, and each of
    those decisions has the structural properties."""
    H, W, NB = row["H"], row["W"], 2 * row["B"]
    options = {k: v for k, v in row["options"].items() if k not in NOT_DECISION_OPTIONS}
    for li in decided_layers(row):
        what = (row_id(row), li)
        d = decide(row["precision"], li, H, W, NB, row["width"], fuses(row["precision"], li, H, W, row["B"], row["fuse_pose"], row["width"]), max_batch=row["B"], **options)
        check_structure(d, row["precision"], li, H, W, NB, what, row["width"])
        assert [[c // 1000, c % 1000] for c in (d["code0"], d["code1"]) if c] == row["last_plan"][li], what
        assert d["split"] == row["last_split"][li], what
        name = "cnv%d" % (li + 1)
        for label, rem in ((name, 0), (name + ".rem", 1)):
            assert sum(1 for s in d["steps"] if s["rem_label"] == rem) == row["launches"].get(label, 0), (what, label)


# options no GPU test takes: fewer compute units than the device has (CU-masked slot streams) and the partition switch itself
CPU_ONLY = [dict(ncu=n) for n in (32, 64, 104, 128, 208)] + [dict(ncu=128, cu_partition=1), dict(ncu=64, cu_partition=1, fold_fixup=1),
                                                            dict(ncu=128, user_stream=1, fold_fixup=1), dict(ncu=128, wave128=3, merge_cnv4=1)]


@pytest.mark.parametrize("options", CPU_ONLY, ids=lambda o: "-".join("%s%d" % kv for kv in o.items()))
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
def test_structure_with_fewer_compute_units(precision, options):
    for H, W, Bs in ((128, 416, (1, 2, 3, 5, 8, 24, 32, 128)), (256, 832, (1, 6)), (36, 100, (2,))):
        for B in Bs:
            for li in range(7):
                for fuse_pose in (0, 1):
                    d = decide(precision, li, H, W, 2 * B, 128, fuses(precision, li, H, W, B, fuse_pose), max_batch=B, **options)
                    check_structure(d, precision, li, H, W, 2 * B, (precision, options, H, W, B, li, fuse_pose))
                    assert not d["fold_if_xcd"], (options, H, W, B, li)       # never folded on a share of the device's compute units


def test_structure_of_the_feature_attention_cnv6():
    """cnv6 as one group per head reading 512 channels (davo_set_posenn_se), and the pose tail in cnv7's launch."""
    for precision in ("f16x3", "f32"):
        for B in (1, 2, 5, 32):
            d = decide(precision, 5, 128, 416, 2 * B, 128, 0, posenn_se=1)
            check_structure(d, precision, 5, 128, 416, 2 * B, (precision, B))
            # the four-wave tiles, the f16x3 merged grid and split-K are single-group kernels
            assert d["split"] == 1 and all(s["family"] in (H3, H3S, F32, F32_MAINREM) and s["gy"] == (2 if s["family"] != F32_MAINREM else 1) for s in d["steps"]), d
    d = decide("f16x3", 6, 128, 416, 4, 128, 1, pose_tail=1)
    assert d["pose_floats"] == 2 * d["pose_mt"] * d["pose_ntn"] * 6 and d["pose_bm"] <= 13 * 52 and len(d["steps"]) == 1, d


def test_arguments_are_checked():
    out = (ctypes.c_int * 64)()
    L = _lib.lib()
    assert L.davo_decide_layer(1, 7, 128, 416, 2, 128, 0, None, 0, out, 64) < 0
    assert L.davo_decide_layer(2, 3, 128, 416, 2, 128, 0, None, 0, out, 64) < 0
    assert L.davo_decide_layer(1, 3, 128, 416, 0, 128, 0, None, 0, out, 64) < 0
    assert L.davo_decide_layer(1, 3, 128, 416, 2, 128, 0, None, 0, None, 0) < 0
    n = L.davo_decide_layer(1, 3, 128, 416, 2, 128, 0, None, 0, out, 64)          # no options given: a new context's
    assert n == 1 + out[0] * len(STEP) + len(TAIL)
    # ... which is the record of DEFAULTS spelt out; so is float32 cnv4's at B = 32, where mask 6 and mask 7 decide differently
    spelt = (ctypes.c_int * len(OPTIONS))(*[DEFAULTS[k] for k in OPTIONS])
    for precision, NB in ((1, 2), (0, 64)):
        full = (ctypes.c_int * 64)()
        n = L.davo_decide_layer(precision, 3, 128, 416, NB, 128, 0, None, 0, out, 64)
        assert n > 0 and L.davo_decide_layer(precision, 3, 128, 416, NB, 128, 0, spelt, len(OPTIONS), full, 64) == n and out[:n] == full[:n]
