"""The launch sequence of a forward (csrc/plan.h: decide_forward) through davo_decide_forward, on the CPU: structural properties of
every row of tests/forward_plan_cases.py, and tests/golden/forward_launches.json - what the build before the forward's launches were
decided apart from their issuing reported through the profile, Engine.last_plan and Engine.last_split on an MI355X - row by row,
reproduced from davo_decide_forward and davo_decide_layer together."""
import collections
import json
import os

import pytest

import forward_plan_cases as FP
from test_layer_decision import decide

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_launches.json")
with open(GOLDEN) as f:
    RECORDED = {row["id"]: row for row in json.load(f)["rows"]}

CONV = ("cnv1", "cnv2", "cnv3", "cnv4", "cnv5", "cnv6", "cnv7")
FRONT_LABELS = ("se_pool_squeeze", "se_pool_excite", "se_depth_squeeze", "se_class_squeeze", "se_squeeze_partial", "se_excite", "se_excite_far")
STAGE = dict([(k, 0) for k in FRONT_LABELS] + [("mask_pack", 1)] + [(k, 2 + i) for i, k in enumerate(CONV[:5])] +
             [(k, 7) for k in ("se5_squeeze", "se5_excite", "se5_scale")] + [("cnv6", 8), ("cnv7", 8), ("pose_head", 9), ("range_guard_snapshot", 10)])
# options of a row that davo_decide_layer takes (the others choose between runners, or are davo_decide_forward's alone)
LAYER_OPTIONS = {"force_tile", "split_k"}


def test_the_table_is_the_recorded_one():
    assert [FP.row_id(r) for r in FP.ROWS] == list(RECORDED)
    assert set(STAGE) == set(FP.labels())


def test_the_option_positions_and_defaults_are_the_library_table():
    """The first seven PLAN_DEFAULTS, as forward_plan_cases.py types them out, are rows 14..20 of the library's option table."""
    assert FP._lib.option_table()[14:] == list(FP.PLAN_DEFAULTS.items())[:7]


def test_the_table_covers_the_rules():
    """Every front kind in both precisions on both sides of the fold boundary, the three PoseNN forms in both precisions and in
    impl 1 where it has one, one pair, each value of the options the sequence reads, both ways the snapshot travels."""
    have = {(r.variant, r.B <= 2, r.precision) for r in FP.ROWS if not r.options and not r.impl}
    for variant in ("flow", "class", "depth", "split", "pooled"):
        assert all((variant, small, prec) in have for small in (True, False) for prec in ("f16x3", "f32")), variant
    assert {r.B for r in FP.ROWS if r.variant == "flow" and (r.H, r.W) == FP.BIG and not r.options} >= {1, 2, 3}
    for variant in ("triplet", "coupled", "insert"):
        assert {r.precision for r in FP.ROWS if r.variant == variant and not r.impl} == {"f16x3", "f32"}, variant
    assert {r.variant for r in FP.ROWS if r.impl} == {"flow", "coupled", "insert"}
    assert {r.variant for r in FP.ROWS if r.pairs == "src0"} >= {"flow", "class"}
    values = collections.defaultdict(set)
    for r in FP.ROWS:
        for k, v in r.options.items():
            values[k].add(v)
    assert values["fold_tails"] == {0, 1, 2} and values["fuse_pack"] == {1} and values["fuse_pose"] == {0}
    assert all(values[k] == {0} for k in ("patch_cnv2", "patch_cnv3", "patch_f32", "patch_cnv1_t"))
    ticketed = [FP.plan_of(r) for r in FP.ROWS if r.entry == "device" and r.precision == "f16x3"]
    assert {(p["head"] == FP.HEAD_TILES, bool(p["snapshot_launch"])) for p in ticketed} == {(True, False), (False, True)}


def check_structure(p, r, what):
    mode = FP.mode_of(r)
    launches, layers = p["launches"], p["layers"]
    # the front, the packer, cnv1..cnv5, the feature-attention block, cnv6 and cnv7 (impl 1: per head), the head, the snapshot
    stages = [STAGE[k] for k in launches]
    assert stages == sorted(stages), (what, launches)
    conv = [k for k in launches if k in CONV]
    groups = layers[5]["ngroups"]
    assert conv == list(CONV[:5]) + ["cnv6", "cnv7"] * groups and layers[6]["ngroups"] == groups, (what, launches)
    assert groups == (2 if mode == "direct" and r.variant != "coupled" else 1), what
    front = [k for k in launches if k in FRONT_LABELS]
    assert 1 <= len(front) <= 3 and len(set(front)) == len(front), (what, front)
    assert FP.FRONTS[p["front"]] == FP.FRONT_OF[r.variant] or FP.FRONT_OF[r.variant] == "none", what
    assert ("se_excite" in front) == bool(p["excite"]) and ("se_excite_far" in front) == bool(p["excite_far"]), what
    assert not (p["fold_excite"] and (p["excite"] or p["excite_far"])) and (not p["excite_far"] or FP.FRONTS[p["front"]] == "split"), what
    assert ("se_pool_excite" in front) == (FP.FRONTS[p["front"]] == "pooled") and bool(p["squeeze"]) == (front[0] not in ("se_excite",)), what
    # the packer: none exactly where cnv1 builds its patch from the raw inputs
    assert launches.count("mask_pack") == (p["pack"] != FP.PACK_NONE), what
    assert (p["pack"] == FP.PACK_NONE) == (layers[0]["runner"] == FP.RUN_PATCH_FUSED) == (not p["packed_valid"]), what
    assert (p["pack"] == FP.PACK_TRIPLET) == (r.variant == "triplet") and p["pack_ld"] == {"f16x3": 16, "f32": 8, "direct": 10}[mode], what
    # the records chain: each layer reads the one before, at its channels and map size
    assert layers[0]["x_buf"] == FP.BUF_PACKED and layers[0]["x_ch"] == p["packed_ld"] and (layers[0]["Hin"], layers[0]["Win"]) == (r.H, r.W), what
    for li in range(1, 7):
        a, b = layers[li - 1], layers[li]
        assert (b["Hin"], b["Win"]) == (a["Hout"], a["Wout"]), (what, li)
        if li == 5 and p["se5"]:
            assert b["x_buf"] == FP.BUF_SE and b["x_ch"] == 2 * a["y_ld"], (what, li)
        else:
            assert b["x_buf"] == li - 1 and b["x_ch"] == a["y_ld"], (what, li)
    for li, rec in enumerate(layers):
        assert rec["label"] == FP.labels().index(CONV[li]), (what, li)
        assert (rec["Hout"], rec["Wout"]) == tuple(-(-n // (2 if li in (0, 1, 6) else 1)) for n in (rec["Hin"], rec["Win"])), (what, li)
        assert rec["y_f32"] == (mode != "f16x3" or li == 6), (what, li)
        want = {"f16x3": FP.RUN_IGEMM_H3, "f32": FP.RUN_IGEMM_F32, "direct": FP.RUN_DIRECT}[mode]
        assert rec["runner"] == want or (li < 3 and mode != "direct" and rec["runner"] in (FP.RUN_PATCH, FP.RUN_PATCH_FUSED, FP.RUN_PATCH_CNV1T)), (what, li)
        assert bool(rec["plan_code"]) == (rec["runner"] <= FP.RUN_PATCH_CNV1T), (what, li)
        if li < 6:
            assert not (rec["fuse_pose"] or rec["pose_tail"] or rec["pose_six"]), (what, li)
        if mode == "direct":
            for g in range(rec["ngroups"]):
                assert rec["x_coff%d" % g] + rec["cin"] <= rec["x_ch"] and rec["y_coff%d" % g] + rec["cout"] <= rec["y_ld"], (what, li, g)
            assert rec["ngroups"] * rec["cout"] == rec["y_ld"], (what, li)
    assert bool(p["se5"]) == (r.variant == "insert") == ("se5_scale" in launches), what
    # the fuse_pose rule: asked for, a map of at least one 128-row tile per image, the pair topology, an epilogue of the head's width
    c7 = layers[6]
    fused = bool(c7["fuse_pose"])
    asked = r.options.get("fuse_pose", 1)
    assert fused == (mode != "direct" and asked and c7["Hout"] * c7["Wout"] >= 128 and r.variant != "triplet" and
                     not (r.variant == "coupled" and mode == "f32")), what
    assert fused == (not p["cnv7_valid"]) == (p["head"] != FP.HEAD_TWO_PASS) and bool(c7["pose_six"]) == (fused and r.variant == "coupled"), what
    assert (p["head"] == FP.HEAD_TAIL) == (fused and r.options.get("fold_tails") == 1) == ("pose_head" not in launches), what
    assert bool(c7["pose_tail"]) == (mode == "f16x3" and r.options.get("fold_tails") == 1), what
    assert (p["cols"], p["heads"]) == {"triplet": (6, 2), "coupled": (6, 1)}.get(r.variant, (3, 2)), what
    assert p["NB"] == r.B * (1 if r.variant == "triplet" or r.pairs != "both" else 2), what


@pytest.mark.parametrize("r", FP.ROWS, ids=FP.row_id)
def test_structure(r):
    what = FP.row_id(r)
    p = FP.plan_of(r)
    check_structure(p, r, what)
    h3 = FP.mode_of(r) == "f16x3"
    # the snapshot: wanted by every f16x3 batch, carried by pose_from_tiles or by a launch of its own, never both
    assert (p["launches"].count("range_guard_snapshot") == 1) == bool(p["snapshot_launch"]) == (h3 and p["head"] != FP.HEAD_TILES), what
    assert not FP.plan_of(r, want_snapshot=0)["snapshot_launch"], what
    # the record reset: exactly one launch of a ticketed f16x3 batch, the one that evaluates the tables; nobody's otherwise
    z = FP.plan_of(r, zero_record=1)
    if h3:
        name = FP.labels()[z["reset_at"]]
        assert z["launches"].count(name) == 1 and STAGE[name] == 0, (what, name)
        assert name == ("se_pool_excite" if FP.FRONTS[z["front"]] == "pooled" else "se_excite" if z["excite"] else z["launches"][0]), (what, name)
    else:
        assert z["reset_at"] == -1, what
    assert FP.plan_of(r, zero_record=0)["reset_at"] == -1, what
    z.pop("reset_at"), p.pop("reset_at")
    assert z == p, what                                             # and the reset changes nothing else


def reproduce(r):
    """What a forward of the row launches, from davo_decide_forward and, for the layers on the implicit GEMM, davo_decide_layer."""
    p = FP.plan_of(r)
    cfg = FP.parse_version(FP.VERSIONS[r.variant])
    launches = collections.Counter(k for k in p["launches"] if k not in CONV and k not in FP.UNPROFILED)
    last_plan, last_split = [], []
    for li, rec in enumerate(p["layers"]):
        issued = p["launches"].count(CONV[li])
        if rec["runner"] == FP.RUN_DIRECT:                           # no plan code, no split: a new context's zeros
            launches[CONV[li]] += issued
            last_plan.append([])
            last_split.append(0)
        elif rec["runner"] <= FP.RUN_PATCH_CNV1T:
            launches[CONV[li]] += issued
            last_plan.append([[rec["plan_code"] // 1000, rec["plan_code"] % 1000]])
            last_split.append(1)
        else:
            options = {k: v for k, v in r.options.items() if k in LAYER_OPTIONS}
            d = decide(r.precision, li, r.H, r.W, p["NB"], cfg.cnv6_out, rec["fuse_pose"], max_batch=r.B, pose_tail=rec["pose_tail"],
                       posenn_se=p["se5"], triplet=int(r.variant == "triplet"), coupled=int(r.variant == "coupled"), **options)
            assert issued == 1, (FP.row_id(r), li)
            for s in d["steps"]:
                launches[CONV[li] + (".rem" if s["rem_label"] else "")] += 1
            last_plan.append([[c // 1000, c % 1000] for c in (d["code0"], d["code1"]) if c])
            last_split.append(d["split"])
    return {"launches": dict(launches), "last_plan": last_plan, "last_split": last_split}


@pytest.mark.parametrize("r", FP.ROWS, ids=FP.row_id)
def test_recorded_row(r):
    want = RECORDED[FP.row_id(r)]
    got = reproduce(r)
    assert got["launches"] == want["launches"]
    assert got["last_plan"] == want["last_plan"]
    assert got["last_split"] == want["last_split"]


def test_refusals():
    """Every combination forward_device refused as an internal error, and impl 1 on the 6-channel input, is still refused; bad
    arguments are."""
    flow = FP.parse_version(FP.FLOW)
    ok = FP.call_of(flow, 128, 416, 2, "f16x3")
    assert isinstance(FP.decide_forward(ok), dict)
    triplet, coupled = (FP.call_of(FP.parse_version(FP.VERSIONS[k]), 128, 416, 2, "f16x3") for k in ("triplet", "coupled"))
    v0 = FP.call_of(FP.parse_version("v0-sharedNN-dilatedPoseNN-segmask-se_flow-abs_flow-fc_tanh"), 128, 416, 2, "direct")
    assert v0["cin_per_frame"] == 3
    refused = [dict(ok, pairs=0), dict(ok, pairs=4), dict(coupled, topology=1), dict(coupled, posenn_se=1), dict(triplet, pairs=1),
               dict(triplet, pairs=2), dict(triplet, mode=2), v0]
    for call in refused:
        assert FP.decide_forward(call) == -1, call                  # DAVO_ERR_INVALID
    assert isinstance(FP.decide_forward(dict(v0, mode=1)), dict)
    for call in (dict(ok, H=0), dict(ok, B=0), dict(ok, mode=3), dict(ok, att_source=99), dict(ok, topology=2), dict(ok, heads=2), dict(ok, cnv6_out=0)):
        assert FP.decide_forward(call) < 0, call
    assert FP.decide_forward(ok, force_tile=99) < 0
