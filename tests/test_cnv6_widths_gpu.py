"""The cnv6 widths 32, 64 and 256 layer by layer against float64 (tests/layer_check.py), on every plan cnv6 takes at them
(tests/cnv6_width_cases.py; tests/test_cnv6_widths.py keeps that table complete).  cnv6 is a GEMM of N = 64, 128 or 512
columns there and cnv7 reads 32, 64 or 256 channels per head, so these launches are not the flagship's: other tiles on a
K = 2304 layer, the 256x256 tile with two N tiles, cnv7's group offset after 1, 2 or 8 channel blocks, cnv7's rings on 9
and 72 chunks.  Built like tests/test_plan_layers_gpu.py: each table case in f16x3, the launch options where these widths
branch away from the flagship, float32 with its merged and unmerged grids to the bit, the f16x3 sibling launches to the bit,
and the range record against what was stored.  Split-K partial sums of parts x 64, 128 and 512 columns: at 128x416 only
width 32 has few enough tiles at B = 1, so every width also runs on two small ragged maps where Engine.last_split shows that
cnv6 did split (test_split_k_on_small_maps), with tiles that straddle images and a last tile cut short."""
import numpy as np
import pytest

from davo_amd import synth

import cnv6_width_cases as CW
import layer_check as LC
import test_plan_layers_gpu as TP

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """As in tests/test_plan_layers_gpu.py: the worst bar-(b) ratio per precision and layer over this module."""
    yield from LC.report_worst_ratios("test_cnv6_widths_gpu")


def _both_pose_heads(e, cfg, inputs, precision, what, plan_check, H=128, W=416):
    """fuse_pose 0 and 1: all layers and the pose, cnv7 stored exactly when the head is not fused.  A layer the second
    forward stored as the same bits from the same input is not convolved again (LC.check_forward, checked)."""
    checked = {}
    B = inputs[0].shape[0]
    for fuse_pose in (0, 1):
        e.set_option("fuse_pose", fuse_pose)
        stats = TP._run(e, cfg, inputs, precision, "%s fuse_pose %d" % (what, fuse_pose), images="plan" if B > 8 else None,
                        plan_check=plan_check, checked=checked)
        fused = TP._fuses(H, W, fuse_pose)
        assert ("cnv7" in stats) != fused and ("pose(fused)" in stats) == fused, (what, fuse_pose, stats)
        assert "cnv6" in stats


# ---- every plan of the table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,H,W,B,tiles", [pytest.param(*c, id=CW.case_id(*c[:4])) for c in CW.cases()])
def test_table_case_f16x3(width, H, W, B, tiles):
    """cnv6 runs the tiles the table names (no merged grid at these widths: tile 7 is never reported; width 64 at B = 112
    has the merged grid's shape and keeps its two launches), split-K (B = 1) reports the planner's tile."""
    cfg = CW.config(width)
    inputs = synth.make_inputs(B, H, W, first_window=7)
    e = TP._engine(cfg, H, W, B, "f16x3")
    _both_pose_heads(e, cfg, inputs, "f16x3", CW.case_id(width, H, W, B), TP._plan_is(5, list(tiles)), H, W)
    e.close()


# ---- launch options where these widths leave the flagship's branch --------------------------------------------------
def _cnv6_is(width, B):
    return TP._plan_is(5, list(CW.case(width, B)))


def _cnv7_on_208(width, B):
    """force_tile 6: cnv6 is not 256 columns wide, so it keeps the planner's tiles; cnv7 (256 per head) takes the tile."""
    return lambda e: TP._tiles(5)(e) == list(CW.case(width, B)) and TP._tiles(6)(e) == [6]


def _cnv6_split(width, B):
    """"split_k" 1 at 128x416, B = 1: cnv5 (104 tiles of 128x128) splits at every width, cnv6 only at width 32 (104 tiles
    of 128x32; widths 64 and 256 run 208).  The widths that do not split here do in test_split_k_on_small_maps."""
    return lambda e: _cnv6_is(width, B)(e) and e.last_split(4) > 1 and (e.last_split(5) > 1) == (width == 32)


def _unsplit(width, B):
    return lambda e: _cnv6_is(width, B)(e) and e.last_split(4) == 1 and e.last_split(5) == 1


OPTIONS = [
    # (id, B, options in order, check of last_plan given the width)
    ("split_k0", 1, {"split_k": 0}, _unsplit),
    ("split_k1", 1, {"split_k": 1}, _cnv6_split),
    ("fold_fixup", 1, {"split_k": 1, "fold_fixup": 1}, _cnv6_split),
    ("deep_ring0", 2, {"deep_ring": 0}, _cnv6_is),
    ("deep_ring1", 2, {"deep_ring": 1}, _cnv6_is),
    ("share_taps0", 5, {"share_taps": 0}, _cnv6_is),
    ("force_tile6_B2", 2, {"force_tile": 6}, _cnv7_on_208),
    ("force_tile6_B5", 5, {"force_tile": 6}, _cnv7_on_208),
    ("wave128_0", 32, {"wave128": 0}, _cnv6_is),
]
# width 256: the 256x256 tile with two N tiles in one launch.  At 128x416 an image is 3328 = 13 x 256 rows, so no tile of
# B = 5 holds rows of two images; at 64x96 an image is 384 rows and every second tile of B = 3 (9 tiles) straddles two
_ON_TILE_5 = lambda width, B: (lambda e: TP._tiles(4)(e) == [5] and TP._tiles(5)(e) == [5])
OPTION_CASES = [pytest.param(w, c[0], c[1], 128, 416, *c[2:], id="cnv6_%d-%s" % (w, c[0])) for w in CW.WIDTHS for c in OPTIONS] + \
               [pytest.param(256, "force_tile5", 5, 128, 416, {"split_k": 0, "force_tile": 5}, _ON_TILE_5, id="cnv6_256-force_tile5"),
                pytest.param(256, "force_tile5", 3, 64, 96, {"split_k": 0, "force_tile": 5}, _ON_TILE_5, id="cnv6_256-force_tile5-64x96")]


@pytest.mark.parametrize("width,name,B,H,W,options,plan_check", OPTION_CASES)
def test_launch_option_f16x3(width, name, B, H, W, options, plan_check):
    cfg = CW.config(width)
    inputs = synth.make_inputs(B, H, W, first_window=3)
    e = TP._engine(cfg, H, W, B, "f16x3")
    for k, v in options.items():
        e.set_option(k, v)
    _both_pose_heads(e, cfg, inputs, "f16x3", "cnv6_%d %s %dx%d B=%d" % (width, name, H, W, B), plan_check(width, B), H, W)
    e.close()


# ---- split-K where cnv6 really splits ---------------------------------------------------------------------------------
SPLIT_K_CASES = [pytest.param(w, *c[:4], id="cnv6_%d-%dx%d-B%d" % ((w,) + c[:3])) for w in CW.WIDTHS for c in CW.SPLIT_K_CASES[w]]


@pytest.mark.parametrize("width,H,W,B,tiles", SPLIT_K_CASES)
def test_split_k_on_small_maps(width, H, W, B, tiles):
    """cnv6 as one launch of at most 128 tiles (tests/test_cnv6_widths.py checks the count): "split_k" 0 is one chain over
    K, "split_k" 1 runs 2 or 4 parts into float32 partial sums of parts x 2 x width columns that splitk_fixup adds,
    "fold_fixup" 1 lets a tile's last part add them.  Each layer by layer with both pose heads; last_split says which ran
    (last_plan names the same tile every time).  The maps are ragged: 128-row tiles straddle images and the last is cut."""
    cfg = CW.config(width)
    inputs = synth.make_inputs(B, H, W, first_window=3)
    e = TP._engine(cfg, H, W, B, "f16x3")
    sh = LC.shapes(cfg, H, W)
    stored = {}
    for name, split_k, fold in (("split_k0", 0, 0), ("split_k1", 1, 0), ("fold_fixup", 1, 1)):
        e.set_option("split_k", split_k)
        e.set_option("fold_fixup", fold)
        ran = lambda e: TP._tiles(5)(e) == list(tiles) and (e.last_split(5) in (2, 4) if split_k else e.last_split(5) == 1)
        _both_pose_heads(e, cfg, inputs, "f16x3", "cnv6_%d %dx%d B=%d %s" % (width, H, W, B, name), ran, H, W)
        print("cnv6_%d %dx%d B=%d %s: cnv5 in %d parts, cnv6 in %d" % (width, H, W, B, name, e.last_split(4), e.last_split(5)))
        stored[name] = e.debug_read("cnv6", (2 * B,) + sh["cnv6"]).copy()
    # the same partial sums added in the same order by splitk_fixup and by the tile's last part
    assert np.array_equal(stored["split_k1"], stored["fold_fixup"])
    e.close()


# ---- float32 ---------------------------------------------------------------------------------------------------------
# Launches of (cnv6, cnv7) as two launches each where plan_layer (plan.hip) splits off a remainder, by width and B:
# cnv6 has 52 B M tiles of N = 64 / 128 / 512 columns, cnv7 13 B M tiles of 256 columns in two groups, a round is 512 tiles
# of 128 columns.  "merge_rem_f32" 1 makes one grid of cnv6's two launches where the main tile is 128 columns wide
# (not width 32: N = 64); cnv7 keeps its two.
F32_LAUNCHES = {(32, 2): (1, 1), (32, 5): (1, 1), (32, 32): (2, 2),
                (64, 2): (1, 1), (64, 5): (1, 1), (64, 32): (2, 2),
                (256, 2): (1, 1), (256, 5): (2, 1), (256, 32): (1, 2)}


def _f32_launches(width, B, merge):
    n6, n7 = F32_LAUNCHES[(width, B)]
    if merge and width != 32:
        n6 = 1
    return lambda e: (len(e.last_plan(5)), len(e.last_plan(6))) == (n6, n7)


@pytest.mark.parametrize("B", [2, 5, 32])
@pytest.mark.parametrize("width", CW.WIDTHS)
def test_f32(width, B):
    """float32 kernels, default options (merge_rem_f32 1), both pose heads, layer by layer."""
    cfg = CW.config(width)
    H, W = 128, 416
    inputs = synth.make_inputs(B, H, W, first_window=5)
    e = TP._engine(cfg, H, W, B, "f32")
    _both_pose_heads(e, cfg, inputs, "f32", "cnv6_%d f32 B=%d" % (width, B), _f32_launches(width, B, 1))
    e.close()


@pytest.mark.parametrize("B", [5, 32])
@pytest.mark.parametrize("width", CW.WIDTHS)
def test_f32_merged_and_unmerged_grids_are_bit_identical(width, B):
    """merge_rem_f32 0 (main + remainder launches, checked layer by layer) and 1 (one grid where cnv6's main tile is 128
    columns wide): the same tiles' float32 chains, so the same bits in stored cnv6, cnv7 and the poses.  Width 256 has its
    two-launch cnv6 at B = 5, widths 32 and 64 at B = 32."""
    cfg = CW.config(width)
    H, W = 128, 416
    inputs = synth.make_inputs(B, H, W, first_window=5)
    e = TP._engine(cfg, H, W, B, "f32")
    e.set_option("fuse_pose", 0)
    sh = LC.shapes(cfg, H, W)
    e.set_option("merge_rem_f32", 0)
    base = LC.forward(e, *inputs).copy()
    assert _f32_launches(width, B, 0)(e), [e.last_plan(li) for li in range(7)]
    stats = LC.check_forward(e, cfg, TP._weights(cfg), *inputs, base, "f32", images="plan" if B > 8 else None,
                             what="cnv6_%d f32 B=%d merge_rem_f32 0" % (width, B))
    assert "cnv7" in stats
    acts = {k: e.debug_read(k, (2 * B,) + sh[k]).copy() for k in ("cnv6", "cnv7")}
    e.set_option("merge_rem_f32", 1)
    got = LC.forward(e, *inputs)
    assert _f32_launches(width, B, 1)(e), [e.last_plan(li) for li in range(7)]
    for k in acts:
        assert np.array_equal(e.debug_read(k, (2 * B,) + sh[k]), acts[k]), k
    assert np.array_equal(got, base)
    e.close()


# ---- f16x3 siblings to the bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(3, 64, 96), (2, 128, 416)])
@pytest.mark.parametrize("width", CW.WIDTHS)
def test_f16x3_siblings_are_bit_identical(width, B, H, W):
    """share_taps 0 / 1, deep_ring 0 / 1 and cnv7 on the 208x256 tile against the default: the same products reach every
    accumulator in the same order (tests/test_hip_parity.py: test_shared_tap_staging_is_bit_identical,
    test_deep_ring_is_bit_identical, test_tile_208x256_forced), so stored cnv6 and cnv7 are the same bits.  split_k 0: one K
    chain, as those tests have it where a launch option moves a layer between plans."""
    cfg = CW.config(width)
    inputs = synth.make_inputs(B, H, W, first_window=11)
    e = TP._engine(cfg, H, W, B, "f16x3")
    e.set_option("fuse_pose", 0)
    e.set_option("split_k", 0)
    sh = LC.shapes(cfg, H, W)
    read = lambda: {k: e.debug_read(k, (2 * B,) + sh[k]).copy() for k in ("cnv6", "cnv7")}
    base_pose = LC.forward(e, *inputs).copy()
    base = read()
    plan6 = e.last_plan(5)
    assert TP._tiles(6)(e) != [6]
    for options in ({"share_taps": 0}, {"deep_ring": 0}, {"share_taps": 0, "deep_ring": 0}, {"force_tile": 6}):
        for k, v in options.items():
            e.set_option(k, v)
        got = LC.forward(e, *inputs)
        acts = read()
        if "force_tile" in options:
            assert TP._tiles(6)(e) == [6] and e.last_plan(5) == plan6, [e.last_plan(li) for li in range(7)]
        for k in base:
            assert np.array_equal(acts[k], base[k]), (options, k)
        assert np.array_equal(got, base_pose), options
        for k, v in {"share_taps": 1, "deep_ring": 1, "force_tile": -1}.items():
            e.set_option(k, v)
    e.close()


# ---- the range record ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,B", [(32, 20), (64, 10), (256, 5)])
def test_range_record(width, B):
    """The range record of every stored layer against what its kernels stored, cnv6 on 64, 128 and 512 columns and as two
    launches (the smallest two-launch case of each width): unscaled, and with every layer's maximum at the guard's floor."""
    cfg = CW.config(width)
    H, W = 128, 416
    inputs = synth.make_inputs(B, H, W, first_window=3)
    e = TP._engine(cfg, H, W, B, "f16x3")
    what = "cnv6_%d B=%d" % (width, B)
    _, maxima = LC.range_record_forward(e, *inputs)
    assert len(e.last_plan(5)) == 2, e.last_plan(5)
    LC.check_range_record(e, cfg, B, H, W, maxima, what)
    shifts = LC.edge_shifts(maxima, "floor")
    _, rec = LC.range_record_forward(e, *inputs, shifts)
    assert e.activation_range()[1] == shifts
    where = LC.check_range_record(e, cfg, B, H, W, rec, what + " floor")
    assert len(where["cnv6"][1]) == 2, where["cnv6"]
    e.close()
