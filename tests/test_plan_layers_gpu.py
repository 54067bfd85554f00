"""Every launch plan, layer by layer, against float64 (tests/layer_check.py): each conv layer's output against a float64
convolution of the GPU's own input to it, under bar (a) (5e-6 of the tensor max) and bar (b) (tau of each output's L1
mass); the packed inputs and attention tables against the oracle; the pose head (stored or fused) against float64 from
the GPU's last stored activation.  Default plans at the shapes and batch sizes that select them, every launch option at a
shape where it is taken, the float32 merged / unmerged grids to the bit, and the attention sources on labels placed on
the class-table squeeze's chunk boundaries."""
import numpy as np
import pytest

from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION

import layer_check as LC

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "f32"]
_WEIGHTS = {}


@pytest.fixture(scope="module", autouse=True)
def _report_worst_ratios():
    """The worst bar-(b) ratio per precision and layer over the module; written as JSON where DAVO_LAYER_RATIOS names a
    file (how TAU in layer_check.py was measured)."""
    yield from LC.report_worst_ratios("test_plan_layers_gpu")


def _weights(cfg):
    if cfg.version not in _WEIGHTS:
        _WEIGHTS[cfg.version] = synth.make_weights(cfg)
    return _WEIGHTS[cfg.version]


def _engine(cfg, H, W, B, precision):
    e = Engine(cfg, H, W, B)
    e.load_weights(_weights(cfg))
    e.set_precision(precision)
    return e


def _fuses(H, W, fuse_pose):
    """The pose head runs fused where asked and cnv7's map holds at least one 128-row tile per image (forward.hip)."""
    h7, w7, _ = LC.shapes(parse_version(FLAGSHIP_VERSION), H, W)["cnv7"]
    return bool(fuse_pose) and h7 * w7 >= 128


def _run(e, cfg, inputs, precision, what, images=None, stop_after=None, plan_check=None, checked=None):
    """checked: LC.check_forward's dict of the layers an earlier forward on the same inputs and images stored as the same bits."""
    poses = LC.forward(e, *inputs)
    if plan_check is not None:
        assert plan_check(e), (what, [e.last_plan(li) for li in range(7)])
    return LC.check_forward(e, cfg, _weights(cfg), *inputs, poses, precision, images=images, what=what, stop_after=stop_after,
                            checked=checked)


# ---- default plans -------------------------------------------------------------------------------------------------
DEFAULT_PLANS = [(128, 416, 1), (128, 416, 3), (128, 416, 32), (128, 416, 128), (256, 832, 2),
                 (36, 100, 2), (52, 172, 1), (20, 48, 5), (16, 16, 1)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,B", DEFAULT_PLANS)
def test_default_plan(H, W, B, precision):
    """The plan the library picks by itself: stored cnv7 (fuse_pose 0) with every pair image up to B = 32, then the fused
    pose head on the images a plan's launches start and end in (frames whose cnv7 map is under one 128-row tile per image
    never fuse: cnv7 is stored again); B = 128 in one piece on that subset both ways."""
    cfg = parse_version(FLAGSHIP_VERSION)
    inputs = synth.make_inputs(B, H, W, first_window=11)
    e = _engine(cfg, H, W, B, precision)
    for fuse_pose in (0, 1):
        e.set_option("fuse_pose", fuse_pose)
        what = "%dx%d B=%d %s fuse_pose %d" % (H, W, B, precision, fuse_pose)
        stats = _run(e, cfg, inputs, precision, what, images=None if fuse_pose == 0 else "plan")
        fused = _fuses(H, W, fuse_pose)
        assert ("cnv7" in stats) != fused and ("pose(fused)" in stats) == fused, stats
    e.close()


# ---- every launch option at a shape where it is taken ---------------------------------------------------------------
def _tiles(li):
    return lambda e: [t for _, t in e.last_plan(li)]


def _plan_is(li, want):
    return lambda e: _tiles(li)(e) == want


def _profiled_without_mask_pack(e):
    return "mask_pack" not in e.profile_entries() and "cnv1" in e.profile_entries()


F16X3_OPTIONS = [
    # (id, B, H, W, options in order, check of last_plan / profile)
    ("force_tile4", 5, 128, 416, {"split_k": 0, "force_tile": 4}, lambda e: _tiles(4)(e) == [4] and _tiles(5)(e) == [4]),
    ("force_tile5", 5, 128, 416, {"split_k": 0, "force_tile": 5}, lambda e: _tiles(4)(e) == [5] and _tiles(5)(e) == [5]),
    ("force_tile6", 5, 128, 416, {"split_k": 0, "force_tile": 6}, lambda e: _tiles(4)(e) == [6] and _tiles(5)(e) == [6]),
    ("force_tile8", 2, 128, 416, {"split_k": 0, "tile_208x128": 1, "force_tile": 8}, _plan_is(3, [8])),
    ("wave128_0", 32, 128, 416, {"wave128": 0}, lambda e: _tiles(4)(e) == [7] and _tiles(5)(e) == [7]),
    ("wave128_1", 32, 128, 416, {"wave128": 1}, lambda e: len(e.last_plan(4)) == 2 and _tiles(4)(e)[0] == 5),
    ("wave128_2", 32, 128, 416, {"wave128": 2}, lambda e: len(e.last_plan(4)) == 2 and _tiles(4)(e)[0] == 5),
    ("wave128_3", 32, 128, 416, {"wave128": 3}, _plan_is(3, [2])),
    ("merge_rem0", 32, 128, 416, {"wave128": 0, "merge_rem": 0}, lambda e: _tiles(4)(e) == [5, 4] and _tiles(5)(e) == [5, 4]),
    ("merge_cnv4", 32, 128, 416, {"wave128": 0, "merge_cnv4": 1}, _plan_is(3, [7])),
    ("merge_order0", 32, 128, 416, {"wave128": 0, "merge_order": 0}, _plan_is(4, [7])),
    ("merge_order1", 32, 128, 416, {"wave128": 0, "merge_order": 1}, _plan_is(4, [7])),
    ("merge_order2", 32, 128, 416, {"wave128": 0, "merge_order": 2}, _plan_is(4, [7])),
    ("split_k0", 1, 128, 416, {"split_k": 0}, None),
    ("split_k1", 1, 128, 416, {"split_k": 1}, None),
    ("split_k1_256x832", 1, 256, 832, {"split_k": 1}, None),
    ("fold_fixup", 1, 128, 416, {"split_k": 1, "fold_fixup": 1}, None),
    ("deep_ring0", 2, 128, 416, {"deep_ring": 0}, None),
    ("deep_ring1", 4, 128, 416, {"deep_ring": 1}, None),
    ("share_taps0", 5, 128, 416, {"share_taps": 0}, None),
    ("patch_cnv2_0", 2, 128, 416, {"patch_cnv2": 0}, lambda e: _tiles(1)(e)[0] < 90 and _tiles(2)(e) == [97]),
    ("patch_cnv3_0", 2, 128, 416, {"patch_cnv3": 0}, lambda e: _tiles(1)(e) == [98] and _tiles(2)(e)[0] < 90),
    ("patch_cnv23_0", 2, 36, 100, {"patch_cnv2": 0, "patch_cnv3": 0}, lambda e: _tiles(1)(e)[0] < 90 and _tiles(2)(e)[0] < 90),
    ("fuse_pack1", 3, 128, 416, {"fuse_pack": 1}, _profiled_without_mask_pack),
    ("fuse_pack1_ragged", 2, 36, 100, {"fuse_pack": 1}, _profiled_without_mask_pack),
    ("skip_order0", 32, 128, 416, {"skip_order": 0}, None),
    ("skip_order2", 32, 128, 416, {"skip_order": 2, "wave128": 0}, _plan_is(4, [7])),
]

F32_OPTIONS = [
    ("merge_rem_f32_0", 32, 128, 416, {"merge_rem_f32": 0}, lambda e: len(e.last_plan(4)) == 2 and len(e.last_plan(5)) == 2),
    ("merge_rem_f32_1", 32, 128, 416, {"merge_rem_f32": 1}, lambda e: e.last_plan(4) == [(64 * 32 * 104 // 128, 128)] and len(e.last_plan(5)) == 1),
    ("merge_rem_f32_2", 32, 128, 416, {"merge_rem_f32": 2}, lambda e: len(e.last_plan(4)) == 1 and len(e.last_plan(5)) == 1),
    ("f32_n16_0", 2, 128, 416, {"patch_f32": 0, "f32_n16": 0}, lambda e: _tiles(0)(e)[0] != 16),
    ("f32_n16_1", 2, 128, 416, {"patch_f32": 0, "f32_n16": 1}, _plan_is(0, [16])),
    ("f32_n16_1_ragged", 2, 36, 100, {"patch_f32": 0, "f32_n16": 1}, _plan_is(0, [16])),
    ("f32_n256", 32, 128, 416, {"f32_n256": 1}, lambda e: _tiles(4)(e)[0] == 256),
    ("patch_f32_0", 2, 128, 416, {"patch_f32": 0}, lambda e: 99 not in _tiles(0)(e) and _tiles(1)(e)[0] != 98 and _tiles(2)(e)[0] != 97),
    ("patch_f32_1", 2, 128, 416, {"patch_f32": 1}, lambda e: _tiles(0)(e) == [99] and _tiles(1)(e) == [98] and _tiles(2)(e) == [97]),
    ("patch_f32_1_ragged", 3, 20, 48, {"patch_f32": 1}, lambda e: _tiles(0)(e) == [99] and _tiles(1)(e) == [98] and _tiles(2)(e) == [97]),
    ("skip_order0", 32, 128, 416, {"skip_order": 0}, None),
    ("skip_order1", 32, 128, 416, {"skip_order": 1}, None),
    ("skip_order2", 32, 128, 416, {"skip_order": 2}, None),
]

OPTION_CASES = [pytest.param("f16x3", *c, id="f16x3-" + c[0]) for c in F16X3_OPTIONS] + \
               [pytest.param("f32", *c, id="f32-" + c[0]) for c in F32_OPTIONS]


@pytest.mark.parametrize("fuse_pose", [0, 1])
@pytest.mark.parametrize("precision,name,B,H,W,options,plan_check", OPTION_CASES)
def test_launch_option(precision, name, B, H, W, options, plan_check, fuse_pose):
    """One launch option forced, checked layer by layer; with fuse_pose 0 cnv7 and the separate pose head, with 1 the
    fused head.  Batches above 8 on the pair images the plan's launches start and end in."""
    cfg = parse_version(FLAGSHIP_VERSION)
    inputs = synth.make_inputs(B, H, W, first_window=3)
    e = _engine(cfg, H, W, B, precision)
    e.set_option("fuse_pose", fuse_pose)
    for k, v in options.items():
        e.set_option(k, v)
    if "fuse_pack" in options:
        e.profile(1)
    stats = _run(e, cfg, inputs, precision, "%s %s fuse_pose %d" % (precision, name, fuse_pose),
                 images="plan" if B > 8 else None, plan_check=plan_check)
    assert ("cnv7" in stats) != _fuses(H, W, fuse_pose), stats
    e.close()


def test_options_read_back_as_stored():
    """A context only, no forward: every launch option reads back as the table's default on a new engine and, after set_option, as
    what davo_option_store says the value is stored as; a refused value leaves the stored one alone."""
    from davo_amd import _lib
    table = _lib.option_table()
    # one value per row that is not its default; the ranges' from outside, so that the stored value differs from the one set
    values = dict(wave128=7, skip_order=-3, merge_order=5, pad_classes=9, merge_rem_f32=4, fold_tails=3, fuse_pack=5)
    e = Engine(parse_version(FLAGSHIP_VERSION), 36, 100, 1)
    try:
        assert [(k, e.get_option(k)) for k, _ in table] == table
        for k, default in table:
            v = values.get(k, 2 if default == 0 else 0)                       # the switches: on as 2, off as 0
            stored = _lib.option_store(k, v)
            assert stored is not None and stored != default, (k, v, stored)
            e.set_option(k, v)
            assert e.get_option(k) == stored, (k, v)
        with pytest.raises(ValueError, match=r"pad_classes must be 0, 1 or 8 \+ a layer mask \(8\.\.15\), got 2"):
            e.set_option("pad_classes", 2)
        assert e.get_option("pad_classes") == 1
        assert (e.get_option("auto_range"), e.get_option("stable_inputs"), e.get_option("cu_partition"), e.get_option("profile_stride"),
                e.get_option("host_chunk")) == (1, 0, 0, 1, 8)
        for key in ("force_tile", "no_such_option"):
            with pytest.raises(ValueError, match=key):
                e.get_option(key)
    finally:
        e.close()


# ---- float32 siblings to the bit ---------------------------------------------------------------------------------------
def test_f32_merged_and_unmerged_grids_are_bit_identical():
    """merge_rem_f32 0 (main + remainder launches), 1 (cnv4..cnv6 as one grid, the default) and 2 (cnv7 too), and f32_n256
    (cnv5 on the 128 x 256 tile): the same tiles' float32 chains, so the same bits in every stored layer and pose."""
    cfg = parse_version(FLAGSHIP_VERSION)
    B, H, W = 32, 128, 416
    inputs = synth.make_inputs(B, H, W, first_window=5)
    e = _engine(cfg, H, W, B, "f32")
    e.set_option("fuse_pose", 0)
    sh = LC.shapes(cfg, H, W)
    names = ("cnv4", "cnv5", "cnv6", "cnv7")
    e.set_option("merge_rem_f32", 0)
    base = LC.forward(e, *inputs).copy()
    assert all(len(e.last_plan(li)) == 2 for li in (4, 5, 6)), [e.last_plan(li) for li in range(7)]
    acts = {k: e.debug_read(k, (2 * B,) + sh[k]).copy() for k in names}
    for key, val, merged in (("merge_rem_f32", 1, (4, 5)), ("merge_rem_f32", 2, (4, 5, 6)), ("f32_n256", 1, ())):
        e.set_option(key, val)
        got = LC.forward(e, *inputs)
        for li in merged:
            assert len(e.last_plan(li)) == 1, (key, val, li, e.last_plan(li))
        if key == "f32_n256":
            assert e.last_plan(4)[0][1] == 256, e.last_plan(4)
        for k in names:
            assert np.array_equal(e.debug_read(k, (2 * B,) + sh[k]), acts[k]), (key, val, k)
        assert np.array_equal(got, base), (key, val)
    e.close()


# ---- attention sources ---------------------------------------------------------------------------------------------------
BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
FLAGSHIP_FAMILY = [FLAGSHIP_VERSION, BASE + "-static", "v1-sharedNN-dilatedPoseNN-cnv6_64-no_segmask"]
CLASS_TABLE = [BASE + s for s in ("-se_seg_wo_tgt-fc_tanh", "-se_rgb_wo_tgt_to_seg-fc_tanh", "-se_rgb_to_seg-fc_tanh",
                                  "-se_SegFlow_to_seg_wo_tgt-fc_tanh", "-se_SegFlow_to_seg-norm_flow-fc_tanh",
                                  "-se_SegFlow_to_seg_8_wo_tgt-fc_tanh", "-se_SegFlow_to_seg_8-abs_flow-fc_tanh")]
SQ_CHUNKS = 32                  # csrc/params.h: the class-table squeeze's chunks per frame
RARE = 18                       # the class the boundary labels use; removed everywhere else


def _boundary_labels(B, H, W):
    """Inputs whose labels put a class found nowhere else on the first and last 4-pixel unit of every chunk of
    se_class_squeeze (units [c * per, min((c + 1) * per, HW / 4)), per = ceil(HW / 4 / SQ_CHUNKS)) and on the frame's
    last unit, in every frame: a chunk range off by one unit moves that class's bin by 4 pixels per chunk."""
    img, flow, seg = synth.make_inputs(B, H, W, first_window=2)
    seg[seg == RARE] = RARE - 1
    units = H * W // 4
    per = -(-units // SQ_CHUNKS)
    marks = {units - 1}
    for c in range(SQ_CHUNKS):
        beg, end = c * per, min((c + 1) * per, units)
        if beg < end:
            marks.update((beg, end - 1))
    for u in sorted(marks):
        y, x = divmod(4 * u, W)
        seg[:, :, y, x:x + 4, 0] = RARE
    return img, flow, seg


@pytest.mark.parametrize("H,W,B", [(64, 96, 2), (128, 416, 4)])
@pytest.mark.parametrize("version", FLAGSHIP_FAMILY)
def test_flagship_family_inputs(version, H, W, B):
    """se_flow, static and no_segmask: att_table, packed and cnv1."""
    cfg = parse_version(version)
    inputs = _boundary_labels(B, H, W)
    for precision in PRECISIONS:
        e = _engine(cfg, H, W, B, precision)
        _run(e, cfg, inputs, precision, "%s %dx%d B=%d %s" % (version, H, W, B, precision), stop_after="cnv1")
        e.close()


@pytest.mark.parametrize("H,W,B", [(64, 96, 2), (128, 416, 4), (256, 832, 1)])
@pytest.mark.parametrize("version", CLASS_TABLE)
def test_class_table_sources_on_squeeze_chunk_boundaries(version, H, W, B):
    """The seven class-table sources, excitation folded into the squeeze launch and as a launch of its own: att_table,
    packed and cnv1.  At 128x416 and 256x832 a chunk is more than one pass of the squeeze loop."""
    cfg = parse_version(version)
    img, flow, seg = inputs = _boundary_labels(B, H, W)
    assert (seg == RARE).any()
    for precision in PRECISIONS:
        e = _engine(cfg, H, W, B, precision)
        for fold in (0, 1):
            e.set_option("fold_tails", fold)
            _run(e, cfg, inputs, precision, "%s %dx%d B=%d %s fold_tails %d" % (version, H, W, B, precision, fold),
                 stop_after="cnv1")
        e.close()
