"""The depth-source class tables (att_source 11, 12: -se_depth_wo_tgt_to_seg, -se_depth_to_seg) on the CPU: version
parsing, the float64 restatement the GPU tests check against (tests/depth_source_ref.py), the loaders' fourth plane set,
TF bundles with the se_depth scope, and the four `_depth' entry points of the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

from davo_amd import synth, _lib
from davo_amd import loader as L
from davo_amd import sequence as S
from davo_amd.version import parse_version, weight_shapes, UnsupportedVariantError, NUM_SEG_CLASSES

import depth_source_ref as D
from layer_check import TABLE_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
PUBLISHED = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all-se_depth_wo_tgt_to_seg-fc_tanh"    # doc/arch-variants.md
# substring -> (att_source, C value, tgt_attended)
SOURCES = {"-se_depth_wo_tgt_to_seg": ("se_depth_wo_tgt_to_seg", 11, False),
           "-se_depth_to_seg": ("se_depth_to_seg", 12, True)}
DEPTH_ENTRY_POINTS = ("davo_forward_depth", "davo_forward_device_depth", "davo_submit_depth", "davo_calibrate_depth")


def _check(cfg, sub, act):
    name, value, tgt = SOURCES[sub]
    assert cfg.att_source == name and cfg.tgt_attended is tgt and cfg.se_scope == "se_depth" and cfg.needs_depth is True
    assert cfg.as_c_ints() == (5, 128, {"relu": 0, "tanh": 1}[act], 0, 0, value, 1, 1)
    sh = weight_shapes(cfg)
    p = "pose_exp_net/se_depth/"
    se = {k: v for k, v in sh.items() if "/se_" in k}
    assert se == {p + "bottleneck_fc/kernel": (1, 8), p + "bottleneck_fc/bias": (8,),
                  p + "recover_fc/kernel": (8, NUM_SEG_CLASSES), p + "recover_fc/bias": (NUM_SEG_CLASSES,)}
    assert not any("seg_channel_weight" in k for k in sh)
    assert len(sh) == 22 + 4


# ---- parser ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sub", sorted(SOURCES))
def test_each_substring_alone(sub):
    _check(parse_version(BASE + sub), sub, "relu")
    _check(parse_version(BASE + sub + "-fc_tanh"), sub, "tanh")


def test_published_string():
    _check(parse_version(PUBLISHED), "-se_depth_wo_tgt_to_seg", "tanh")


def test_elif_order():
    """-se_depth_wo_tgt_to_seg contains neither other substring's branch first: it is 11, not 12; `-se_flow' anywhere in
    the string wins (davo.py:1175 comes first) and such a version never uses the depth it reads."""
    assert parse_version(BASE + "-se_depth_wo_tgt_to_seg").as_c_ints()[5] == 11
    assert parse_version(BASE + "-se_depth_to_seg").as_c_ints()[5] == 12
    for sub in SOURCES:
        c = parse_version(BASE + sub + "-se_flow-abs_flow-fc_tanh")
        assert c.att_source == "se_flow" and c.needs_depth is False and c.se_scope == "se_flow"
    assert parse_version(BASE + "-se_flow-abs_flow-fc_tanh").needs_depth is False
    assert parse_version(BASE).needs_depth is False
    for sub in SOURCES:                                               # -norm_flow / -abs_flow do not touch the depth input
        c = parse_version(BASE + sub + "-norm_flow-abs_flow_h")
        assert c.needs_depth and c.norm_flow and c.abs_mode == "h"


@pytest.mark.parametrize("sub", ["-se_depth", "-se_depth_wo_tgt", "-se_disp_to_seg", "-se_disp_wo_tgt_to_seg", "-se_mixDepthFlow",
                                 "-se_depth_to_seg-norm_depth", "-se_flow_on_depthseg_sharedlayers"])
def test_other_depth_branches_still_rejected(sub):
    with pytest.raises(UnsupportedVariantError):
        parse_version(BASE + sub + "-fc_tanh")


def test_rejections_say_why():
    with pytest.raises(UnsupportedVariantError, match="1110"):
        parse_version(BASE + "-se_depth_to_seg-norm_depth")
    with pytest.raises(UnsupportedVariantError, match="label maps"):
        parse_version(BASE + "-se_disp_to_seg")


# ---- the float64 restatement against hand-built answers ------------------------------------------------------------------
def _constant_depth(B, H, W):
    depth = np.empty((B, 3, H, W, 1), np.float32)
    depth[:, 0], depth[:, 1], depth[:, 2] = 3.0, 5.0, 11.0              # file order src0, tgt, src1
    return depth


def test_descriptor_known_answer():
    """davo.py:1109: the SE input of frame i is depth_i + depth_tgt; frames (tgt, src0, src1)."""
    for sub in SOURCES:
        d = D.descriptors(parse_version(BASE + sub), _constant_depth(2, 8, 12))
        assert d.shape == (2, 3, 1)
        assert np.array_equal(d[:, :, 0], np.tile([10.0, 8.0, 16.0], (2, 1)))


def equivalent_weights(cfg, static_weights):
    w = {k: v for k, v in static_weights.items() if "seg_channel_weight" not in k}
    p = "pose_exp_net/se_depth/"
    for name, shape in weight_shapes(cfg).items():
        if name.startswith(p):
            w[name] = np.zeros(shape, np.float32)
    w[p + "recover_fc/bias"] = static_weights["pose_exp_net/pose_exp_net/seg_channel_weight/weight"].copy()
    return w


def test_zero_kernels_give_the_static_packing():
    """Zero kernels and recover_fc/bias = the static weight vector: -se_depth_wo_tgt_to_seg packs like -static and
    -se_depth_to_seg like static_all (-segmask_all), whatever the depth."""
    from oracle import davo_oracle as O
    img, flow, seg = synth.make_inputs(1, 16, 24)
    depth = synth.make_depth(1, 16, 24)
    for sub, static in (("-se_depth_wo_tgt_to_seg", BASE + "-static"), ("-se_depth_to_seg", BASE)):
        cfg, scfg = parse_version(BASE + sub), parse_version(static)
        ws = synth.make_weights(scfg)
        w = equivalent_weights(cfg, ws)
        assert np.allclose(D.pack(cfg, img, flow, seg, depth, w), O.pack_inputs(scfg, img, flow, seg, ws), rtol=0, atol=1e-12)


def test_left_right_flip_leaves_the_tables():
    """The test loader flips depth left-right like the other planes (data_loader.py:296); a global mean does not see it."""
    depth = synth.make_depth(2, 36, 100)
    for sub in SOURCES:
        cfg = parse_version(BASE + sub + "-fc_tanh")
        w = D.sensitive_weights(cfg, synth.make_weights(cfg), depth)
        a, b = D.class_tables(cfg, depth, w), D.class_tables(cfg, depth[:, :, :, ::-1], w)
        assert np.abs(a - b).max() <= 1e-15


def test_wo_tgt_target_row_is_ones_and_sources_agree():
    depth = synth.make_depth(2, 16, 24)
    ca, cb = parse_version(BASE + "-se_depth_wo_tgt_to_seg-fc_tanh"), parse_version(BASE + "-se_depth_to_seg-fc_tanh")
    w = D.sensitive_weights(ca, synth.make_weights(ca), depth)
    ta, tb = D.class_tables(ca, depth, w), D.class_tables(cb, depth, w)
    assert np.array_equal(ta[:, 0], np.ones((2, 19))) and np.array_equal(ta[:, 1:], tb[:, 1:])
    assert np.all((tb > 0) & (tb < 1))


@pytest.mark.parametrize("act", ["", "-fc_tanh"])
@pytest.mark.parametrize("sub", sorted(SOURCES))
def test_scaled_weights_make_depth_matter(sub, act):
    """The condition the GPU tests rest on: with the bottleneck kernel scaled by the batch's mean descriptor, two different
    depth fields give tables more than 100 x TABLE_TOL apart; with synth.make_weights' own kernel every tanh unit saturates."""
    cfg = parse_version(BASE + sub + act)
    depth = synth.make_depth(2, 36, 100)
    w = D.sensitive_weights(cfg, synth.make_weights(cfg), depth)
    rows = slice(None) if cfg.tgt_attended else slice(1, None)
    diff = np.abs(D.class_tables(cfg, depth, w) - D.class_tables(cfg, D.other_depth(depth), w))[:, rows].max()
    assert diff > 100 * TABLE_TOL, diff


def test_synthetic_depth_is_reproducible_and_in_range():
    d = synth.make_depth(3, 36, 100, first_window=4)
    assert d.shape == (3, 3, 36, 100, 1) and d.dtype == np.float32
    assert d.min() > 1.0 and d.max() < 80.0
    assert np.array_equal(d[2], synth.make_depth(1, 36, 100, first_window=6)[0])         # a window is reproducible on its own
    assert not np.array_equal(d[0], d[1]) and not np.array_equal(d[0, 0], d[0, 1])
    a, b = synth.make_inputs(1, 16, 24), synth.make_inputs(1, 16, 24)                     # the other planes keep their three
    assert len(a) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.abs(np.diff(d[0, 0, :, :, 0], axis=1)).max() < 0.2 * d.max()                # smooth: no pixel-to-pixel jumps


# ---- loaders -----------------------------------------------------------------------------------------------------------
H, W, NF = 32, 48, 9


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("depth_dump"))
    assert L.write_synthetic_dump(d, 3, NF, H, W, depth=True) == NF - 2
    return d


def test_dump_layout(dump, tmp_path):
    names = sorted(os.listdir(os.path.join(dump, "03")))
    assert "000001-monodepth2_depth.npy" in names and len(names) == 4 * (NF - 2)
    a = np.load(os.path.join(dump, "03", "000004-monodepth2_depth.npy"))
    assert a.dtype == np.float32 and a.shape == (3, H, W, 1)
    assert np.array_equal(a, synth.make_depth(1, H, W, first_window=3)[0])                # file order src0, tgt, src1
    L.write_synthetic_dump(str(tmp_path), 3, 4, H, W)                                     # off by default
    assert not any("depth" in f for f in os.listdir(os.path.join(str(tmp_path), "03")))


def test_inline_and_threaded_loaders_carry_depth(dump):
    want = synth.make_depth(NF - 2, H, W)
    _, wflow, wseg = synth.make_inputs(NF - 2, H, W)
    ld = S.kitti_window_loader(dump, 3, NF, H, W, depth=True)
    inline = ld(0, NF - 2)
    assert len(inline) == 4 and np.array_equal(inline[3], want) and np.array_equal(inline[1], wflow) and np.array_equal(inline[2], wseg)
    seen = 0
    for s, e, batch in ld.for_range(0, NF - 2, 3):
        assert len(batch) == 4
        for k in range(4):
            assert np.array_equal(batch[k], inline[k][s:e]), (s, k)
        seen += e - s
    assert seen == NF - 2


def test_process_loader_carries_depth(dump):
    """One more shared buffer per ring place: the depth planes, all three, in file order; a loader without depth keeps its three."""
    want = synth.make_depth(NF - 2, H, W)
    img, flow, seg = synth.make_inputs(NF - 2, H, W)
    ld = S.kitti_window_loader(dump, 3, NF, H, W, procs=2, depth=True).for_range(0, NF - 2, 3)
    assert isinstance(ld, L.ProcessWindowLoader) and ld.depth
    seen = 0
    for s, e, batch in ld:
        assert len(batch) == 4 and batch[3].shape == (e - s, 3, H, W, 1)
        assert np.array_equal(batch[3], want[s:e]), s
        assert np.array_equal(batch[1][:, :2], flow[s:e, :2]) and np.array_equal(batch[2][:, (0, 2)], seg[s:e][:, (0, 2)])
        seen += e - s
    ld.close()
    assert seen == NF - 2
    plain = S.kitti_window_loader(dump, 3, NF, H, W, procs=2).for_range(0, NF - 2, 3)
    assert all(len(b) == 3 for _, _, b in plain)
    plain.close()


def test_process_loader_propagates_a_missing_depth_file(dump, tmp_path):
    import shutil
    d = str(tmp_path / "copy")
    shutil.copytree(dump, d)
    os.remove(L.depth_path(d, 3, 2))
    ld = L.ProcessWindowLoader(d, 3, H, W, 0, NF - 2, 3, procs=2, depth=True)
    with pytest.raises(Exception):
        list(ld)
    ld.close()
    ok = L.ProcessWindowLoader(d, 3, H, W, 0, NF - 2, 3, procs=2)             # ... and is not missed without depth
    assert sum(e - s for s, e, _ in ok) == NF - 2
    ok.close()


def test_a_variant_without_depth_never_opens_a_depth_file(dump, tmp_path):
    import shutil
    d = str(tmp_path / "copy")
    shutil.copytree(dump, d)
    ld = S.kitti_window_loader(d, 3, NF, H, W)
    assert all(len(b) == 3 for _, _, b in ld.for_range(0, NF - 2, 3)) and len(ld(0, 2)) == 3
    os.remove(L.depth_path(d, 3, 5))                                  # window 4's depth file
    got = [b for _, _, b in ld.for_range(0, NF - 2, 7)]               # ... is not missed by a variant that reads no depth
    assert len(got) == 1 and len(got[0]) == 3 and got[0][0].shape[0] == NF - 2
    assert len(ld(3, 6)) == 3
    dl = S.kitti_window_loader(d, 3, NF, H, W, depth=True)
    with pytest.raises(FileNotFoundError):                            # ... and propagates from the loaders that do
        dl(3, 6)
    with pytest.raises(FileNotFoundError):
        list(dl.for_range(0, NF - 2, 3))
    assert len(list(dl.for_range(0, 3, 3))) == 1                      # the windows before it still load


def test_run_shard_hands_depth_to_the_driver_and_the_stream(dump):
    """run_shard: a four-array batch reaches infer_fn as four arguments and a stream as depth=; the ragged last batch is
    padded in all four; three-array batches make the calls they always made."""
    ld = S.kitti_window_loader(dump, 3, NF, H, W, depth=True)
    want = synth.make_depth(NF - 2, H, W)
    calls = []

    def infer(img, flow, seg, depth):
        calls.append(depth.copy())
        assert img.shape[0] == flow.shape[0] == seg.shape[0] == depth.shape[0] == 3
        return np.zeros((3, 2, 6), np.float32)
    S.run_shard(infer, ld.for_range(0, NF - 2, 3), 0, NF - 2, 3)
    assert np.array_equal(np.concatenate(calls)[:NF - 2], want) and np.array_equal(calls[-1][1], calls[-1][0])

    class Stream:
        def __init__(self):
            self.depths, self.plain = [], 0

        def submit(self, img, flow, seg, out, **kw):
            if kw:
                assert list(kw) == ["depth"]
                self.depths.append(kw["depth"].copy())
            else:
                self.plain += 1
            out[...] = 0

        def drain(self):
            pass
    st = Stream()
    S.run_shard(None, ld, 0, NF - 2, 3, None, st)
    assert np.array_equal(np.concatenate(st.depths)[:NF - 2], want) and st.plain == 0
    st = Stream()
    S.run_shard(None, S.kitti_window_loader(dump, 3, NF, H, W), 0, NF - 2, 3, None, st)
    assert st.plain == 3 and not st.depths
    syn = S.synthetic_window_loader(H, W, depth=True)(2, 5)
    assert len(syn) == 4 and np.array_equal(syn[3], want[2:5]) and len(S.synthetic_window_loader(H, W)(2, 5)) == 3


# ---- plumbing ----------------------------------------------------------------------------------------------------------
def test_cli_loader_label_planes():
    from davo_amd.run_kitti_pose import loader_seg_planes
    assert loader_seg_planes(parse_version(BASE + "-se_depth_wo_tgt_to_seg")) is None
    assert loader_seg_planes(parse_version(BASE + "-se_depth_to_seg")) == (0, 1, 2)


@pytest.mark.parametrize("sub", sorted(SOURCES))
def test_tf_bundle_round_trips_the_se_depth_scope(tmp_path, sub):
    from davo_amd import tf_checkpoint as T
    cfg = parse_version(BASE + sub + "-fc_tanh")
    w = synth.make_weights(cfg)
    T.write_checkpoint(str(tmp_path / "model-1"), w, num_shards=2)
    got = T.load_weights(str(tmp_path))
    assert set(got) == set(w)
    for k in w:
        assert got[k].dtype == np.float32 and np.array_equal(got[k], w[k]), k
    listed = {name: shape for name, shape, _ in T.list_variables(str(tmp_path / "model-1"))}
    for k in w:
        if "/se_depth/" in k:
            assert listed[k] == w[k].shape, k
    assert sum("/se_depth/" in k for k in w) == 4


def test_abi_header_binding_and_library_agree_on_the_depth_entry_points():
    src = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(davo_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_lib.build())
    for name in DEPTH_ENTRY_POINTS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
        # the depth pointer sits behind `seg': one more pointer argument than the three-input form
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, src)
        m0 = re.search(r"\b%s\s*\(([^)]*)\)" % name[:-len("_depth")], src)
        assert m.group(1).count(",") == m0.group(1).count(",") + 1 and "depth" in m.group(1)
    bound = _lib.lib()
    for name in DEPTH_ENTRY_POINTS:
        assert len(getattr(bound, name).argtypes) == len(getattr(bound, name[:-len("_depth")]).argtypes) + 1
    assert ctypes.sizeof(_lib.DavoVariant) == 32


def test_engine_surface_takes_depth_by_keyword():
    import inspect
    from davo_amd import Engine, DAVO
    for fn in (Engine.forward, Engine.submit, Engine.calibrate, Engine.forward_device):
        p = inspect.signature(fn).parameters["depth"]
        assert p.default is None
    assert "input_depth" in inspect.signature(DAVO.setup_inference).parameters
