"""The coupled shared PoseNN (`-sharedNN-dilatedCouplePoseNN'; davo_set_posenn_heads) on the GPU against the float64 restatement
of tests/coupled_ref.py.

Layer by layer with tests/layer_check.py's functions and bars, each launch judged on the GPU's own input to it
(Engine.debug_read): att_table and packed as on the flagship; cnv1..cnv5 under their existing bars; cnv6 as ONE group of cnv6_out
columns from all of cnv5; cnv7 as ONE group of 256 columns from ALL cnv6_out channels; the six-column pose head from the GPU's
cnv7 at POSE_REL (fused into cnv7's epilogue - f16x3, maps of at least 128 pixels - from the GPU's cnv6 through a float64 cnv7); the
poses end to end at tests/helpers.py's parity bar.  Then every (cnv6, cnv7) launch plan of
tests/coupled_cases.py in both precisions, the sibling launches to the bit, the entry points to the bit against davo_forward,
range recovery, the error codes and the drivers.  The conditions on the inputs are asserted on the restatement alone in
tests/test_coupled.py."""
import ctypes
import os

import numpy as np
import pytest

import davo_amd
from davo_amd import DavoRangeError, Engine, synth, parse_version, FLAGSHIP_VERSION, labels_to_u8, flow_to_f16, depth_to_f16
from davo_amd import loader as L
from davo_amd import sequence as S

import coupled_cases as K
import coupled_ref as C
import layer_check as LC
from helpers import assert_pose_close, hip_free_bytes
from test_stream import _rescaled

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "f32"]
INVALID = -1                             # DAVO_ERR_INVALID
ROW = {"src0": 0, "src1": 1}


def _engine(cfg, H, W, max_batch, weights, precision, **kw):
    e = Engine(cfg, H, W, max_batch, **kw)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


def _tiles(e, li):
    return tuple(t for _, t in e.last_plan(li))


@pytest.fixture(scope="module", autouse=True)
def flagship_before():
    """One flagship forward in each precision before any coupled engine exists in this process (the module's first act)."""
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, B = K.SMALL
    inp = K.inputs(H, W, B)
    out = {}
    for precision in PRECISIONS:
        e = _engine(cfg, H, W, B, synth.make_weights(cfg), precision)
        out[precision] = (e.forward(*inp), [e.last_plan(li) for li in range(7)])
        e.close()
    return out


def _plan_images(e, cfg, B, H, W):
    """tests/layer_check.py's plan_images for cnv6 and cnv7 of a coupled engine: the first and last pair image, and those holding the
    first and last row of every launch of the last forward."""
    NB = 2 * B
    sh = C.shapes(cfg, H, W)
    keep = {0, NB - 1}
    for li, name in ((5, "cnv6"), (6, "cnv7")):
        per = sh[name][0] * sh[name][1]
        row = 0
        for m, _ in e.last_plan(li):
            for r in (row, min(row + 128 * m, NB * per) - 1):
                keep.add(min(r // per, NB - 1))
            row = min(row + 128 * m, NB * per)
    return sorted(keep)


def _fuses(H, W, precision, fuse_pose=1):
    """The six-column pose head runs in cnv7's epilogue in f16x3 where asked ("fuse_pose", the default) and cnv7's map holds at least
    one 128-row tile per image (forward.hip); float32 and the small maps store cnv7 and run the two-pass head."""
    h7, w7, _ = C.shapes(None, H, W)["cnv7"]
    return bool(fuse_pose) and precision == "f16x3" and h7 * w7 >= 128


def _layer_by_layer(e, cfg, w, inp, poses, precision, what, images=None, start="packed", depth=None, fused=False):
    """The last forward of a coupled engine against float64, each layer from the GPU's own input.  start = "cnv5": cnv6, cnv7 and the
    pose head only (the launches in front of them are the flagship's).  images: pair images to check (None = all).  fused: the pose
    head ran in cnv7's epilogue - cnv7 must be refused, and the poses are judged from the GPU's cnv6."""
    img, flow, seg = inp[:3]
    B, H, W = img.shape[0], img.shape[1], img.shape[2] // 3
    NB = 2 * B
    sh = C.shapes(cfg, H, W)
    images = np.arange(NB) if images is None else np.asarray(images)
    shifts = e.activation_range()[1] if precision == "f16x3" else {}
    floor = lambda name: LC.STORE_FLOOR * 2.0 ** -shifts.get(name, 0) if precision == "f16x3" else 0.0      # noqa: E731
    lay = C.layers(cfg, w)
    stats = {}
    if start == "packed":
        want_tab, rows = LC.ref_tables(cfg, img, flow, seg, w)
        LC.check_table(e.debug_read("att_table", (B, 3, 19)), want_tab, rows, what)
        packed = e.debug_read("packed", (NB,) + sh["packed"])
        want_p = C.pack(cfg, img, flow, seg, w, depth).reshape(NB, H, W, 10)[..., C.PACK8]
        stats["packed"] = LC.check_packed(packed, want_p, what)
        acts = {"packed": packed[images]}
    else:
        acts = {start: e.debug_read(start, (NB,) + sh[start])[images]}
        lay = lay[[l[0] for l in lay].index(start) + 1:]
    for name, prev, stride, rate, groups in lay:
        assert len(groups) == 1                                  # one group: cnv7 reads every channel of cnv6
        if name == "cnv7" and fused:
            with pytest.raises(Exception, match="not materialised"):
                e.debug_read("cnv7", (NB,) + sh["cnv7"])
            break                                                # the pose head ran in cnv7's epilogue: judged from the GPU's cnv6 below
        acts[name] = e.debug_read(name, (NB,) + sh[name])[images]
        worst = (0.0, 0.0)
        for c0 in range(0, len(images), 8):
            s = slice(c0, c0 + 8)
            a, b = LC.check_layer(name, acts[name][s], acts[prev][s], groups, stride, rate, LC.TAU[precision][name], what, floor(name))
            worst = (max(worst[0], a), max(worst[1], b))
        stats[name] = worst
        del acts[prev]
    got = np.asarray(poses, np.float64).reshape(NB, 6)[images]
    if fused:
        _, _, stride, rate, ((w7, b7, _, _),) = lay[-1]
        c7 = np.concatenate([LC.conv64(acts["cnv6"][c0:c0 + 8], w7, b7, stride, rate) for c0 in range(0, len(images), 8)])
        stats["pose(fused)"] = LC.check_pose(got, C.pose_from_cnv7(c7, w), what + " fused head")
    else:
        stats["pose"] = LC.check_pose(got, C.pose_from_cnv7(acts["cnv7"], w), what + " pose head")
    return stats


# ---- layer by layer at the four shapes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,B", K.SHAPES, ids=K.IDS)
def test_layer_by_layer(H, W, B, precision):
    cfg, inp, w = K.case(H, W, B)
    what = "%dx%d B=%d %s" % (H, W, B, precision)
    e = _engine(cfg, H, W, B, w, precision)
    e.set_option("fuse_pose", 0)
    poses = LC.forward(e, *inp)
    stats = _layer_by_layer(e, cfg, w, inp, poses, precision, what)
    assert set(np.unique(inp[2][0]).astype(int)) >= set(range(19)) | {255}
    want = K.reference(H, W, B)
    err = assert_pose_close(poses, want, what)
    print("%s: pose max|err| %.3g of max|pose| %.3g; worst (a, b) %s" % (what, err, np.abs(want).max(), {k: v for k, v in stats.items() if k.startswith("cnv")}))
    sh = C.shapes(cfg, H, W)
    assert e.debug_read("cnv7", (2 * B,) + sh["cnv7"]).shape[-1] == 256 and e.debug_read("cnv6", (2 * B,) + sh["cnv6"]).shape[-1] == cfg.cnv6_out
    with pytest.raises(ValueError, match="holds"):               # the decoupled sizes are not the coupled tensors'
        e.debug_read("cnv7", (2 * B,) + sh["cnv7"][:2] + (512,))
    e.set_option("fuse_pose", 1)                                 # the default
    fused = _fuses(H, W, precision)
    got = LC.forward(e, *inp)
    if not fused:                                                # float32, and maps under 128 pixels: the two-pass head, cnv7 stays stored
        assert np.array_equal(got, poses)
        e.debug_read("cnv7", (2 * B,) + sh["cnv7"])
        e.set_option("fold_tails", 1)                            # nothing to fold the pose tail into
        assert_pose_close(LC.forward(e, *inp), want, what + " fold_tails 1")
        e.debug_read("cnv7", (2 * B,) + sh["cnv7"])
    else:                                                        # the six-column epilogue: cnv7 never stored
        assert 6 not in _tiles(e, 6) and len(e.last_plan(6)) == 1, e.last_plan(6)
        _layer_by_layer(e, cfg, w, inp, got, precision, what + " fused", start="cnv5", fused=True)
        assert_pose_close(got, poses, what + " fused against the two-pass head")
        assert_pose_close(got, want, what + " fused")
        for _ in range(50):
            assert np.array_equal(e.forward(*inp), got)
        e.set_option("fold_tails", 1)                            # the launch's last workgroup writes the poses: pose_from_tiles' sums, to the bit
        assert np.array_equal(LC.forward(e, *inp), got)
        with pytest.raises(Exception, match="not materialised"):
            e.debug_read("cnv7", (2 * B,) + sh["cnv7"])
        for _ in range(50):
            assert np.array_equal(e.forward(*inp), got)
        e.set_option("fold_tails", -1)
        e.set_option("force_tile", 6)                            # the 208x256 tile has the three-column epilogue alone: the planner's tile instead
        assert_pose_close(LC.forward(e, *inp), got, what + " force_tile 6")      # (cnv5 takes that tile and leaves split-K: rounding)
        assert 6 not in _tiles(e, 6) and _tiles(e, 4) == (6,), [e.last_plan(li) for li in range(7)]
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("width", K.WIDTHS)
def test_all_four_widths(width, precision):
    H, W, B = K.SMALL
    ver = K.version(width)
    cfg, inp, w = K.case(H, W, B, ver)
    what = "cnv6_%d %s" % (width, precision)
    e = _engine(cfg, H, W, B, w, precision)
    poses = LC.forward(e, *inp)
    _layer_by_layer(e, cfg, w, inp, poses, precision, what)
    assert_pose_close(poses, K.reference(H, W, B, ver), what)
    e.close()


@pytest.mark.parametrize("version", K.VERSIONS[1:])
def test_the_other_versions(version):
    """Every attention source in front of the coupled head: the poses end to end in f16x3 (the depth source with its depth planes)."""
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B, version)
    depth = K.depth_planes(H, W, B) if cfg.needs_depth else None
    e = _engine(cfg, H, W, B, w, "f16x3")
    got = e.forward(*inp, depth=depth) if depth is not None else e.forward(*inp)
    assert_pose_close(got, K.reference(H, W, B, version), version)
    e.close()


# ---- the duplicated-head identity on the device -----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,B", [K.SMALL, (52, 172, 3)])
def test_duplicated_heads_on_the_device(H, W, B, precision):
    """A decoupled engine whose two heads hold the coupled cnv6 / cnv7 and the halves of pred computes the coupled poses in exact
    arithmetic: the two engines against each other at the parity bar, on kernels that share nothing behind cnv5 (the fused
    three-column epilogue at 52x172 against the two-pass six-column head)."""
    cfg, inp, w = K.case(H, W, B)
    dversion, dw = C.duplicated(cfg, w)
    e = _engine(cfg, H, W, B, w, precision)
    d = _engine(parse_version(dversion), H, W, B, dw, precision)
    got, twin = e.forward(*inp), d.forward(*inp)
    assert_pose_close(got, twin, "coupled against duplicated heads %s" % precision)
    assert_pose_close(twin, K.reference(H, W, B), "duplicated heads against float64")
    e.close()
    d.close()


# ---- every plan of the table ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width,B,t6,t7", [pytest.param(*c, id=K.plan_case_id(*c[:2])) for c in K.plan_cases()])
def test_plan_case_f16x3(width, B, t6, t7):
    """cnv6 and cnv7 run the tiles the table names (no merged grid: tile 7 is never reported; the 256x256 tile of cnv7 stays on
    conv_igemm_h3, conv_igemm_h3w has no stride-2 form), each checked from the GPU's own input, with the pose head."""
    H, W = K.PLAN_H, K.PLAN_W
    ver = K.version(width)
    cfg, w = parse_version(ver), K.weights(ver)
    inp = synth.make_inputs(B, H, W, first_window=7)
    e = _engine(cfg, H, W, B, w, "f16x3")
    e.set_option("fuse_pose", 0)                                 # the table's cnv7 is the stored one
    poses = LC.forward(e, *inp).copy()
    assert (_tiles(e, 5), _tiles(e, 6)) == (t6, t7), [e.last_plan(li) for li in range(7)]
    what = "%s f16x3" % K.plan_case_id(width, B)
    images = _plan_images(e, cfg, B, H, W)
    _layer_by_layer(e, cfg, w, inp, poses, "f16x3", what, images=images, start="cnv5")
    e.set_option("fuse_pose", 1)                                 # the default: one launch of one tile no taller than an image, never the 208x256 one
    got = LC.forward(e, *inp)
    assert _tiles(e, 5) == t6 and len(e.last_plan(6)) == 1 and 6 not in _tiles(e, 6), [e.last_plan(li) for li in range(7)]
    _layer_by_layer(e, cfg, w, inp, got, "f16x3", what + " fused", images=images, start="cnv6", fused=True)
    assert_pose_close(got, poses, what + " fused against the two-pass head")
    e.close()


def _f32_expected(t6, t7, merge):
    """last_plan's N tiles of (cnv6, cnv7): "merge_rem_f32" 1 makes one grid of cnv6's two launches where the main tile is 128 columns
    wide (reported as one launch of 128), 2 of cnv7's too."""
    m6 = (128,) if merge >= 1 and len(t6) == 2 and t6[0] == 128 else t6
    m7 = (128,) if merge >= 2 and len(t7) == 2 and t7[0] == 128 else t7
    return m6, m7


@pytest.mark.parametrize("width,B,t6,t7", [pytest.param(w, *c, id=K.plan_case_id(w, c[0])) for w in K.WIDTHS for c in K.F32_CASES[w]])
def test_plan_case_f32(width, B, t6, t7):
    """float32: the unmerged launches ("merge_rem_f32" 0) are the table's and are checked layer by layer; the merged grids of cnv6
    (1, the default) and of cnv7 as well (2) run the same tiles' float32 chains: the same bits."""
    H, W = K.PLAN_H, K.PLAN_W
    ver = K.version(width)
    cfg, w = parse_version(ver), K.weights(ver)
    inp = synth.make_inputs(B, H, W, first_window=5)
    sh = C.shapes(cfg, H, W)
    e = _engine(cfg, H, W, B, w, "f32")
    e.set_option("merge_rem_f32", 0)
    base = LC.forward(e, *inp).copy()
    assert (_tiles(e, 5), _tiles(e, 6)) == (t6, t7), [e.last_plan(li) for li in range(7)]
    what = "%s f32" % K.plan_case_id(width, B)
    _layer_by_layer(e, cfg, w, inp, base, "f32", what, images=_plan_images(e, cfg, B, H, W), start="cnv5")
    acts = {k: e.debug_read(k, (2 * B,) + sh[k]).copy() for k in ("cnv6", "cnv7")}
    for merge in (1, 2):
        if _f32_expected(t6, t7, merge) == _f32_expected(t6, t7, merge - 1):
            continue                                             # nothing more merges at this batch size
        e.set_option("merge_rem_f32", merge)
        got = LC.forward(e, *inp)
        assert (_tiles(e, 5), _tiles(e, 6)) == _f32_expected(t6, t7, merge), (merge, [e.last_plan(li) for li in range(7)])
        for k in acts:
            assert np.array_equal(e.debug_read(k, (2 * B,) + sh[k]), acts[k]), (merge, k)
        assert np.array_equal(got, base), merge
    e.close()


def test_f32_options_keyed_on_the_layer():
    """"f32_n256" (cnv5 / cnv6 at 256 columns on the 128x256 tile) takes a coupled cnv6 only at width 256, where it is the flagship's
    GEMM; "pad_classes" 0 runs cnv6 in natural row order.  Both against the default at the parity bar, layer by layer."""
    H, W, B = K.PLAN_H, K.PLAN_W, 5
    for width in (128, 256):
        ver = K.version(width)
        cfg, w = parse_version(ver), K.weights(ver)
        inp = synth.make_inputs(B, H, W, first_window=5)
        e = _engine(cfg, H, W, B, w, "f32")
        base = LC.forward(e, *inp).copy()
        for option, value in (("f32_n256", 1), ("pad_classes", 0)):
            e.set_option(option, value)
            got = LC.forward(e, *inp)
            if option == "f32_n256":
                assert (256 in _tiles(e, 5)) == (width == 256), e.last_plan(5)
            _layer_by_layer(e, cfg, w, inp, got, "f32", "cnv6_%d %s %d" % (width, option, value), images=[0, 2 * B - 1], start="cnv5")
            assert_pose_close(got, base, "%s %d" % (option, value))
            e.set_option(option, 0 if option == "f32_n256" else 1)
        e.close()


# ---- f16x3 siblings --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(3, 64, 96), (2, 128, 416)])
@pytest.mark.parametrize("width", K.WIDTHS)
def test_f16x3_siblings_are_bit_identical(width, B, H, W):
    """share_taps 0 / 1, deep_ring 0 / 1, a forced tile (128x128 where a layer has 128 columns; the 208x256 tile for cnv7 - and for
    cnv6 at width 256) against the planner's launches under one K chain ("split_k" 0): the same products reach every accumulator in the
    same order (tests/test_cnv6_widths_gpu.py: test_f16x3_siblings_are_bit_identical), so stored cnv6, cnv7 and the poses are
    the same bits."""
    ver = K.version(width)
    cfg, w = parse_version(ver), K.weights(ver)
    inp = synth.make_inputs(B, H, W, first_window=11)
    e = _engine(cfg, H, W, B, w, "f16x3")
    e.set_option("split_k", 0)
    e.set_option("fuse_pose", 0)
    sh = C.shapes(cfg, H, W)
    read = lambda: {k: e.debug_read(k, (2 * B,) + sh[k]).copy() for k in ("cnv6", "cnv7")}      # noqa: E731
    base_pose = LC.forward(e, *inp).copy()
    base = read()
    assert 6 not in _tiles(e, 6)
    for options in ({"share_taps": 0}, {"deep_ring": 0}, {"force_tile": 4}, {"force_tile": 6}):
        for k, v in options.items():
            e.set_option(k, v)
        got = LC.forward(e, *inp)
        acts = read()
        if options.get("force_tile") == 6:
            assert _tiles(e, 6) == (6,) and (_tiles(e, 5) == (6,)) == (width == 256), [e.last_plan(li) for li in range(7)]
        for k in base:
            assert np.array_equal(acts[k], base[k]), (options, k)
        assert np.array_equal(got, base_pose), options
        for k, v in {"share_taps": 1, "deep_ring": 1, "force_tile": -1}.items():
            e.set_option(k, v)
    e.close()


@pytest.mark.parametrize("H,W,B", [(36, 100, 2), (52, 172, 2)])
@pytest.mark.parametrize("width", K.WIDTHS)
def test_split_k_on_small_maps(width, H, W, B):
    """cnv6 as one launch of few tiles runs as 2 or 4 parts over K into float32 partial sums of parts x cnv6_out columns (32 columns
    at width 32: a width no decoupled network has) - where the planner's launch is small enough, which davo_last_split reports;
    "split_k" 0 is one chain, "fold_fixup" 1 lets a tile's last part add the sums.  Each layer by layer; the two fix-ups to the bit."""
    ver = K.version(width)
    cfg, w = parse_version(ver), K.weights(ver)
    inp = synth.make_inputs(B, H, W, first_window=3)
    e = _engine(cfg, H, W, B, w, "f16x3")
    sh = C.shapes(cfg, H, W)
    stored = {}
    split_seen = False
    for name, split_k, fold in (("split_k0", 0, 0), ("split_k1", 1, 0), ("fold_fixup", 1, 1)):
        e.set_option("split_k", split_k)
        e.set_option("fold_fixup", fold)
        poses = LC.forward(e, *inp)
        parts = e.last_split(5)
        (bm, bn), = [k for k, v in K.TILE_ID.items() if (v,) == _tiles(e, 5)]
        tiles = -(-2 * B * sh["cnv6"][0] * sh["cnv6"][1] // bm) * (width // bn)
        splits = split_k and 2 * tiles <= 256                      # at most half a workgroup per CU (plan.hip); width 256 at 52x172 runs 144 tiles
        assert parts in (2, 4) if splits else parts == 1, (name, parts, tiles, e.last_plan(5))
        split_seen = split_seen or parts > 1
        assert e.last_split(6) == 1
        _layer_by_layer(e, cfg, w, inp, poses, "f16x3", "cnv6_%d %dx%d B=%d %s" % (width, H, W, B, name), start="cnv4", fused=_fuses(H, W, "f16x3"))
        stored[name] = e.debug_read("cnv6", (2 * B,) + sh["cnv6"]).copy()
    assert np.array_equal(stored["split_k1"], stored["fold_fixup"])
    assert split_seen or (width, H) == (256, 52)
    e.close()


# ---- entry points, to the bit against davo_forward ----------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_device_and_streaming_entry_points_and_repeats(precision):
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, precision)
    first = e.forward(*inp)
    assert_pose_close(first, K.reference(H, W, B), precision)
    for _ in range(50):
        assert np.array_equal(e.forward(*inp), first)
    e.set_option("host_chunk", 1)                                # one window per sub-batch
    assert np.array_equal(e.forward(*inp), first)
    e.set_option("host_chunk", 8)
    bufs = [e.alloc(a.nbytes).upload(a) for a in inp]
    d_pose = e.alloc(B * 12 * 4)
    e.forward_device(B, *bufs, d_pose)
    e.synchronize()
    assert np.array_equal(d_pose.download((B, 2, 6)), first)
    out = np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*inp, out)
    e.wait()
    assert np.array_equal(out, first)
    e.set_inflight(2)
    outs = [np.full((B, 2, 6), np.nan, np.float32) for _ in range(3)]
    for o in outs:
        e.submit(*inp, o)
    e.wait()
    assert all(np.array_equal(o, first) for o in outs)
    shifts = e.calibrate(*inp)                                   # davo_calibrate on a coupled context
    assert set(shifts) >= {"cnv6"}
    assert_pose_close(e.forward(*inp), K.reference(H, W, B), precision + " calibrated")
    for b in bufs + [d_pose]:
        b.free()
    e.close()


@pytest.mark.parametrize("labels,flow_fmt", [("f32", "f32"), ("u8", "f16")])
def test_frame_entry_points_and_the_narrow_formats(labels, flow_fmt):
    """The three `_frames' calls against davo_forward on windows_from_frames of the same arrays, in the default formats and with
    byte labels and binary16 flow; the narrow formats against the float32 engine on the rounded flow."""
    H, W, N = 36, 100, 3
    cfg = parse_version(K.FLAGSHIP_C)
    w = K.weights(K.FLAGSHIP_C)
    fr = synth.make_frames(N + 2, H, W, labels=labels, flow=flow_fmt)
    win = davo_amd.windows_from_frames(*fr)
    e = _engine(cfg, H, W, N, w, "f16x3", labels=labels, flow=flow_fmt)
    want = e.forward(*win)
    assert np.array_equal(e.forward_frames(*fr), want)
    out = np.full((N, 2, 6), np.nan, np.float32)
    e.submit_frames(*fr, out)
    e.wait()
    assert np.array_equal(out, want)
    bufs = [e.alloc(a.nbytes).upload(a) for a in fr]
    d_pose = e.alloc(N * 12 * 4)
    e.forward_device_frames(N, *bufs, d_pose)
    e.synchronize()
    assert np.array_equal(d_pose.download((N, 2, 6)), want)
    for b in bufs + [d_pose]:
        b.free()
    e.close()
    if labels == "u8":                                           # the same network on float labels and the widened flow: the same bits
        fr32 = synth.make_frames(N + 2, H, W)
        assert np.array_equal(labels_to_u8(fr32[2]), fr[2]) and np.array_equal(flow_to_f16(fr32[1]), fr[1])
        win32 = davo_amd.windows_from_frames(fr32[0], fr[1].astype(np.float32), fr32[2])
        f = _engine(cfg, H, W, N, w, "f16x3")
        assert np.array_equal(f.forward(*win32), want)
        f.close()
    assert_pose_close(want, C.forward(cfg, win[0], np.asarray(win[1], np.float32), np.asarray(win[2], np.float32), w), "frames %s %s" % (labels, flow_fmt))


def test_a_depth_source_with_binary16_depth_and_flip():
    """`-se_depth_to_seg' in front of the coupled head: depth planes as binary16 equal the float32 engine on the widened planes to
    the bit and meet the bar; davo_set_flip equals the engine on flip_windows of the inputs."""
    H, W, B = K.SMALL
    version = K.BASE + "-segmask_all-se_depth_to_seg-fc_tanh"
    cfg, inp, w = K.case(H, W, B, version)
    depth = K.depth_planes(H, W, B)
    d16 = depth_to_f16(depth)
    e = _engine(cfg, H, W, B, w, "f16x3", depth="f16")
    got = e.forward(*inp, depth=d16)
    f = _engine(cfg, H, W, B, w, "f16x3")
    assert np.array_equal(f.forward(*inp, depth=d16.astype(np.float32)), got)
    assert_pose_close(f.forward(*inp, depth=depth), K.reference(H, W, B, version), "depth source, float32 planes")
    flipped = davo_amd.flip_windows(*inp, depth)
    want = f.forward(*flipped[:3], depth=flipped[3])
    f.set_flip(True)
    assert np.array_equal(f.forward(*inp, depth=depth), want) and not np.array_equal(want, got)
    e.close()
    f.close()


def _poisoned(inp, sel, W):
    """tests/test_pairs_gpu.py's: the unselected source frame's third of the strip replaced by other bytes, its flow and label planes
    by NaN"""
    out = [a.copy() for a in inp]
    other = 1 - ROW[sel]
    third = slice(0, W) if other == 0 else slice(2 * W, 3 * W)
    out[0][:, :, third] = 255 - out[0][:, :, third]
    out[1][:, other] = np.nan
    out[2][:, 2 * other] = np.nan                                # file order src0, tgt, src1
    return tuple(out)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_pair_batches(precision):
    """davo_set_pairs on a coupled context: the selected row is the both-pairs forward's to the bit (B = 3: an odd image count), the
    other row exactly +0.0, and nothing of the unselected frame is read."""
    H, W, B = 52, 172, 3
    cfg, inp, w = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, precision)
    e.set_option("split_k", 0)                                   # one K chain whatever the image count and a stored cnv7, as
    e.set_option("fuse_pose", 0)                                 # tests/test_pairs_gpu.py has it for its bit comparison
    both = e.forward(*inp).copy()
    assert_pose_close(both, K.reference(H, W, B), precision)
    for sel in ("src1", "src0"):
        e.set_pairs(sel)
        got = e.forward(*inp)
        assert np.array_equal(got[:, ROW[sel]], both[:, ROW[sel]]), sel
        other = got[:, 1 - ROW[sel]]
        assert np.array_equal(other.view(np.uint32), np.zeros(other.shape, np.uint32)), sel      # exactly +0.0
        assert np.array_equal(e.forward(*_poisoned(inp, sel, W)), got), sel
        assert e.debug_read("cnv7", (B,) + C.shapes(cfg, H, W)["cnv7"]).shape[0] == B
    # the default options (f16x3: split-K where the planner picks it, the six-column epilogue on three images - 462 rows, tiles that
    # straddle images, the last cut short): within rounding of both pairs, the other row exactly +0.0
    e.set_option("split_k", 1)
    e.set_option("fuse_pose", 1)
    e.set_pairs("both")
    both = e.forward(*inp).copy()
    e.set_pairs("src1")
    got = e.forward(*inp)
    assert np.abs(got[:, 1] - both[:, 1]).max() <= 1e-6 * np.abs(both).max()
    assert np.array_equal(got[:, 0].view(np.uint32), np.zeros((B, 6), np.uint32))
    assert_pose_close(got[:, 1], K.reference(H, W, B)[:, 1], precision + " src1, default options")
    if _fuses(H, W, precision):
        with pytest.raises(Exception, match="not materialised"):
            e.debug_read("cnv7", (B,) + C.shapes(cfg, H, W)["cnv7"])
        for _ in range(20):
            assert np.array_equal(e.forward(*inp), got)
    e.close()


@pytest.mark.parametrize("H,W,B", [K.SMALL, (128, 416, 1)])
def test_the_direct_convolutions_agree(H, W, B):
    """davo_set_impl(ctx, 1): the raw copies of the one head's tensors on the direct-convolution kernels against the float32 MFMA path."""
    cfg, inp, w = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, "f32")
    mfma = e.forward(*inp).copy()
    e.set_impl("direct")
    direct = e.forward(*inp)
    assert_pose_close(direct, mfma, "impl 1 against the MFMA path")
    assert_pose_close(direct, K.reference(H, W, B), "impl 1")
    e.close()


# ---- range recovery -------------------------------------------------------------------------------------------------------
def test_a_checkpoint_that_leaves_the_range_is_reissued_and_meets_the_bar():
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    want = K.reference(H, W, B)
    e = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    before = e.range_stats()
    assert_pose_close(e.forward(*inp), want, "rescaled, davo_forward")
    mid = e.range_stats()
    assert mid["reissued"] > before["reissued"] and mid["recalibrations"] > before["recalibrations"], (before, mid, e.range_report())
    assert mid["f32_batches"] == 0
    e.close()
    e = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    out = np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*inp, out)
    e.wait()
    e.synchronize()
    assert_pose_close(out, want, "rescaled, davo_submit")
    assert e.range_stats()["reissued"] > 0
    e.close()
    e = _engine(cfg, H, W, B, _rescaled(w, 16), "f16x3")
    e.set_option("auto_range", 0)
    with pytest.raises(DavoRangeError, match="cnv3"):
        e.forward(*inp)
    e.close()


# ---- error codes ------------------------------------------------------------------------------------------------------------
def _load(eng, name, a):
    return eng._L.davo_load_weight(eng._ctx, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (ctypes.c_int64 * a.ndim)(*a.shape), a.ndim)


def test_error_codes():
    H, W, B = 16, 16, 1
    cfg, inp, w = K.case(16, 16, 3)
    e = _engine(cfg, H, W, B, w, "f16x3")
    for heads in (0, 1):                                         # after a weight
        rc = e._L.davo_set_posenn_heads(e._ctx, heads)
        assert rc == INVALID
        with pytest.raises(ValueError, match="before the first davo_load_weight"):
            e._check(rc)
    # the conflicting calls on a coupled context
    with pytest.raises(ValueError, match="feature export"):
        e.set_feature_export(True)
    with pytest.raises(ValueError, match="heat export"):
        e.set_heat_export(True)
    e.set_feature_export(False)
    e.set_heat_export(False)
    assert_pose_close(e.forward(*[a[:1] for a in inp]), K.reference(16, 16, 3)[:1], "after the refused calls")
    e.close()
    raw = Engine(cfg, H, W, B)                                   # a coupled context without weights
    assert raw._L.davo_set_posenn_topology(raw._ctx, 1) == INVALID and "couple_net_v0_dilation" in raw._L.davo_last_error(raw._ctx).decode()
    assert raw._L.davo_set_posenn_topology(raw._ctx, 0) == 0
    k6 = np.zeros((3, 3, 256, cfg.cnv6_out), np.float32)
    assert _load(raw, "pose_exp_net/pose/rotation/cnv6/weights", k6) == INVALID and "not part of this variant" in raw._L.davo_last_error(raw._ctx).decode()
    assert _load(raw, "pose_exp_net/pose/pred/weights", np.zeros((1, 1, 256, 3), np.float32)) == INVALID
    assert _load(raw, "pose_exp_net/pose/pred/weights", np.zeros((1, 1, 256, 6), np.float32)) == 0
    raw.close()
    # davo_set_posenn_se(ctx, 1) on a coupled context of att_source 0 (`-no_segmask', the one source the block runs with: any other is
    # refused one check earlier): the coupled refusal itself, then the mode 0 round trip, and the forward is still the coupled network's
    nver = K.BASE + "-no_segmask"
    ncfg, _, nw = K.case(16, 16, 3, nver)
    assert ncfg.att_source == "ones" and ncfg.as_c_ints()[5] == 0
    raw = Engine(ncfg, H, W, B)
    assert raw._L.davo_set_posenn_se(raw._ctx, 1) == INVALID
    assert "coupled PoseNN (davo_set_posenn_heads)" in raw._L.davo_last_error(raw._ctx).decode(), raw._L.davo_last_error(raw._ctx).decode()
    assert raw._L.davo_set_posenn_se(raw._ctx, 0) == 0
    raw.load_weights(nw)
    assert_pose_close(raw.forward(*[a[:1] for a in inp]), K.reference(16, 16, 3, nver)[:1], "after davo_set_posenn_se(ctx, 1) was refused and (ctx, 0) accepted")
    raw.close()
    # ... and the other order on the same att_source: the block first, then the coupled heads are refused and the block still runs
    from oracle import davo_oracle as O
    sver = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-no_segmask-se_insert"
    scfg = parse_version(sver)
    se = Engine(scfg, H, W, B)
    assert se._L.davo_set_posenn_heads(se._ctx, 1) == INVALID and "davo_set_posenn_se(ctx, 1) is set" in se._L.davo_last_error(se._ctx).decode()
    se.load_weights(synth.make_weights(scfg))
    assert np.isfinite(se.forward(*[a[:1] for a in inp])).all()
    se.close()
    # a decoupled context: values out of range, the other order of the conflicting calls, the coupled names
    dcfg = parse_version(K.FLAGSHIP_C.replace("-dilatedCouplePoseNN", "-dilatedPoseNN"))
    d = Engine(dcfg, H, W, B)
    set_heads = d._L.davo_set_posenn_heads
    assert set_heads(d._ctx, 2) == INVALID and set_heads(d._ctx, -1) == INVALID
    assert _load(d, "pose_exp_net/pose/cnv6/weights", k6) == INVALID and "not part of this variant" in d._L.davo_last_error(d._ctx).decode()
    assert set_heads(d._ctx, 1) == 0 and set_heads(d._ctx, 0) == 0 and set_heads(d._ctx, 1) == 0      # free until the first weight
    assert _load(d, "pose_exp_net/pose/cnv6/weights", k6) == 0
    d.close()
    d = Engine(dcfg, H, W, B)
    assert d._L.davo_set_posenn_topology(d._ctx, 1) == 0
    assert set_heads(d._ctx, 1) == INVALID and "couple_net_v0_dilation" in d._L.davo_last_error(d._ctx).decode()
    assert set_heads(d._ctx, 0) == 0
    d.close()
    for export in ("set_feature_export", "set_heat_export"):
        d = Engine(dcfg, H, W, B)
        getattr(d, export)(True)
        assert set_heads(d._ctx, 1) == INVALID and "export" in d._L.davo_last_error(d._ctx).decode()
        getattr(d, export)(False)
        assert set_heads(d._ctx, 1) == 0
        d.close()
    se = Engine(parse_version("v1-sharedNN-dilatedPoseNN-no_segmask-se_insert"), H, W, B)      # after davo_set_posenn_se(ctx, 1)
    assert se._L.davo_set_posenn_heads(se._ctx, 1) == INVALID and "feature-attention" in se._L.davo_last_error(se._ctx).decode()
    se.close()
    # a decoupled context is still right after the refused calls
    d = Engine(dcfg, H, W, B)
    assert set_heads(d._ctx, 7) == INVALID
    dw = K.weights(dcfg.version)
    d.load_weights(dw)
    from oracle import davo_oracle as O
    assert_pose_close(d.forward(*[a[:1] for a in inp]), O.forward(dcfg, *[a[:1] for a in inp], dw, np.float64), "decoupled after the refused call")
    d.close()
    dd = davo_amd.DAVO(K.FLAGSHIP_C)
    dd.setup_inference(H, W, 'davo', 3, B)
    with pytest.raises(ValueError, match="feature export"):      # the library's message
        dd.enable_feature_mode()
    with pytest.raises(ValueError, match="heat export"):
        dd.enable_feature_mode(features='heat')
    dd.engine.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_heads_and_inflight_slots_in_either_order(precision):
    """davo_set_posenn_heads and davo_set_inflight are both free until the first weight.  A slot built while the context was
    coupled must hold the decoupled network's cnv6 (2 c6 channels) and cnv7 (512) if the heads go back, and the other way round:
    every slot's buffers have the decoupled widths whenever it is built.  Three batches through two slots (so slot 1 runs), to the
    bit against a context that never changed its heads."""
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    dversion = K.FLAGSHIP_C.replace("-dilatedCouplePoseNN", "-dilatedPoseNN")
    dcfg, dw = parse_version(dversion), K.weights(dversion)
    plain = {}
    for name, c, ww in (("coupled", cfg, w), ("decoupled", dcfg, dw)):
        e = _engine(c, H, W, B, ww, precision)
        plain[name] = e.forward(*inp).copy()
        e.close()
    assert_pose_close(plain["coupled"], K.reference(H, W, B), precision)

    def streamed(e, ww):
        e.load_weights(ww)
        e.set_precision(precision)
        outs = [np.full((B, 2, 6), np.nan, np.float32) for _ in range(3)]
        for o in outs:
            e.submit(*inp, o)
        e.wait()
        assert e._L.davo_set_posenn_heads(e._ctx, 1) == INVALID      # the heads are fixed now
        e.close()
        return outs
    # coupled -> two slots -> decoupled: slot 1 was built on a coupled context and runs the decoupled network
    e = Engine(dcfg, H, W, B)
    assert e._L.davo_set_posenn_heads(e._ctx, 1) == 0
    e.set_inflight(2)
    assert e._L.davo_set_posenn_heads(e._ctx, 0) == 0
    assert all(np.array_equal(o, plain["decoupled"]) for o in streamed(e, dw))
    # decoupled -> two slots -> coupled
    e = Engine(dcfg, H, W, B)
    e.set_inflight(2)
    assert e._L.davo_set_posenn_heads(e._ctx, 1) == 0
    e.cfg = cfg                                                  # (Engine.load_weights looks the variables up by its config's names)
    assert all(np.array_equal(o, plain["coupled"]) for o in streamed(e, w))
    # coupled from the start (Engine sets the heads), two slots afterwards
    e = Engine(cfg, H, W, B)
    e.set_inflight(2)
    assert all(np.array_equal(o, plain["coupled"]) for o in streamed(e, w))


# ---- the rest -----------------------------------------------------------------------------------------------------------------
def test_the_davo_class_runs_pose_inference():
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    d = davo_amd.DAVO(K.FLAGSHIP_C)
    d.setup_inference(H, W, 'davo', 3, B, input_img_uint8=inp[0], input_flow=inp[1], input_seglabel=inp[2])
    d.load_weights(w)
    assert_pose_close(d.inference(mode='pose')['pose'], K.reference(H, W, B), "DAVO.inference")
    d.engine.close()


def test_create_and_close_leaves_no_device_memory_behind():
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    free = []
    for _ in range(10):
        e = _engine(cfg, H, W, B, w, "f16x3")
        e.set_inflight(2)
        e.forward(*inp)
        out = np.empty((B, 2, 6), np.float32)
        e.submit(*inp, out)
        e.wait()
        e.close()
        free.append(hip_free_bytes())
    assert free[9] == free[0], free


@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_flagship_is_untouched(flagship_before, precision):
    """A flagship engine beside a live coupled engine of the same library: the plan of all seven layers and the bits of the one
    that ran before any such engine existed."""
    H, W, B = K.SMALL
    cfg, inp, w = K.case(H, W, B)
    t = _engine(cfg, H, W, B, w, precision)
    t.forward(*inp)
    fcfg = parse_version(FLAGSHIP_VERSION)
    f = _engine(fcfg, H, W, B, synth.make_weights(fcfg), precision)
    poses = f.forward(*inp)
    want_poses, want_plan = flagship_before[precision]
    assert [f.last_plan(li) for li in range(7)] == want_plan and np.array_equal(poses, want_poses)
    f.close()
    t.close()


def test_the_cli_writes_a_trajectory_from_a_dump(tmp_path):
    from davo_amd import run_kitti_pose as R
    H, W, seq, n_frames = 64, 96, 9, 6
    dump = str(tmp_path / "dump")
    L.write_synthetic_dump(dump, seq, n_frames, H, W, seed=1234)
    cfg = parse_version(K.FLAGSHIP_C)
    w = K.weights(K.FLAGSHIP_C)
    ckpt = str(tmp_path / "w.npz")
    np.savez(ckpt, **w)
    seen = {}
    inner = S.run_sequences

    def capturing(*a, **k):
        for s, traj, poses, timing in inner(*a, **k):
            seen[s] = poses.copy()
            yield s, traj, poses, timing
    S.run_sequences = capturing
    try:
        R.main(["--test_seq", str(seq), "--concat_img_dir", dump, "--ckpt_file", ckpt, "--version", K.FLAGSHIP_C, "--batch_size", "2",
                "--output_dir", str(tmp_path / "out"), "--img_height", str(H), "--img_width", str(W), "--loader_procs", "0"])
    finally:
        S.run_sequences = inner
    path = os.path.join(str(tmp_path / "out"), "%.2d-pred_kitti_pose.txt" % seq)
    lines = open(path).read().splitlines()
    assert len(lines) == n_frames
    fac = S.kitti_window_loader(dump, None, None, H, W)
    e = _engine(cfg, H, W, n_frames - 2, w, "f16x3")
    parts = [fac.load_inline(seq, k, k + 1) for k in range(n_frames - 2)]
    poses = e.forward(*(np.concatenate([p[k] for p in parts]) for k in range(3)))
    e.close()
    assert seen[seq].shape == (n_frames - 2, 2, 6)
    assert_pose_close(seen[seq], poses, "run_kitti_pose against Engine.forward")
    assert_pose_close(seen[seq][[0, n_frames - 3]], C.forward(cfg, *(np.concatenate([parts[k][j] for k in (0, n_frames - 3)]) for j in range(3)), w),
                      "run_kitti_pose against float64")
    # the file is the stitch of the poses the CLI computed, and those are Engine.forward's
    S.write_kitti_poses(str(tmp_path / "want.txt"), S.stitch_trajectory(seen[seq]))
    assert open(path, "rb").read() == open(str(tmp_path / "want.txt"), "rb").read()
