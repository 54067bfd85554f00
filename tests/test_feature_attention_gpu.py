"""The feature-attention PoseNN (`-se_insert') on the GPU against the float64 restatement of tests/feature_attention_ref.py.

Layer by layer, each launch judged on the GPU's own input to it (Engine.debug_read):
  cnv5_se_scale  from the GPU's cnv5 by the literal reading (mean of the scaled tensor), absolute, SCALE_TOL;
  cnv5_se        from the GPU's cnv5 and the GPU's scales, element-wise: f16x3 2^-20 |ref| + STORE_FLOOR 2^-shift (one float32
                 product - the table already holds s_r s_t - and a re-split at 2^-22, together below 2^-21), float32 2^-22 |ref|;
  cnv6           per group from the matching half of cnv5_se, then cnv7 and the pose head, under tests/layer_check.py's bars;
and the poses end to end at tests/helpers.py's parity bar (1e-4 absolute and relative).  The conditions on the inputs (scales
not saturated, different from image to image) are asserted on the restatement alone in tests/test_feature_attention.py."""
import ctypes

import numpy as np
import pytest

from davo_amd import Engine, synth, parse_version, FLAGSHIP_VERSION
from davo_amd.davo import DavoRangeError

import feature_attention_cases as K
import feature_attention_ref as F
import layer_check as LC
from helpers import assert_pose_close, hip_free_bytes

pytestmark = pytest.mark.gpu

PRECISIONS = ["f16x3", "f32"]
# The scale table against float64, absolute (the entries are sigmoids and products of two): layer_check.TABLE_TOL = 2e-6.  Worst
# seen on an MI355X over every case below and both precisions (the SCALE_WORST lines of the test's output): 2.7e-7, below a
# quarter of the bar, so the bar stays (layer_check.TAU's convention would otherwise raise it to 4x the measurement).
SCALE_TOL = LC.TABLE_TOL
SE_REL = {"f16x3": 2.0 ** -20, "f32": 2.0 ** -22}
SMALL = (36, 100, 2)


def _engine(cfg, H, W, max_batch, weights, precision):
    e = Engine(cfg, H, W, max_batch)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


@pytest.fixture(scope="module", autouse=True)
def flagship_before():
    """One flagship forward before any feature-attention engine exists in this process (the module's first act)."""
    cfg = parse_version(FLAGSHIP_VERSION)
    H, W, B = SMALL
    inp = K.inputs(B, H, W)
    out = {}
    for precision in PRECISIONS:
        e = _engine(cfg, H, W, B, synth.make_weights(cfg), precision)
        out[precision] = (e.forward(*inp), [e.last_plan(li) for li in range(7)])
        e.close()
    return out


def _se_shapes(H, W):
    H2, W2 = LC.out_size(LC.out_size(H, 2), 2), LC.out_size(LC.out_size(W, 2), 2)
    return H2, W2


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H,W,B,max_batch,c6", K.SHAPES, ids=K.IDS)
def test_layer_by_layer(H, W, B, max_batch, c6, precision):
    cfg, inp, w, _ = K.case(H, W, B, c6)
    what = "%dx%d B=%d cnv6_%d %s" % (H, W, B, c6, precision)
    NB = 2 * B
    H2, W2 = _se_shapes(H, W)
    e = _engine(cfg, H, W, max_batch, w, precision)
    e.set_option("fuse_pose", 0)                               # cnv7 is stored: the last layer is checked like the others
    poses = LC.forward(e, *inp)
    assert e.last_split(5) == 1, "the grouped cnv6 takes no split-K plan"
    c5 = e.debug_read("cnv5", (NB, H2, W2, 256)).astype(np.float64)
    # -- the scales, from the GPU's cnv5
    scale = e.debug_read("cnv5_se_scale", (NB, 2, 256))
    err = float(np.abs(scale.astype(np.float64) - F.scale_table(c5, w)).max())
    print("SCALE_WORST %s: cnv5_se_scale max|err| %.3g (bar %.1g)" % (what, err, SCALE_TOL))
    assert err <= SCALE_TOL, (what, err)
    # -- the scaled tensor, from the GPU's cnv5 and the GPU's scales
    shifts = e.activation_range()[1] if precision == "f16x3" else {}
    se = e.debug_read("cnv5_se", (NB, H2, W2, 512))
    ref = np.concatenate([c5 * scale[:, 0].astype(np.float64)[:, None, None, :], c5 * scale[:, 1].astype(np.float64)[:, None, None, :]], -1)
    floor = LC.STORE_FLOOR * 2.0 ** -shifts["cnv5"] if precision == "f16x3" else 0.0
    excess = np.abs(se - ref) - (SE_REL[precision] * np.abs(ref) + floor)
    i = np.unravel_index(int(np.argmax(excess)), excess.shape)
    assert excess[i] <= 0, "%s cnv5_se at %s: got %.9g, ref %.9g" % (what, i, se[i], ref[i])
    # -- cnv6 per group from its half of cnv5_se, cnv7, the pose head: on every pair image, the first and the last at full size
    images = list(range(NB)) if H * W < 128 * 416 else sorted({0, NB - 1})
    g6 = [(w["pose_exp_net/pose/%s/cnv6/weights" % h], w["pose_exp_net/pose/%s/cnv6/biases" % h],
           slice(256 * k, 256 * (k + 1)), slice(c6 * k, c6 * (k + 1))) for k, h in enumerate(F.HEADS)]
    got6 = e.debug_read("cnv6", (NB, H2, W2, 2 * c6))[images]
    floor6 = LC.STORE_FLOOR * 2.0 ** -shifts["cnv6"] if precision == "f16x3" else 0.0
    a, b = LC.check_layer("cnv6", got6, se[images], g6, 1, 2, LC.TAU[precision]["cnv6"], what, floor6)
    print("%s: cnv6 bar (a) %.3g bar (b) %.3g" % (what, a, b))
    name, _, stride, rate, g7 = LC.layers(cfg, w)[6]
    got7 = e.debug_read("cnv7", (NB,) + LC.shapes(cfg, H, W)["cnv7"])[images]
    LC.check_layer("cnv7", got7, got6, g7, stride, rate, LC.TAU[precision]["cnv7"], what, LC.STORE_FLOOR if precision == "f16x3" else 0.0)
    LC.check_pose(np.asarray(poses, np.float64).reshape(NB, 6)[images], LC.pose_from_cnv7(got7, w), what + " pose head")
    # -- end to end
    want = K.reference(H, W, B, c6)
    perr = assert_pose_close(poses, want, what)
    print("%s: pose max|err| %.3g of max|pose| %.3g" % (what, perr, np.abs(want).max()))
    e.set_option("fuse_pose", 1)                               # the default plan (fused pose head where the map allows)
    assert_pose_close(LC.forward(e, *inp), want, what + " fuse_pose 1")
    e.close()


def test_the_direct_cross_check_runs_the_block():
    """davo_set_impl(ctx, 1) must not return the poses of the network without the block."""
    H, W, B = SMALL
    cfg, inp, w, _ = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, "f32")
    e.set_impl("direct")
    assert_pose_close(e.forward(*inp), K.reference(H, W, B), "impl 1")
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_swapped_windows_swap_the_poses_to_the_bit(precision):
    """With the 0.01 spread between images (tests/test_feature_attention.py) a scale read from the wrong image shows here."""
    H, W, B = SMALL
    cfg, inp, w, _ = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, precision)
    a = e.forward(*inp)
    b = e.forward(*[np.ascontiguousarray(x[::-1]) for x in inp])
    assert not np.array_equal(a[0], a[1])
    assert np.array_equal(b, a[::-1])
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_repeats_and_the_streaming_entry_give_the_same_bits(precision):
    H, W, B = SMALL
    cfg, inp, w, _ = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, precision)
    first = e.forward(*inp)
    scale = e.debug_read("cnv5_se_scale", (2 * B, 2, 256))
    for _ in range(20):
        assert np.array_equal(e.forward(*inp), first)
    assert np.array_equal(e.debug_read("cnv5_se_scale", (2 * B, 2, 256)), scale)
    out = np.full((B, 2, 6), np.nan, np.float32)
    e.submit(*inp, out)
    e.wait()
    assert np.array_equal(out, first)
    e.set_inflight(2)                                          # a second slot gets a workspace of its own
    outs = [np.full((B, 2, 6), np.nan, np.float32) for _ in range(3)]
    for o in outs:
        e.submit(*inp, o)
    e.wait()
    assert all(np.array_equal(o, first) for o in outs)
    e.close()


def _shut(weights):
    """recover biases of -20 in both blocks: scales of 1e-10 .. 1e-7, the scaled tensor far under the storage floor"""
    w = dict(weights)
    for head in F.HEADS:
        k = "pose_exp_net/pose/%s/cnv5_se_attention/recover_fc/bias" % head
        w[k] = np.full_like(weights[k], -20.0)
    return w


def test_a_scaled_tensor_under_the_floor_ends_on_the_float32_kernels():
    H, W, B = SMALL
    cfg, inp, w, cnv5 = K.case(H, W, B)
    w = _shut(w)
    want = F.forward(cfg, *inp, w, cnv5=cnv5)
    assert np.abs(cnv5).max() * F.scale_table(cnv5, w).max() < LC.GUARD_FLOOR / 64          # on the restatement: far under the floor at shift 0
    e = _engine(cfg, H, W, B, w, "f16x3")
    before = e.range_stats()
    got = e.forward(*inp)                                      # returns: never an error under the default auto_range
    assert_pose_close(got, want, "cnv5_se under the floor")
    after = e.range_stats()
    assert after["f32_batches"] == before["f32_batches"] + 1, (before, after)
    assert "cnv5_se" in e.range_report(), e.range_report()
    out = np.full((B, 2, 6), np.nan, np.float32)               # the ticketed device path reaches the same end
    e.submit(*inp, out)
    e.wait()
    assert_pose_close(out, want, "cnv5_se under the floor, submit")
    assert e.range_stats()["f32_batches"] == after["f32_batches"] + 1 and "cnv5_se" in e.range_report()
    e.close()
    e = _engine(cfg, H, W, B, w, "f16x3")
    e.set_option("auto_range", 0)
    with pytest.raises(DavoRangeError, match="cnv5_se"):
        e.forward(*inp)
    e.close()


def test_the_mode_is_fixed_before_the_first_weight():
    H, W, B = SMALL
    cfg, inp, w, _ = K.case(H, W, B)
    e = _engine(cfg, H, W, B, w, "f16x3")
    for mode in (0, 1):
        rc = e._L.davo_set_posenn_se(e._ctx, mode)
        assert rc == -1, rc                                    # DAVO_ERR_INVALID
        with pytest.raises(ValueError, match="before the first davo_load_weight"):
            e._check(rc)
    assert_pose_close(e.forward(*inp), K.reference(H, W, B), "after the refused calls")
    e.close()
    # an input-attention source beside it is refused by the library as by the parser
    fcfg = parse_version(FLAGSHIP_VERSION)
    f = Engine(fcfg, H, W, B)
    rc = f._L.davo_set_posenn_se(f._ctx, 1)
    assert rc == -1
    with pytest.raises(ValueError, match="no_segmask"):
        f._check(rc)
    f.close()
    # a plain engine refuses the block's variables; the mode can be set and cleared while nothing is loaded
    p = Engine(parse_version(K.PLAIN), H, W, B)
    name = "pose_exp_net/pose/rotation/cnv5_se_attention/recover_fc/bias"
    a = np.zeros(256, np.float32)
    load = lambda: p._L.davo_load_weight(p._ctx, name.encode(), a.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), (ctypes.c_int64 * 1)(256), 1)   # noqa: E731
    assert load() == -1
    assert p._L.davo_set_posenn_se(p._ctx, 1) == 0 and load() == 0
    p.close()


def test_create_and_close_leaves_no_device_memory_behind():
    H, W, B = SMALL
    cfg, inp, w, _ = K.case(H, W, B)
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
    """A flagship engine beside a live feature-attention engine of the same library: the plan and the bits of the one that ran
    before any such engine existed."""
    H, W, B = SMALL
    cfg, inp, w, _ = K.case(H, W, B)
    se = _engine(cfg, H, W, B, w, precision)
    se.forward(*inp)
    fcfg = parse_version(FLAGSHIP_VERSION)
    f = _engine(fcfg, H, W, B, synth.make_weights(fcfg), precision)
    poses = f.forward(*inp)
    want_poses, want_plan = flagship_before[precision]
    assert [f.last_plan(li) for li in range(7)] == want_plan
    assert f.last_plan(5) == want_plan[5] and np.array_equal(poses, want_poses)
    f.close()
    se.close()
