"""The class-table attention sources (att_source 4..10: segmentation, rgb and seg+flow descriptors) on the GPU, against the
float64 restatement of tests/class_table_ref.py.  Bar: tests/helpers.py (1e-4 absolute and relative)."""
import numpy as np
import pytest

from davo_amd import DAVO, Engine, synth, parse_version
from davo_amd.version import weight_shapes

import class_table_ref as R
from helpers import assert_pose_close

pytestmark = pytest.mark.gpu

BASE = "v1-decay100k-sharedNN-dilatedPoseNN-cnv6_128-segmask_all"
VARIANTS = [BASE + s for s in ("-se_seg_wo_tgt-fc_tanh", "-se_rgb_wo_tgt_to_seg-fc_tanh", "-se_rgb_to_seg-fc_tanh",
                               "-se_SegFlow_to_seg_wo_tgt-fc_tanh", "-se_SegFlow_to_seg-norm_flow-fc_tanh",
                               "-se_SegFlow_to_seg_8_wo_tgt-fc_tanh", "-se_SegFlow_to_seg_8-abs_flow-fc_tanh")]
PRECISIONS = ["f16x3", "f32"]


def _engine(cfg, H, W, B, weights, precision):
    e = Engine(cfg, H, W, B)
    e.load_weights(weights)
    e.set_precision(precision)
    return e


def _inputs(B, H, W):
    img, flow, seg = synth.make_inputs(B, H, W)
    seg[0, 0, :3, :5] = np.nan                  # labels outside the 19 classes: no bin, no table row
    seg[-1, 1, 4:9, 10:13] = -0.75              # truncates to class 0
    seg[-1, 2, :2] = 19.0
    return img, flow, seg


_REF = {}


def _reference(version):
    if version not in _REF:
        cfg = parse_version(version)
        img, flow, seg = _inputs(2, 64, 96)
        w = synth.make_weights(cfg)
        _REF[version] = (cfg, img, flow, seg, w, R.forward(cfg, img, flow, seg, w))
    return _REF[version]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("version", VARIANTS)
def test_variant_matches_the_restatement(version, precision):
    """64x96, B = 2: the excitation folded into the squeeze launch (the default at this batch) and as a launch of its own
    give the same bits, and both match the restatement."""
    cfg, img, flow, seg, w, want = _reference(version)
    e = _engine(cfg, 64, 96, 2, w, precision)
    got = e.forward(img, flow, seg)
    assert_pose_close(got, want, version)
    e.set_option("fold_tails", 0)
    assert np.array_equal(e.forward(img, flow, seg), got)
    e.close()


def test_device_entry_and_class_surface():
    version = VARIANTS[4]                       # with-target SegFlow, -norm_flow
    cfg, img, flow, seg, w, want = _reference(version)
    e = _engine(cfg, 64, 96, 2, w, "f16x3")
    bufs = [e.alloc(a.nbytes) for a in (img, flow, seg)] + [e.alloc(2 * 2 * 6 * 4)]
    for buf, a in zip(bufs, (img, flow, seg)):
        buf.upload(a)
    e.forward_device(2, *bufs)
    e.synchronize()
    assert_pose_close(bufs[3].download((2, 2, 6)), want, "davo_forward_device")
    for buf in bufs:
        buf.free()
    e.close()
    system = DAVO(version=version)
    system.setup_inference(64, 96, "davo", 3, 2, img, input_flow=flow, input_seglabel=seg)
    system.load_weights(w)
    assert_pose_close(system.inference(None, mode='pose')['pose'], want, "DAVO.inference")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_full_size_submit_reads_the_target_label_plane(c_oracle, precision):
    """128x416, B = 4, through davo_submit: at B >= 4 the streaming path copies only the label planes the variant reads;
    a with-target source reads the target's."""
    cfg = parse_version(BASE + "-se_SegFlow_to_seg_8-fc_tanh")
    img, flow, seg = _inputs(4, 128, 416)
    w = synth.make_weights(cfg)
    want = R.forward(cfg, img, flow, seg, w, conv=c_oracle.conv2d_same)
    e = _engine(cfg, 128, 416, 4, w, precision)
    out = np.empty((4, 2, 6), np.float32)
    e.submit(img, flow, seg, out)
    e.wait()
    assert_pose_close(out, want, "submit 128x416")
    e.close()


def _equivalent_weights(cfg, static_weights):
    w = {k: v for k, v in static_weights.items() if "seg_channel_weight" not in k}
    for name, shape in weight_shapes(cfg).items():
        if name.startswith("pose_exp_net/%s/" % cfg.se_scope):
            w[name] = np.zeros(shape, np.float32)
    w["pose_exp_net/%s/recover_fc/bias" % cfg.se_scope] = static_weights["pose_exp_net/pose_exp_net/seg_channel_weight/weight"].copy()
    return w


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("sub,static", [("-se_seg_wo_tgt-fc_tanh", "-static"), ("-se_rgb_to_seg-fc_tanh", "")])
def test_zero_kernels_reproduce_the_static_attention_to_the_bit(sub, static, precision):
    """Zero kernels and recover_fc/bias = the static weight vector make the class table the static one: -se_seg_wo_tgt gives
    exactly the poses of -segmask_all-static, -se_rgb_to_seg those of -segmask_all (target masked too).  Host and submit
    paths, B = 2 (excitation folded) and B = 5 (a launch of its own, label planes copied per the target rule)."""
    cfg, scfg = parse_version(BASE + sub), parse_version(BASE + static)
    ws = synth.make_weights(scfg)
    w = _equivalent_weights(cfg, ws)
    img, flow, seg = _inputs(5, 64, 96)
    es, ec = _engine(scfg, 64, 96, 5, ws, precision), _engine(cfg, 64, 96, 5, w, precision)
    for B in (2, 5):
        a, b = es.forward(img[:B], flow[:B], seg[:B]), ec.forward(img[:B], flow[:B], seg[:B])
        assert np.array_equal(a, b), (B, np.abs(a - b).max())
        oa, ob = np.empty((B, 2, 6), np.float32), np.empty((B, 2, 6), np.float32)
        es.submit(img[:B], flow[:B], seg[:B], oa)
        ec.submit(img[:B], flow[:B], seg[:B], ob)
        es.wait()
        ec.wait()
        assert np.array_equal(oa, a) and np.array_equal(ob, a)
    es.close()
    ec.close()


def test_ignore_label_everywhere_zeroes_target_and_sources():
    """seg = 255 everywhere in a with-target source: every table row is unused, the target and source rgb and the flow are
    all masked to zero, so neither the images nor the flow change the pose."""
    cfg = parse_version(BASE + "-se_rgb_to_seg-fc_tanh")
    img, flow, seg = synth.make_inputs(2, 64, 96)
    seg255 = np.full_like(seg, 255.0)
    w = synth.make_weights(cfg)
    e = _engine(cfg, 64, 96, 2, w, "f16x3")
    got = e.forward(img, flow, seg255)
    assert_pose_close(got, R.forward(cfg, img, flow, seg255, w), "all-ignore")
    img2 = (255 - img).astype(np.uint8)
    flow2 = flow * np.float32(3.0)
    assert np.array_equal(e.forward(img2, flow2, seg255), got)
    e.close()


@pytest.mark.parametrize("precision", PRECISIONS)
def test_repeated_forwards_are_bit_identical(precision):
    cfg = parse_version(BASE + "-se_SegFlow_to_seg-abs_flow-fc_tanh")
    img, flow, seg = synth.make_inputs(6, 64, 96)
    e = _engine(cfg, 64, 96, 6, synth.make_weights(cfg), precision)
    first = e.forward(img, flow, seg)
    for _ in range(3):
        assert np.array_equal(e.forward(img, flow, seg), first)
    e.close()


def test_cli_restores_a_with_target_variant_from_a_tf_bundle(tmp_path, c_oracle):
    """run_kitti_pose --version <-se_rgb_to_seg> --ckpt_file <TF bundle> on a dump in the reference's on-disk format: the
    loader decodes the target label plane too, and the trajectory matches the restatement on the same decoded files."""
    from davo_amd import run_kitti_pose, sequence as S, loader as L, tf_checkpoint as T
    version = BASE + "-se_rgb_to_seg-fc_tanh"
    cfg = parse_version(version)
    dump = str(tmp_path / "dump")
    L.write_synthetic_dump(dump, 9, 9, 64, 96)
    weights = synth.make_weights(cfg)
    ck = tmp_path / "ckpt"
    ck.mkdir()
    T.write_checkpoint(str(ck / "model-1"), weights)
    run_kitti_pose.main(["--concat_img_dir", dump, "--ckpt_file", str(ck), "--output_dir", str(tmp_path), "--version", version,
                         "--test_seq", "9", "--batch_size", "4", "--img_height", "64", "--img_width", "96"])
    got = S.read_kitti_poses(str(tmp_path / "09-pred_kitti_pose.txt"))
    infer = lambda img, flow, seg: R.forward(cfg, img, flow, seg, weights, conv=c_oracle.conv2d_same)   # noqa: E731
    want, _ = S.run_sequence(infer, S.kitti_window_loader(dump, 9, 9, 64, 96).__call__, 9, 4)
    assert got.shape == (9, 4, 4) and np.abs(got - np.array(want)).max() < 2e-4
