"""Mirrored inputs (include/davo_hip.h: davo_set_flip), the parts that need no GPU: the ABI's three statements of the entry
points, the numpy statement of the rule (davo_amd.flip_windows / flip_frames), the drivers' flags, the CLI around the CPU oracle,
and kitti_eval reading the mirrored ground truth."""
import ctypes
import os
import re

import numpy as np
import pytest

import davo_amd
from davo_amd import _lib, synth
from davo_amd import loader as L

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


# ---- header, binding, export list -----------------------------------------------------------------------------------------
def test_header_binding_and_export_list_agree():
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "davo_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+davo_set_flip\s*\(\s*davo_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+davo_get_flip\s*\(\s*const\s+davo_ctx\s*\*\s*\w+\s*\)\s*;", code)
    assert {"davo_set_flip", "davo_get_flip"} <= set(_lib.EXPORTS)
    raw = ctypes.CDLL(_lib.build())
    assert hasattr(raw, "davo_set_flip") and hasattr(raw, "davo_get_flip")
    lib = _lib.lib()
    assert lib.davo_set_flip.argtypes == [ctypes.c_void_p, ctypes.c_int] and lib.davo_get_flip.argtypes == [ctypes.c_void_p]
    assert lib.davo_set_flip(None, 1) == -1 and lib.davo_get_flip(None) == -1          # DAVO_ERR_INVALID without a context


def test_header_states_the_rule_and_the_switch_that_is_not_built():
    text = " ".join(open(os.path.join(ROOT, "include", "davo_hip.h")).read().split())
    for phrase in ("NOT negated", "inside its own third of the strip", "img_flip", "window_mirror", "never written"):
        assert phrase in text, phrase
    doc = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "davo_set_flip" in doc and "img_flip" in doc


# ---- flip_windows / flip_frames ----------------------------------------------------------------------------------------------
def hand_built_window():
    """one window of 1 x 4 pixels: every byte and every float names its frame / plane, its pixel and its channel"""
    W = 4
    img = np.zeros((1, 1, 3 * W, 3), np.uint8)
    for k in range(3):
        for x in range(W):
            img[0, 0, k * W + x] = [100 * k + 10 * x + c for c in range(3)]          # third k, pixel x, channel c
    flow = np.zeros((1, 4, 1, W, 2), np.float32)
    for p in range(4):
        for x in range(W):
            flow[0, p, 0, x] = [(-1) ** x * (p + 1 + 0.25 * x), -(10 * p + x) - 0.5]            # x components of both signs
    seg = np.arange(3 * W, dtype=np.float32).reshape(1, 3, 1, W, 1)
    depth = (100.0 + np.arange(3 * W, dtype=np.float32)).reshape(1, 3, 1, W, 1)
    return img, flow, seg, depth


def test_flip_windows_on_a_hand_built_window():
    img, flow, seg, depth = hand_built_window()
    W = 4
    f_img, f_flow, f_seg, f_depth = davo_amd.flip_windows(img, flow, seg, depth)
    for k in range(3):                                       # each third reversed inside itself, pixels whole, thirds in place
        for x in range(W):
            assert list(f_img[0, 0, k * W + x]) == list(img[0, 0, k * W + (W - 1 - x)])
    assert list(f_img[0, 0, 0]) == [30, 31, 32] and list(f_img[0, 0, 4]) == [130, 131, 132] and list(f_img[0, 0, 11]) == [200, 201, 202]
    for p in range(4):                                       # plane order kept; values unchanged, the x component NOT negated
        for x in range(W):
            assert list(f_flow[0, p, 0, x]) == list(flow[0, p, 0, W - 1 - x])
    assert f_flow[0, 0, 0, 0, 0] == flow[0, 0, 0, 3, 0] == -1.75 and f_flow[0, 0, 0, 3, 0] == 1.0
    assert sorted(f_flow.ravel().tolist()) == sorted(flow.ravel().tolist())
    assert f_seg.ravel().tolist() == [3, 2, 1, 0, 7, 6, 5, 4, 11, 10, 9, 8]
    assert f_depth.ravel().tolist() == [103, 102, 101, 100, 107, 106, 105, 104, 111, 110, 109, 108]
    assert len(davo_amd.flip_windows(img, flow, seg)) == 3
    for a in (f_img, f_flow, f_seg, f_depth):
        assert a.flags.c_contiguous
    with pytest.raises(ValueError):
        davo_amd.flip_windows(img, flow[:, :2], seg)
    with pytest.raises(ValueError):
        davo_amd.flip_windows(img, flow, seg[:, :2])


def test_flip_windows_is_an_involution_and_keeps_dtypes():
    img, flow, seg = synth.make_inputs(2, 16, 20, labels="u8", flow="f16")
    depth = synth.make_depth(2, 16, 20)
    assert flow.dtype == np.float16 and seg.dtype == np.uint8
    once = davo_amd.flip_windows(img, flow, seg, depth)
    assert [a.dtype for a in once] == [np.uint8, np.float16, np.uint8, np.float32]
    assert [a.shape for a in once] == [img.shape, flow.shape, seg.shape, depth.shape]
    assert not np.array_equal(once[0], img) and not np.array_equal(once[1], flow)
    twice = davo_amd.flip_windows(*once)
    for got, want in zip(twice, (img, flow, seg, depth)):
        assert got.dtype == want.dtype and np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8))
    assert davo_amd.flip_windows(img, flow, seg[..., 0])[2].shape == seg.shape[:4]      # byte maps without the trailing axis


@pytest.mark.parametrize("labels,flow", [("f32", "f32"), ("u8", "f16")])
def test_flip_frames_agrees_with_windows_from_frames_then_flip_windows(labels, flow):
    fr = synth.make_frames(6, 16, 24, depth=True, labels=labels, flow=flow)
    a = davo_amd.windows_from_frames(*davo_amd.flip_frames(*fr))
    b = davo_amd.flip_windows(*davo_amd.windows_from_frames(*fr))
    assert len(a) == len(b) == 4
    for x, y, src in zip(a, b, fr):
        assert x.dtype == y.dtype == np.asarray(src).dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    assert [q.shape for q in davo_amd.flip_frames(*fr)] == [np.asarray(q).shape for q in fr]
    assert len(davo_amd.flip_frames(*fr[:3])) == 3


# ---- the drivers' flags --------------------------------------------------------------------------------------------------------
def test_cli_flags_parse():
    from davo_amd import generate_feature_map as G
    from davo_amd import run_kitti_pose as R
    assert R.build_parser().parse_args(["--output_dir", "o"]).flip is False
    assert R.build_parser().parse_args(["--output_dir", "o", "--flip"]).flip is True
    assert G.build_parser().parse_args(["--output_dir", "o"]).flip is False
    assert G.build_parser().parse_args(["--output_dir", "o", "--flip", "--synthetic", "5"]).flip is True
    import inspect
    assert '"-flip"' in inspect.getsource(G.main)                       # the reference's output root with `-flip' appended
    from davo_amd.davo import DAVO
    assert inspect.signature(DAVO.__init__).parameters["flip"].default is False
    assert inspect.signature(DAVO.setup_inference).parameters["flip"].default is None
    assert DAVO("v", flip=True)._flip is True and DAVO("v")._flip is False


# ---- the CLI around the CPU oracle -----------------------------------------------------------------------------------------
H, W, N_FRAMES, SEQ = 32, 64, 6, 3


def write_dump(d, windows):
    """a dump of `windows' (img [n,H,3W,3], flow, seg) in the reference's file layout.  The strips are stored losslessly (PNG data
    under the dump's .jpg names - Pillow reads by content): a JPEG of a mirrored strip does not decode to the mirror of the JPEG."""
    from PIL import Image
    img, flow, seg = windows
    os.makedirs(os.path.join(d, "%.2d" % SEQ), exist_ok=True)
    for w in range(img.shape[0]):
        jpg, flo, sg = L.window_paths(d, SEQ, w + 1)
        Image.fromarray(img[w]).save(jpg, format="PNG")
        np.save(flo, flow[w])
        np.save(sg, seg[w])
    return d


class OracleDAVO:
    """run_kitti_pose's DAVO with the CPU oracle in the engine's place: flip is flip_windows ahead of the forward"""
    made = []

    class _Engine:
        def range_stats(self):
            return {"recalibrations": 0, "f32_batches": 0, "reissued": 0}

        def reset_range_state(self):
            pass

    def __init__(self, version=None, device=0):
        from davo_amd import parse_version
        self.cfg, self.engine, self.flip = parse_version(version), self._Engine(), None
        self.weights = synth.make_weights(self.cfg)
        OracleDAVO.made.append(self)

    def setup_inference(self, *a, flip=None, **k):
        self.flip = flip

    def load_weights(self, weights):
        pass

    def calibrate(self, inputs):
        pass

    def inference(self, sess=None, mode="pose", inputs=None):
        from oracle import c_oracle
        inputs = davo_amd.flip_windows(*inputs) if self.flip else inputs
        return {"pose": c_oracle.forward(self.cfg, *inputs, self.weights, nthreads=2)}


def test_cli_flip_on_a_dump_equals_the_cli_on_the_flipped_dump(c_oracle, monkeypatch, tmp_path):
    import json
    from davo_amd import davo
    from davo_amd import run_kitti_pose as R
    OracleDAVO.made = []
    monkeypatch.setattr(R, "DAVO", OracleDAVO)
    monkeypatch.setattr(davo, "pin_array", lambda arr, device=0: None)          # page-locking needs the GPU's runtime
    monkeypatch.setattr(davo, "unpin_array", lambda arr: None)
    monkeypatch.setattr(davo, "pinned_empty", lambda shape, dtype, device=0: np.empty(shape, dtype))
    X = synth.make_inputs(N_FRAMES - 2, H, W)
    plain = write_dump(str(tmp_path / "plain"), X)
    flipped = write_dump(str(tmp_path / "flipped"), davo_amd.flip_windows(*X))
    np.savez(str(tmp_path / "w.npz"), x=np.zeros(1, np.float32))
    common = ["--ckpt_file", str(tmp_path / "w.npz"), "--batch_size", "3", "--img_height", str(H), "--img_width", str(W), "--loader_procs", "0",
              "--sync_driver", "--test_seq", str(SEQ), "--no_calibrate"]
    R.main(common + ["--concat_img_dir", plain, "--output_dir", str(tmp_path / "a"), "--flip", "--report", str(tmp_path / "a.json")])
    R.main(common + ["--concat_img_dir", flipped, "--output_dir", str(tmp_path / "b"), "--report", str(tmp_path / "b.json")])
    R.main(common + ["--concat_img_dir", plain, "--output_dir", str(tmp_path / "c")])
    assert [m.flip for m in OracleDAVO.made] == [True, None, None]
    name = "%.2d-pred_kitti_pose.txt" % SEQ                                   # the same file name with and without the flag
    a, b, c = (open(tmp_path / d / name, "rb").read() for d in "abc")
    assert a == b and a != c and len(a.splitlines()) == N_FRAMES
    assert json.load(open(tmp_path / "a.json"))["flip"] is True and "flip" not in json.load(open(tmp_path / "b.json"))


# ---- the mirrored ground truth -----------------------------------------------------------------------------------------------
def test_evaluate_reads_the_mirrored_ground_truth_by_pattern(tmp_path):
    import shutil
    from davo_amd import kitti_eval as K
    gt_dir, res_dir = tmp_path / "poses-flip", tmp_path / "res"
    gt_dir.mkdir()
    res_dir.mkdir()
    shutil.copy(os.path.join(HERE, "golden", "kitti_gt_poses_03_flip.txt"), gt_dir / "03-flip.txt")
    shutil.copy(os.path.join(HERE, "golden", "kitti_gt_poses_03_flip.txt"), res_dir / "03-pred_kitti_pose.txt")
    errs = K.evaluate(str(gt_dir), str(res_dir), [3], gt_pattern="%.2d-flip.txt")
    assert list(errs) == ["03"] and len(errs["03"]) > 0
    assert float(np.abs(np.asarray(errs["03"])[:, 1:3]).max()) < 1e-9          # the file against itself: no error
    with pytest.raises((FileNotFoundError, OSError)):
        K.evaluate(str(gt_dir), str(res_dir), [3])                             # the default pattern still looks for 03.txt
    # the unmirrored trajectory is a different one: evaluated against the mirrored ground truth it is far off
    shutil.copy(os.path.join(HERE, "golden", "kitti_gt_poses_03.txt"), res_dir / "03-pred_kitti_pose.txt")
    off = K.evaluate(str(gt_dir), str(res_dir), [3], gt_pattern="%.2d-flip.txt")
    assert float(np.asarray(off["03"])[:, 2].mean()) > 0.01
