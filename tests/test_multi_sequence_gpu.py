"""Several sequences in one launch of run_kitti_pose, on the GPU: every sequence's trajectory file is byte for byte the file of a
launch of its own - streamed and synchronous, with the forced gather, with either calibration, at batch 1 and 4, from files and
synthetic, and after a neighbour whose windows tripped the f16x3 range guard - while the launch builds one context, loads the
weights once and builds one communicator, and leaves no device memory behind.  The oracle is the checker only.

The sequences are those of tests/test_multi_sequence.py: 13, 6, 3 and 22 frames of 64x96, each written from its own seed."""
import gc
import json
import os

import numpy as np
import pytest

from davo_amd import synth, parse_version, FLAGSHIP_VERSION
from davo_amd import loader as L
from davo_amd import sequence as S

from helpers import assert_pose_close, hip_free_bytes

pytestmark = pytest.mark.gpu
H, W = 64, 96
SEQS = [(3, 13), (9, 6), (10, 3), (0, 22)]
LIST = "3,9-10,0"
SAMPLED = {3: (0, 5, 10), 9: (0, 3), 10: (0,), 0: (0, 7, 19)}            # windows held against the oracle: first, last, one between


@pytest.fixture(scope="module")
def world(tmp_path_factory, c_oracle):
    """the four dumps, the checkpoint, and the oracle's poses of the sampled windows (computed once)"""
    d = tmp_path_factory.mktemp("multi")
    dump = str(d / "dump")
    for seq, n_frames in SEQS:
        L.write_synthetic_dump(dump, seq, n_frames, H, W, seed=1000 + seq)
    cfg = parse_version(FLAGSHIP_VERSION)
    weights = synth.make_weights(cfg)
    ckpt = str(d / "w.npz")
    np.savez(ckpt, **weights)
    fac = S.kitti_window_loader(dump, None, None, H, W)
    want = {}
    for seq, windows in SAMPLED.items():
        parts = [fac.load_inline(seq, w, w + 1) for w in windows]
        want[seq] = c_oracle.forward(cfg, *(np.concatenate([p[k] for p in parts]) for k in range(3)), weights)
    synth_want = {}
    for seq, n_frames in SEQS:
        windows = SAMPLED[seq]
        parts = [synth.make_inputs(1, H, W, first_window=w) for w in windows]
        synth_want[seq] = c_oracle.forward(cfg, *(np.concatenate([p[k] for p in parts]) for k in range(3)), weights)
    return {"dir": d, "dump": dump, "ckpt": ckpt, "want": want, "synth_want": synth_want}


def run(args, out_dir, monkeypatch=None):
    """run_kitti_pose.main(args) into out_dir -> {seq: poses} of what the run computed (captured from the driver loop)"""
    from davo_amd import run_kitti_pose as R
    seen = {}
    if monkeypatch is not None:
        inner = S.run_sequences

        def capturing(*a, **k):
            for seq, traj, poses, timing in inner(*a, **k):
                seen[seq] = poses.copy()
                yield seq, traj, poses, timing
        monkeypatch.setattr(S, "run_sequences", capturing)
    try:
        R.main(list(args) + ["--output_dir", str(out_dir), "--img_height", str(H), "--img_width", str(W), "--loader_procs", "2"])
    finally:
        if monkeypatch is not None:
            monkeypatch.setattr(S, "run_sequences", inner)
    return seen


def file_of(out_dir, seq):
    return open(os.path.join(str(out_dir), "%.2d-pred_kitti_pose.txt" % seq), "rb").read()


def check_against_single_runs(common, tmp_path, monkeypatch, want, single_args):
    poses = run(common + ["--test_seq", LIST] + single_args(None), tmp_path / "multi", monkeypatch)
    assert list(poses) == [s for s, _ in SEQS]
    for seq, n_frames in SEQS:
        run(common + ["--test_seq", str(seq)] + single_args(n_frames), tmp_path / ("single%d" % seq))
        got, alone = file_of(tmp_path / "multi", seq), file_of(tmp_path / ("single%d" % seq), seq)
        assert len(alone.splitlines()) == n_frames
        assert got == alone, "sequence %.2d: the file of the four-sequence launch differs from the file of its own launch" % seq
        # identical, and not identically wrong: the sampled windows at the oracle's bar
        assert poses[seq].shape == (n_frames - 2, 2, 6)
        assert_pose_close(poses[seq][list(SAMPLED[seq])], want[seq], "sequence %.2d, windows %s" % (seq, SAMPLED[seq]))


@pytest.mark.parametrize("flags", [["--batch_size", "4"], ["--batch_size", "4", "--sync_driver"], ["--batch_size", "4", "--force_comm"],
                                   ["--batch_size", "4", "--calibrate_on_first_windows"], ["--batch_size", "1"]],
                         ids=["streamed", "sync_driver", "force_comm", "calibrate_on_first_windows", "batch1"])
def test_files_from_one_launch_equal_the_files_of_single_launches(world, tmp_path, monkeypatch, flags):
    common = ["--concat_img_dir", world["dump"], "--ckpt_file", world["ckpt"]] + flags
    check_against_single_runs(common, tmp_path, monkeypatch, world["want"], lambda n_frames: [])


def test_synthetic_sequences_from_one_launch_equal_single_launches(world, tmp_path, monkeypatch):
    """--synthetic 13,6,3,22: one count per sequence; a single run's output for --synthetic N is what it always was (no seed
    that depends on the sequence's number: test_sequence_driver_on_gpu holds that run against the oracle)"""
    check_against_single_runs(["--batch_size", "4"], tmp_path, monkeypatch, world["synth_want"],
                              lambda n_frames: ["--synthetic", "13,6,3,22" if n_frames is None else str(n_frames)])


def test_one_launch_builds_one_of_everything(world, tmp_path, monkeypatch):
    from davo_amd import DAVO
    from davo_amd.comm import RcclComm
    calls = {"setup_inference": 0, "load_weights": 0, "from_env_async": 0}
    for cls, name in ((DAVO, "setup_inference"), (DAVO, "load_weights")):
        def counted(self, *a, _inner=getattr(cls, name), _name=name, **k):
            calls[_name] += 1
            return _inner(self, *a, **k)
        monkeypatch.setattr(cls, name, counted)
    inner = RcclComm.from_env_async.__func__

    def from_env_async(cls, engine):
        calls["from_env_async"] += 1
        return inner(cls, engine)
    monkeypatch.setattr(RcclComm, "from_env_async", classmethod(from_env_async))
    report = str(tmp_path / "r.json")
    run(["--concat_img_dir", world["dump"], "--ckpt_file", world["ckpt"], "--batch_size", "4", "--test_seq", LIST, "--force_comm",
         "--report", report], tmp_path)
    assert calls == {"setup_inference": 1, "load_weights": 1, "from_env_async": 1}
    r = json.load(open(report))
    assert [e["seq"] for e in r["sequences"]] == [s for s, _ in SEQS] and r["windows"] == sum(n - 2 for _, n in SEQS)
    assert all(e["streamed"] and e["wall_s"] > 0 and e["gather_s"] >= 0 for e in r["sequences"])
    assert all(os.path.exists(tmp_path / ("%.2d-pred_kitti_pose.txt" % s)) for s, _ in SEQS)
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("psm_")]


def test_a_neighbour_that_trips_the_range_guard_does_not_leak_into_the_next_sequence(tmp_path):
    """One checkpoint serves the whole launch, so the neighbour trips the guard through its inputs (the device tests/test_stream.py
    uses on cnv3's weights, here on the flow): sequence 05's first batch - the windows it is calibrated on - is ordinary, the flow
    fields of its later windows are 4096 times larger, and the layers' values follow the flow far enough (measured: cnv1..cnv6 at
    32..13 reach 58,700..19,400) to run past the 64-128x headroom of the calibrated scales: the guard trips, the batch is re-issued
    and the scales are re-calibrated in mid-sequence.  Sequence 06 after it is ordinary.  Its file must be the file of its own
    launch and its share of the recoveries none: the scales, the records and the counters start over between sequences.
    (Without calibration this network cannot be made to trip through its inputs: whatever the flow's scale, its layers stay
    between 0.19 and 58,700, inside the fp16-pair range on no scales at all.)"""
    dump = str(tmp_path / "dump")
    L.write_synthetic_dump(dump, 5, 13, H, W, seed=1005)
    L.write_synthetic_dump(dump, 6, 13, H, W, seed=1006)
    for w in range(4, 11):
        path = L.window_paths(dump, 5, w + 1)[1]
        np.save(path, np.load(path) * np.float32(4096.0))
    cfg = parse_version(FLAGSHIP_VERSION)
    ckpt = str(tmp_path / "w.npz")
    np.savez(ckpt, **synth.make_weights(cfg))
    common = ["--concat_img_dir", dump, "--ckpt_file", ckpt, "--batch_size", "4"]
    report = str(tmp_path / "r.json")
    run(common + ["--test_seq", "5,6", "--report", report], tmp_path / "multi")
    r = json.load(open(report))
    print("range recoveries per sequence:", [e["range_recovery"] for e in r["sequences"]])
    assert r["sequences"][0]["range_recovery"]["reissued"] >= 1, "the first sequence was meant to trip the guard: %s" % r["sequences"][0]
    assert r["sequences"][1]["range_recovery"] == {"recalibrations": 0, "f32_batches": 0, "reissued": 0}
    run(common + ["--test_seq", "6", "--report", report], tmp_path / "single")
    assert json.load(open(report))["range_recovery"] == {"recalibrations": 0, "f32_batches": 0, "reissued": 0}
    assert file_of(tmp_path / "multi", 6) == file_of(tmp_path / "single", 6)
    run(common + ["--test_seq", "5"], tmp_path / "single")
    assert file_of(tmp_path / "multi", 5) == file_of(tmp_path / "single", 5)


def test_four_sequences_leave_no_more_device_memory_behind_than_one(world, tmp_path):
    common = ["--concat_img_dir", world["dump"], "--ckpt_file", world["ckpt"], "--batch_size", "4"]
    free = []
    for seqs in ("3", "3", LIST, "3"):                       # the first run also pays what the runtime keeps for the process
        run(common + ["--test_seq", seqs], tmp_path)
        gc.collect()
        free.append(hip_free_bytes())
    assert free[1] == free[2] == free[3], free
