"""Several sequences in one launch (run_kitti_pose --test_seq 0,2,5-7), without a GPU: the list grammar, run_sequences
against run_sequence sequence by sequence, two ranks over gloo, the process loader serving several segments from one
worker pool and one ring, the report and the failure path of the CLI around a stand-in for the GPU engine.

The sequences: 13, 6, 3 and 22 frames (11, 4, 1 and 20 windows) of 64x96 - multiples of neither the 4-window chunk nor of every
batch size, one window only, less than a batch, and at world 2 a rank without a window.  Each is written from its own seed: a
window taken from the wrong sequence changes the result."""
import json
import os

import numpy as np
import pytest

from davo_amd import loader as L
from davo_amd import sequence as S

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 64, 96
SEQS = [(3, 13), (9, 6), (10, 3), (0, 22)]                 # (sequence number, frames), in running order


def seed_of(seq):
    return 1000 + seq


def write_dumps(d, seqs=SEQS, depth=False):
    for seq, n_frames in seqs:
        assert L.write_synthetic_dump(d, seq, n_frames, H, W, seed=seed_of(seq), depth=depth) == n_frames - 2
    return d


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return write_dumps(str(tmp_path_factory.mktemp("dumps")))


def fake_infer(img, flow, seg, depth=None):
    """[B,2,6] from each window's own bytes, and only the planes every loader fills (flow 0,1; the source frames' label maps):
    row by row, so a window's result does not depend on its batch"""
    B = img.shape[0]
    out = np.zeros((B, 2, 6), np.float32)
    for i in range(B):
        a = float(np.asarray(img[i], np.float64).mean()) / 255.0
        third = [float(np.asarray(img[i][:, k * W:(k + 1) * W], np.float64).mean()) / 255.0 for k in range(3)]
        f = [float(np.asarray(flow[i, k], np.float64).mean()) for k in (0, 1)]
        g = [float(np.asarray(seg[i, k], np.float64).mean()) for k in (0, 2)]
        d = 0.0 if depth is None else float(np.asarray(depth[i], np.float64).mean())
        out[i, 0] = [a, third[0], f[0], g[0], third[1] - third[2], d]
        out[i, 1] = [f[1], g[1], a * f[0], third[2], g[0] - g[1], a + d]
    return 0.05 * out


def inline_source(dump):
    fac = S.kitti_window_loader(dump, None, None, H, W)
    return lambda k, seq, n_frames, lo, hi: (lambda s, e: fac.load_inline(seq, s, e))


def alone(dump, seq, n_frames, B, emulate=None):
    fac = S.kitti_window_loader(dump, seq, n_frames, H, W)
    return S.run_sequence(fake_infer, fac.__call__, n_frames, B, emulate=emulate)


# ---- the list grammar -------------------------------------------------------------------------------------------------
def test_sequence_list_grammar():
    assert S.parse_seq_list("9") == [9] and S.parse_seq_list("03") == [3]
    assert S.parse_seq_list("0,2,5-7") == [0, 2, 5, 6, 7]
    assert S.parse_seq_list("0-10") == list(range(11))
    assert S.parse_seq_list("7,3,10,0") == [7, 3, 10, 0] and S.parse_seq_list("5-6,1-2") == [5, 6, 1, 2]     # order as given
    assert S.parse_seq_list("4-4") == [4] and S.parse_seq_list(" 1 , 2 ") == [1, 2]
    for bad in ("3,3", "1-4,2", "1,,2", "", "3,", "7-5", "a", "1-", "-1", "1-2-3", "2.5"):
        with pytest.raises(ValueError):
            S.parse_seq_list(bad)
    assert S.parse_frame_counts("13", 4) == [13] * 4 and S.parse_frame_counts("13,6,3,22", 4) == [13, 6, 3, 22]
    for bad, n in (("13,6", 4), ("13,6,3,22,5", 4), ("13,", 2), ("x", 1)):
        with pytest.raises(ValueError):
            S.parse_frame_counts(bad, n)


def test_cli_takes_a_list_and_rejects_a_bad_one_before_anything_starts(tmp_path, capsys):
    from davo_amd import run_kitti_pose as R
    ap_args = ["--output_dir", str(tmp_path), "--img_height", str(H), "--img_width", str(W)]
    for bad in (["--test_seq", "3,3", "--synthetic", "13"], ["--test_seq", "7-5", "--synthetic", "13"],
                ["--test_seq", "3,,9", "--synthetic", "13"], ["--test_seq", "3,9", "--synthetic", "13,6,3"],
                ["--test_seq", "3,9", "--synthetic", "13,2"]):
        with pytest.raises(SystemExit) as exc:
            R.main(ap_args + bad)
        assert exc.value.code == 2
    assert "named twice" in capsys.readouterr().err

    class Args:
        test_seq, synthetic, concat_img_dir, seq_length, ckpt_file = "3,9-10,0", "13,6,3,22", None, 3, None
    assert R.sequences_to_run(Args) == ([(3, 13), (9, 6), (10, 3), (0, 22)], True)
    Args.test_seq, Args.synthetic = "3", "13"
    assert R.sequences_to_run(Args) == ([(3, 13)], True)


# ---- the driver loop --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 4, 8])
def test_every_sequence_equals_its_own_run(dump, B):
    got = list(S.run_sequences(fake_infer, SEQS, inline_source(dump), B))
    assert [g[0] for g in got] == [s for s, _ in SEQS]
    for (seq, n_frames), (_, traj, poses, timing) in zip(SEQS, got):
        want_traj, want_poses = alone(dump, seq, n_frames, B)
        assert poses.shape == (n_frames - 2, 2, 6) and np.array_equal(poses, want_poses)
        assert np.array_equal(np.array(traj), np.array(want_traj))
        assert timing["windows_this_rank"] == n_frames - 2 and {"load_wait_s", "forward_s", "gather_s", "stitch_s"} <= set(timing)
    # the sequences differ (a window from the wrong one would show)
    assert not np.array_equal(got[0][2][:4], got[1][2][:4])


@pytest.mark.parametrize("r", [0, 1])
def test_emulated_shards_equal_their_own_runs(dump, r):
    for B in (1, 4, 8):
        got = list(S.run_sequences(fake_infer, SEQS, inline_source(dump), B, emulate=(r, 2)))
        for (seq, n_frames), (_, traj, poses, timing) in zip(SEQS, got):
            want_traj, want_poses = alone(dump, seq, n_frames, B, emulate=(r, 2))
            assert np.array_equal(poses, want_poses) and np.array_equal(np.array(traj), np.array(want_traj))
            lo, hi = S.shard_windows(n_frames - 2, 2, r)
            assert timing["windows_this_rank"] == hi - lo
    assert S.shard_windows(1, 2, 1) == (1, 1)              # the one-window sequence leaves rank 1 without a window


class LateStream:
    """delivers at drain() only, as PoseStream may; counts what it is asked"""

    def __init__(self):
        self.jobs, self.drains, self.sizes = [], 0, []

    def submit(self, img, flow, seg, out, depth=None):
        self.sizes.append(img.shape[0])
        self.jobs.append((fake_infer(img, flow, seg, depth), out))

    def drain(self):
        self.drains += 1
        for poses, out in self.jobs:
            out[...] = poses
        self.jobs = []


def test_streamed_run_drains_at_every_sequence_end_and_hooks_run_in_order(dump):
    st, seen = LateStream(), []

    def hook(k, seq, n_frames, load):
        assert not st.jobs                                   # the sequence before has been drained
        seen.append((k, seq, n_frames))
    got = list(S.run_sequences(None, SEQS, inline_source(dump), 4, stream=st, before_sequence=hook))
    assert st.drains == len(SEQS) and seen == [(k, s, n) for k, (s, n) in enumerate(SEQS)]
    assert st.sizes == [4] * (3 + 1 + 1 + 5)                # each sequence batched on its own (11, 4, 1, 20 windows), short batches padded
    for (seq, n_frames), (_, traj, poses, _) in zip(SEQS, got):
        assert np.array_equal(poses, alone(dump, seq, n_frames, 4)[1])


def test_a_failing_sequence_is_named_and_the_stream_is_drained_first(dump):
    st = LateStream()

    def source(k, seq, n_frames, lo, hi):
        def load(s, e):
            if seq == 10:
                raise IOError("gone")
            return S.kitti_window_loader(dump, seq, n_frames, H, W).load_inline(seq, s, e)
        return load
    it = S.run_sequences(None, SEQS, source, 4, stream=st)
    assert next(it)[0] == 3 and next(it)[0] == 9
    drains = st.drains
    with pytest.raises(S.SequenceError, match="sequence 10 failed") as exc:
        next(it)
    assert exc.value.seq == 10 and isinstance(exc.value.__cause__, IOError) and st.drains == drains + 1


# ---- two ranks --------------------------------------------------------------------------------------------------------
class GlooComm:
    """RcclComm's allgather contract over gloo on CPU (the stand-in of tests/test_sequence.py)"""

    def __init__(self, rank, world):
        self.rank, self.world = rank, world

    def allgather(self, local, n_per_rank=None):
        import torch
        import torch.distributed as dist
        local = np.ascontiguousarray(local, np.float32).reshape(-1, 2, 6)
        per = local.shape[0] if n_per_rank is None else n_per_rank
        buf = torch.zeros((per, 2, 6), dtype=torch.float32)
        buf[:local.shape[0]] = torch.from_numpy(local)
        parts = [torch.empty_like(buf) for _ in range(self.world)]
        dist.all_gather(parts, buf)
        return torch.cat(parts, 0).numpy(), 0.0


def _rank_main(rank, world, port, dump, B, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = [(seq, np.array(traj), poses, timing["windows_this_rank"])
           for seq, traj, poses, timing in S.run_sequences(fake_infer, SEQS, inline_source(dump), B, rank, world, GlooComm(rank, world))]
    q.put((rank, out))
    dist.destroy_process_group()


def test_two_ranks_over_gloo_match_the_single_process(dump):
    import torch.multiprocessing as mp
    B = 4
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, dump, B, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank in (0, 1):
        assert [o[0] for o in results[rank]] == [s for s, _ in SEQS]
        for (seq, n_frames), (_, traj, poses, mine) in zip(SEQS, results[rank]):
            want_traj, want_poses = alone(dump, seq, n_frames, B)
            assert np.array_equal(poses, want_poses) and np.array_equal(traj, np.array(want_traj))
            lo, hi = S.shard_windows(n_frames - 2, 2, rank)
            assert mine == hi - lo
    assert results[1][2][3] == 0                            # rank 1 had no window of the one-window sequence and gathered all the same


# ---- the process loader over several segments ---------------------------------------------------------------------------
def consumed_equal(parts, ref, seg_planes=(0, 2)):
    img, flow, seg = parts[:3]
    ok = np.array_equal(img, ref[0]) and np.array_equal(flow[:2], ref[1][:2]) and np.array_equal(seg[list(seg_planes)], ref[2][list(seg_planes)])
    return ok and (len(parts) == 3 or np.array_equal(parts[3], ref[3]))


def shm_names(ld):
    return [sm.name.lstrip("/") for trio in ld._segs for sm in trio] + [ld._ctrl_shm.name.lstrip("/")]


@pytest.mark.parametrize("B,procs,chunk", [(4, 3, None), (8, 2, None), (1, 2, None), (5, 3, 2)])
def test_segments_come_from_one_pool_and_one_ring(dump, B, procs, chunk):
    """every window of every segment equals the inline load; the same worker processes serve all segments; every buffer is
    page-locked once; segments that start inside a sequence and lengths that are multiples of nothing keep the ring's ownership"""
    segments = [(3, 0, 11), (9, 1, 4), (10, 0, 1), (10, 1, 1), (0, 3, 20)]      # one empty (a rank without a window), two that start late
    pins, unpins = [], []
    ld = L.ProcessWindowLoader(dump, None, H, W, None, None, B, procs=procs, prefetch=1, chunk=chunk, segments=segments,
                               pin=lambda a: pins.append(a.ctypes.data), unpin=lambda a: unpins.append(a.ctypes.data))
    assert len(ld) == sum(-(-(hi - lo) // B) for _, lo, hi in segments) and ld.worker_pids() == []
    ld.start()
    pids, names = ld.worker_pids(), shm_names(ld)
    assert len(set(pids)) == procs
    with pytest.raises(TypeError):
        iter(ld)
    with pytest.raises(ValueError):
        ld.segment(1)                                       # in order only
    for k, (seq, lo, hi) in enumerate(segments):
        at = lo
        for s, e, parts in ld.segment(k):
            assert s == at and e == min(s + B, hi) and parts[0].shape[0] == e - s
            for i, w in enumerate(range(s, e)):
                assert consumed_equal(tuple(p[i] for p in parts), L.load_window(dump, seq, w + 1, H, W)), (seq, w)
            at = e
        assert at == max(lo, hi)
        if k + 1 < len(segments):
            assert ld.worker_pids() == pids                 # the same processes after the boundary
            assert all(os.path.exists("/dev/shm/" + n) for n in names)
    assert ld.worker_pids() == []                           # the last segment's end stops the workers
    ld.close()                                              # joins the page-locking thread
    assert len(pins) == ld.nring * 3 and len(set(pins)) == len(pins)          # once per buffer, not once per segment
    assert sorted(unpins) == sorted(pins)
    assert not any(os.path.exists("/dev/shm/" + n) for n in names)


def test_chunk_ownership_follows_the_batch_index_not_the_window_number():
    """what the workers and the consumer agree on: a batch's place in the ring and its chunks' owners come from its index in the
    run, so a segment of 11 or of 1 window shifts nothing for the next one"""
    segments = [(3, 0, 11), (9, 0, 4), (10, 0, 1), (0, 0, 20)]
    for B in (1, 4, 8):
        batches = L._segment_batches(segments, B)
        per_seq = [[(s, e) for q, s, e in batches if q == seq] for seq, _, _ in segments]
        assert per_seq == [[(s, min(s + B, hi)) for s in range(lo, hi, B)] for _, lo, hi in segments]       # each batched on its own
        cpb, nring, P = -(-B // min(4, B)), 5, 3
        for bi in range(len(batches)):
            for j in range(cpb):
                c = bi * cpb + j
                assert L._chunk_owner(c, cpb * nring, P) == L._chunk_owner(c % (cpb * nring), cpb * nring, P) == ((bi % nring) * cpb + j) % P


def test_hold_keeps_the_last_batch_of_a_segment_across_the_boundary(dump):
    import time
    segments = [(3, 0, 11), (9, 0, 4), (0, 0, 20)]
    ld = L.ProcessWindowLoader(dump, None, H, W, None, None, 4, procs=2, prefetch=1, hold=1, segments=segments)
    held = None
    for k, (seq, lo, hi) in enumerate(segments):
        for s, e, parts in ld.segment(k):
            time.sleep(0.05)                                # the workers run ahead as far as the ring lets them
            if held is not None:                            # the batch before this one - of the segment before, at a boundary - is intact
                hseq, hs, he, hparts = held
                for i, w in enumerate(range(hs, he)):
                    assert consumed_equal(tuple(p[i] for p in hparts), L.load_window(dump, hseq, w + 1, H, W)), (hseq, w, "held over", seq, s)
            held = (seq, s, e, parts)
    ld.close()


def test_a_missing_file_in_the_second_segment_fails_there_and_not_before(dump, tmp_path):
    import shutil
    d2 = str(tmp_path / "broken")
    shutil.copytree(dump, d2)
    os.remove(L.window_paths(d2, 9, 2)[2])
    ld = L.ProcessWindowLoader(d2, None, H, W, None, None, 4, procs=3, segments=[(3, 0, 11), (9, 0, 4), (0, 0, 20)]).start()
    names = shm_names(ld)
    got = [(s, e) for s, e, parts in ld.segment(0)
           if all(consumed_equal(tuple(p[i] for p in parts), L.load_window(d2, 3, s + i + 1, H, W)) for i in range(e - s))]
    assert got == [(0, 4), (4, 8), (8, 11)]                 # the first segment is served whole, although the workers have met the gap
    with pytest.raises(FileNotFoundError):
        list(ld.segment(1))
    assert ld.worker_pids() == []
    ld.close()
    assert not any(os.path.exists("/dev/shm/" + n) for n in names)


def test_depth_planes_over_two_segments(tmp_path):
    d = write_dumps(str(tmp_path / "depth"), [(9, 6), (10, 3), (4, 7)], depth=True)
    segments = [(9, 0, 4), (10, 0, 1), (4, 0, 5)]
    ld = L.ProcessWindowLoader(d, None, H, W, None, None, 4, procs=2, depth=True, segments=segments, seg_planes=(0, 1, 2))
    for k, (seq, lo, hi) in enumerate(segments):
        n = 0
        for s, e, parts in ld.segment(k):
            assert len(parts) == 4
            for i, w in enumerate(range(s, e)):
                assert consumed_equal(tuple(p[i] for p in parts), L.load_window(d, seq, w + 1, H, W, depth=True), (0, 1, 2))
            n += e - s
        assert n == hi - lo
    ld.close()


def test_factory_hands_out_segments_of_one_loader_or_threaded_loaders(dump):
    segments = [(seq, 0, n - 2) for seq, n in SEQS]
    want = [alone(dump, seq, n, 4)[1] for seq, n in SEQS]
    for procs in (2, 0):
        fac = S.kitti_window_loader(dump, None, None, H, W, procs=procs, workers=2)
        fac.prestart_segments(segments, 4)
        assert (fac.segment_loader is not None) == (procs > 0)
        pids = fac.segment_loader.worker_pids() if procs else None
        got = list(S.run_sequences(fake_infer, SEQS, lambda k, seq, n, lo, hi: fac.for_segment(k, segments, 4), 4))
        assert all(np.array_equal(g[2], w) for g, w in zip(got, want))
        if procs:
            assert len(pids) == 2 and fac.segment_loader.worker_pids() == []
        fac.close()
        assert fac.segment_loader is None


# ---- the CLI around a stand-in for the engine ---------------------------------------------------------------------------
class FakeEngine:
    max_batch = 4

    def __init__(self):
        self.resets = 0

    def range_stats(self):
        return {"recalibrations": 0, "f32_batches": 0, "reissued": 0}

    def reset_range_state(self):
        self.resets += 1


class FakeDAVO:
    made = []

    def __init__(self, version=None, device=0):
        self.engine, self.calibrated = FakeEngine(), []
        FakeDAVO.made.append(self)

    def setup_inference(self, *a, **k):
        pass

    def load_weights(self, weights):
        pass

    def calibrate(self, inputs):
        self.calibrated.append(inputs[0].shape[0])

    def inference(self, sess=None, mode="pose", inputs=None):
        return {"pose": fake_infer(*inputs)}


@pytest.fixture
def cli(monkeypatch):
    from davo_amd import run_kitti_pose as R
    FakeDAVO.made = []
    monkeypatch.setattr(R, "DAVO", FakeDAVO)
    from davo_amd import davo
    monkeypatch.setattr(davo, "pin_array", lambda arr, device=0: None)          # page-locking needs the GPU's runtime
    monkeypatch.setattr(davo, "unpin_array", lambda arr: None)
    monkeypatch.setattr(davo, "pinned_empty", lambda shape, dtype, device=0: np.empty(shape, dtype))
    return R


TODAY = {"load_wait_s", "forward_s", "gather_s", "stitch_s", "windows_this_rank", "write_s", "startup", "total_s", "windows", "world",
         "batch_size", "windows_per_s", "range_recovery", "note"}            # what a --sync_driver run has always reported


def test_report_of_one_sequence_is_unchanged_and_of_three_is_per_sequence(cli, dump, tmp_path):
    np.savez(str(tmp_path / "w.npz"), x=np.zeros(1, np.float32))
    common = ["--concat_img_dir", dump, "--ckpt_file", str(tmp_path / "w.npz"), "--output_dir", str(tmp_path), "--batch_size", "4",
              "--img_height", str(H), "--img_width", str(W), "--loader_procs", "2", "--sync_driver", "--report", str(tmp_path / "r.json")]
    cli.main(common + ["--test_seq", "3"])
    one = json.load(open(tmp_path / "r.json"))
    assert set(one) == TODAY and one["windows"] == 11 and FakeDAVO.made[-1].engine.resets == 0
    single = open(tmp_path / "03-pred_kitti_pose.txt").read()
    cli.main(common + ["--test_seq", "9-10,3"])
    three = json.load(open(tmp_path / "r.json"))
    assert set(three) == {"startup", "world", "batch_size", "windows", "total_s", "note", "sequences"}
    assert three["windows"] == 4 + 1 + 11 and len(three["sequences"]) == 3 and [e["seq"] for e in three["sequences"]] == [9, 10, 3]
    for e, n in zip(three["sequences"], (4, 1, 11)):
        assert set(e) == (TODAY - {"startup", "world", "batch_size", "note"}) | {"seq", "wall_s"}
        assert e["windows"] == n and e["wall_s"] >= e["write_s"] >= 0 and e["range_recovery"] == one["range_recovery"]
    assert abs(three["total_s"] - sum(e["wall_s"] for e in three["sequences"])) < 1e-3
    system = FakeDAVO.made[-1]
    assert len(FakeDAVO.made) == 2 and system.engine.resets == 2 and system.calibrated == [4, 1, 4]      # each on its own first batch
    assert open(tmp_path / "03-pred_kitti_pose.txt").read() == single            # the same file as the sequence's own launch
    assert len(open(tmp_path / "10-pred_kitti_pose.txt").read().splitlines()) == 3
    assert not [f for f in os.listdir("/dev/shm") if f.startswith("psm_")]


def test_a_missing_sequence_directory_is_named_before_any_context_exists(cli, dump, tmp_path):
    np.savez(str(tmp_path / "w.npz"), x=np.zeros(1, np.float32))
    args = ["--concat_img_dir", dump, "--output_dir", str(tmp_path), "--img_height", str(H), "--img_width", str(W)]
    with pytest.raises(SystemExit, match=r"sequence 07: no directory .*07"):
        cli.main(args + ["--ckpt_file", str(tmp_path / "w.npz"), "--test_seq", "3,7,9"])
    with pytest.raises(SystemExit, match="no checkpoint"):
        cli.main(args + ["--ckpt_file", str(tmp_path / "nothing.npz"), "--test_seq", "3,9"])
    assert FakeDAVO.made == [] and not os.path.exists(tmp_path / "03-pred_kitti_pose.txt")


def test_a_file_that_vanished_ends_the_run_naming_its_sequence(cli, dump, tmp_path):
    import shutil
    d2 = str(tmp_path / "broken")
    shutil.copytree(dump, d2)
    os.remove(L.window_paths(d2, 10, 1)[1])
    np.savez(str(tmp_path / "w.npz"), x=np.zeros(1, np.float32))
    before = set(os.listdir("/dev/shm"))
    with pytest.raises(S.SequenceError, match="sequence 10 failed"):
        cli.main(["--concat_img_dir", d2, "--ckpt_file", str(tmp_path / "w.npz"), "--output_dir", str(tmp_path / "out"), "--batch_size", "4",
                  "--img_height", str(H), "--img_width", str(W), "--loader_procs", "2", "--sync_driver", "--test_seq", "3,9,10,0"])
    assert sorted(os.listdir(tmp_path / "out")) == ["03-pred_kitti_pose.txt", "09-pred_kitti_pose.txt"]      # what was written stays
    assert set(os.listdir("/dev/shm")) <= before
