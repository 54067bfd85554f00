"""Pair selection (include/davo_hip.h: davo_set_pairs), the parts that need no GPU: the contract the 'trajectory' mode rests on
(stitch_trajectory reads row 0 of window 0 and row 1 of every window, test_kitti_pose.py:143-145), the driver's choice of a
selection per batch, the CLI flag, the launch planner on odd pair-image counts, and the ABI."""
import ctypes
import os
import re

import numpy as np
import pytest

from davo_amd import _lib, sequence as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    return _lib.build()


def _random_poses(n, seed=7):
    rng = np.random.RandomState(seed)
    p = np.empty((n, 2, 6), np.float32)
    p[..., :3] = rng.uniform(-0.2, 0.2, (n, 2, 3))
    p[..., 3:] = rng.uniform(-1.5, 1.5, (n, 2, 3))
    return p


def test_the_stitch_reads_row_0_of_the_first_window_only():
    p = _random_poses(40)
    q = p.copy()
    q[1:, 0] = 0.0
    a, b = S.stitch_trajectory(p), S.stitch_trajectory(q)
    assert len(a) == len(b) == 42
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    # ... and it does read what is left: zeroing either of them moves the chain
    r = q.copy()
    r[0, 0] = 0.0
    assert not np.array_equal(np.array(S.stitch_trajectory(r)), np.array(a))
    r = q.copy()
    r[17, 1] = 0.0
    assert not np.array_equal(np.array(S.stitch_trajectory(r)), np.array(a))


# ---- a recording stand-in for the engine: poses are a function of the window's id, rows that were not selected are zero -------
H, W = 4, 4


def _load(offset=0):
    def load(s, e):
        n = e - s
        img = np.zeros((n, H, 3 * W, 3), np.uint8)
        assert e + offset < 256                                   # the id rides in a byte of the strip
        img[:, 0, 0, 0] = np.arange(s, e) + offset
        return img, np.zeros((n, 4, H, W, 2), np.float32), np.zeros((n, 3, H, W, 1), np.float32)
    return load


def _poses_of(ids, pairs):
    ids = np.asarray(ids, np.float32)
    out = np.empty((ids.shape[0], 2, 6), np.float32)
    for s in range(2):
        for k in range(6):
            out[:, s, k] = np.float32(0.01) * np.sin(ids * np.float32(0.37) + np.float32(s * 6 + k))
    if pairs == "src1":
        out[:, 0] = 0.0
    elif pairs == "src0":
        out[:, 1] = 0.0
    return out


class Recorder:
    """infer_fn and stream in one: every call is recorded as (first window id, batch size, pairs or None)"""

    def __init__(self):
        self.calls, self.jobs = [], []

    def infer(self, img, flow, seg, **kw):
        assert set(kw) <= {"pairs"}
        self.calls.append((int(img[0, 0, 0, 0]), img.shape[0], kw.get("pairs")))
        return _poses_of(img[:, 0, 0, 0], kw.get("pairs", "both"))

    def submit(self, img, flow, seg, out, **kw):
        assert set(kw) <= {"pairs"}
        self.calls.append((int(img[0, 0, 0, 0]), img.shape[0], kw.get("pairs")))
        self.jobs.append((img[:, 0, 0, 0].copy(), kw.get("pairs", "both"), out))      # delivered late, like the library

    def drain(self):
        for ids, pairs, out in self.jobs:
            out[...] = _poses_of(ids, pairs)
        self.jobs = []


def _expected_calls(n_frames, B, world=1, rank=0, offset=0):
    lo, hi = S.shard_windows(n_frames - 2, world, rank)
    return [(s + offset, B, "both" if s == 0 else "src1") for s in range(lo, hi, B)]


# (frames, batch): several batches, a sequence shorter than one batch, a ragged last batch
CASES = [(14, 4), (5, 8), (13, 3), (12, 5)]


@pytest.mark.parametrize("streamed", [False, True])
@pytest.mark.parametrize("n_frames,B", CASES)
def test_trajectory_mode_issues_both_pairs_for_window_0_only(n_frames, B, streamed):
    ref = Recorder()
    want_traj, want_poses = S.run_sequence(ref.infer, _load(), n_frames, B)
    assert all(c[2] is None for c in ref.calls)                   # 'both': the calls are made as they always were
    r = Recorder()
    traj, poses = S.run_sequence(None if streamed else r.infer, _load(), n_frames, B, stream=r if streamed else None, pairs="trajectory")
    assert r.calls == _expected_calls(n_frames, B)
    assert sum(1 for c in r.calls if c[2] == "both") == 1
    assert np.array_equal(np.array(traj), np.array(want_traj))
    # the rows the stitch reads are the both-pairs ones; the others were not run
    first = min(B, n_frames - 2)
    assert np.array_equal(poses[:, 1], want_poses[:, 1]) and np.array_equal(poses[:first, 0], want_poses[:first, 0])
    assert not poses[first:, 0].any()


def test_unknown_mode_is_refused_before_anything_runs():
    r = Recorder()
    with pytest.raises(ValueError, match="pairs"):
        S.run_sequence(r.infer, _load(), 9, 4, pairs="src1")
    assert r.calls == []
    assert S.batch_pairs("both", 0) is None and S.batch_pairs("trajectory", 0) == "both" and S.batch_pairs("trajectory", 8) == "src1"


@pytest.mark.parametrize("streamed", [False, True])
def test_two_sequences_in_one_launch_repeat_the_both_pairs_batch(streamed):
    sequences = [(3, 11), (7, 4), (9, 10)]                        # the second is shorter than a batch
    B = 4
    r, ref = Recorder(), Recorder()
    source = lambda k, seq, n_frames, lo, hi: _load(20 * seq)    # noqa: E731
    want = list(S.run_sequences(ref.infer, sequences, source, B))
    got = list(S.run_sequences(None if streamed else r.infer, sequences, source, B, stream=r if streamed else None, pairs="trajectory"))
    expect = []
    for seq, n_frames in sequences:
        expect += _expected_calls(n_frames, B, offset=20 * seq)
    assert r.calls == expect
    assert [c[0] for c in r.calls if c[2] == "both"] == [60, 140, 180]
    for (seq, traj, _, _), (wseq, wtraj, _, _) in zip(got, want):
        assert seq == wseq and np.array_equal(np.array(traj), np.array(wtraj))


def _rank_main(rank, world, port, n_frames, B, q):
    import torch.distributed as dist
    from test_sequence import GlooComm
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    r = Recorder()
    traj, poses = S.run_sequence(r.infer, _load(), n_frames, B, rank, world, GlooComm(rank, world), pairs="trajectory")
    q.put((rank, r.calls, np.array(traj), poses))
    dist.destroy_process_group()


def test_two_ranks_only_the_owner_of_window_0_runs_both_pairs():
    """world 2 over gloo (tests/test_sequence.py's stand-in for the RCCL gather): 11 windows, shards of 6 and 5, batches of 4 -
    ragged on both ranks.  Rank 0's first batch runs both pairs; every other batch of either rank runs src1."""
    import torch.multiprocessing as mp
    n_frames, B = 13, 4
    ref = Recorder()
    want_traj, _ = S.run_sequence(ref.infer, _load(), n_frames, B)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 31500 + os.getpid() % 2000
    procs = [ctx.Process(target=_rank_main, args=(r, 2, port, n_frames, B, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = dict((rank, rest) for rank, *rest in (q.get(timeout=300) for _ in range(2)))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank in (0, 1):
        calls, traj, poses = results[rank]
        assert calls == _expected_calls(n_frames, B, 2, rank), (rank, calls)
        assert np.array_equal(traj, np.array(want_traj))
        assert poses.shape == (11, 2, 6) and not poses[B:, 0].any()
    assert [c[2] for c in results[1][0]] == ["src1", "src1"]


def test_cli_flag():
    from davo_amd import run_kitti_pose as R
    ap = R.build_parser()
    assert ap.parse_args(["--output_dir", "x"]).pairs == "both"
    assert ap.parse_args(["--output_dir", "x", "--pairs", "trajectory"]).pairs == "trajectory"
    action = next(a for a in ap._actions if a.dest == "pairs")
    assert tuple(action.choices) == ("both", "trajectory")
    with pytest.raises(SystemExit):
        ap.parse_args(["--output_dir", "x", "--pairs", "src1"])


def test_planner_covers_odd_pair_image_counts(built):
    """One pair per window makes the pair-image count odd for odd batches.  davo_plan_layer on M = n x P rows, n in {1, 3, 5},
    P the cnv2..cnv6 map of a 64x96 and of a 128x416 frame, for the padded widths and group counts the seven layers use
    (cnv1 16 -> 32, cnv2 32, cnv3 64, cnv4 128, cnv5 / cnv6 256, the feature-attention cnv6 and cnv7 256 x 2 groups): the
    launches cover the rows exactly once, in order, with tiles that divide the width."""
    L = ctypes.CDLL(built)
    L.davo_plan_layer.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 3
    for P in (16 * 24, 32 * 104):
        for n in (1, 3, 5):
            M = n * P
            for npad, groups in ((32, 1), (64, 1), (128, 1), (256, 1), (256, 2), (128, 2)):
                rows, bm, bn = (ctypes.c_int * 2)(), (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
                k = L.davo_plan_layer(M, npad, groups, rows, bm, bn)
                assert k in (1, 2), (M, npad, groups, k)
                assert sum(rows[i] for i in range(k)) == M, (M, npad, groups)
                for i in range(k):
                    assert rows[i] > 0 and bm[i] > 0 and bn[i] > 0 and npad % bn[i] == 0
                if k == 2:                      # the kernels address tiles from row 0 of the layer
                    assert rows[0] % bm[0] == 0 and rows[0] % bm[1] == 0
                # the tiles of the plan, walked: every row of M in exactly one tile
                covered, row0 = 0, 0
                for i in range(k):
                    tiles = -(-rows[i] // bm[i])
                    covered += min(tiles * bm[i], rows[i])
                    assert (tiles - 1) * bm[i] < rows[i]
                    row0 += rows[i]
                assert covered == M and row0 == M


def test_abi_declares_exports_and_binds_the_entry_points(built):
    src = open(os.path.join(ROOT, "include", "davo_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+davo_set_pairs\s*\(\s*davo_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", code)
    assert re.search(r"\bint\s+davo_get_pairs\s*\(\s*const\s+davo_ctx\s*\*\s*\w+\s*\)\s*;", code)
    for name, value in (("DAVO_PAIRS_SRC0", 1), ("DAVO_PAIRS_SRC1", 2), ("DAVO_PAIRS_BOTH", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), code), name
    assert "test_kitti_pose.py:143-145" in src
    raw = ctypes.CDLL(built)
    assert hasattr(raw, "davo_set_pairs") and hasattr(raw, "davo_get_pairs")
    assert {"davo_set_pairs", "davo_get_pairs"} <= set(_lib.EXPORTS)
    L = _lib.lib()
    assert L.davo_set_pairs.argtypes == [ctypes.c_void_p, ctypes.c_int] and L.davo_get_pairs.argtypes == [ctypes.c_void_p]
    assert L.davo_set_pairs(None, 3) == -1 and L.davo_get_pairs(None) == -1          # DAVO_ERR_INVALID without a context
    from davo_amd import Engine
    assert Engine.PAIRS == {"src0": 1, "src1": 2, "both": 3} and isinstance(Engine.pairs, property)
