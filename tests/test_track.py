"""Online tracking on the host (include/davo_hip.h "Online tracking"; davo_amd/track.py, davo_amd/frames.py): the ABI's new
symbols, the bytes a push copies - from the function the library's copies use -, the ring's index rule, the Tracker's pose chain
against a fake engine, the per-push helper and the --online flag.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

import davo_amd
from davo_amd import _lib, synth
from davo_amd import frames as F
from davo_amd import sequence as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("davo_track_begin", "davo_track_push", "davo_track_push_device", "davo_track_frames", "davo_track_end", "davo_track_plan",
       "davo_track_ring", "davo_track_debug_fill")


def test_new_symbols_are_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "davo_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(davo_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(_lib.build())
    for name in NEW:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert "DAVO_TRACK_TRAJECTORY = 0" in src and "DAVO_TRACK_AS_SET = 1" in src
    assert (_lib.TRACK_TRAJECTORY, _lib.TRACK_AS_SET) == (0, 1)


# ---- davo_track_plan --------------------------------------------------------------------------------------------------------
def test_link_bytes_of_a_push_at_the_flagship_shape():
    """the header's figures: a frame + one float32 flow plane + one float32 label map per lane, against davo_submit_frames' N = 1"""
    assert F.track_plan(128, 416, 1, "src1") == 159744 + 425984 + 212992 == 798720
    assert F.track_plan(128, 416, 1, "src1", labels="u8", flow="f16") == 159744 + 212992 + 53248 == 425984
    assert F.frames_plan(128, 416, 1, "src1")["link_bytes"] == 958464
    assert F.frames_plan(128, 416, 1, "src1", labels="u8", flow="f16")["link_bytes"] == 585728
    assert F.track_plan(128, 416, 3, "src1") == 3 * 798720


def test_a_push_is_a_one_window_frame_batch_less_the_frames_sent_again():
    """every att_source, both one-pair selections and both pairs, every label, flow and depth format: one frame, one label map
    and one depth plane (where the source reads depth) cross the link per push, whatever the batch of one window reads"""
    H, W = 36, 100
    elem = {"f32": 4, "u8": 1, "f16": 2}
    n = 0
    for att in range(18):
        for pairs in ("src0", "src1", "both"):
            for labels in ("f32", "u8"):
                for flow in ("f32", "f16"):
                    for depth in ("f32", "f16"):
                        p = F.frames_plan(H, W, 1, pairs, att, labels, flow, depth)
                        again = lambda r: max(r[1] - r[0] - 1, 0)      # noqa: E731
                        resent = H * W * (3 * again(p["frames"]) + elem[labels] * again(p["seg"]) + elem[depth] * again(p["depth"]))
                        for lanes in (1, 3):
                            assert F.track_plan(H, W, lanes, pairs, att, labels, flow, depth) == lanes * (p["link_bytes"] - resent), \
                                (att, pairs, labels, flow, depth, lanes)
                        n += 1
    assert n == 18 * 3 * 8
    bad = [(0, 16, 1, 2, 0, 0, 0, 0), (16, 16, 0, 2, 0, 0, 0, 0), (16, 16, 1, 4, 0, 0, 0, 0), (16, 16, 1, 2, 18, 0, 0, 0),
           (16, 16, 1, 2, 0, 2, 0, 0), (16, 16, 1, 2, 0, 0, 2, 0), (16, 16, 1, 2, 0, 0, 0, 2)]
    out = ctypes.c_longlong(0)
    for args in bad:
        assert _lib.lib().davo_track_plan(*args, ctypes.byref(out)) == -1, args
    assert _lib.lib().davo_track_plan(16, 16, 1, 2, 0, 0, 0, 0, None) == 0


# ---- the ring's index rule --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("inflight", [1, 2, 3, 4])
def test_ring_rule(inflight):
    """For every ring size the library can choose (slots + 2) and pushes 0..20: a push's window reads the places its three frames
    were uploaded into; the place push t overwrites is not among the places push t - 1 reads unless push t - 1 is one of the
    pushes whose gather the upload is ordered behind (the documented event); and that ordering names EVERY earlier push that
    read the place's previous frame."""
    steps = [F.track_ring(inflight, t) for t in range(21)]
    R = steps[0]["R"]
    assert R == inflight + 2 and all(s["R"] == R for s in steps)
    holds = {}                                             # place -> the push whose frame it holds
    for t, s in enumerate(steps):
        assert s["upload"] == t % R
        if t >= 1 and s["upload"] in steps[t - 1]["read"]:
            assert t - 1 in s["upload_after"], (t, s)      # only R = 3 gets here
            assert R == 3
        # everyone who read the frame this upload destroys gathered before it
        readers = [u for u in range(2, t) if s["upload"] in steps[u]["read"] and holds_at(steps, u, s["upload"]) == holds.get(s["upload"])]
        assert sorted(readers) == sorted(u for u in s["upload_after"] if u >= 0), (t, readers, s)
        holds[s["upload"]] = t
        if t < 2:
            assert s["read"] == (-1, -1, -1)
            continue
        assert len(set(s["read"])) == 3
        assert [holds[p] for p in s["read"]] == [t - 2, t - 1, t]      # the window's three frames, still in place
        assert s["gather_after"] == (t - 2, t - 1)
        # with the slots rotating, the youngest gather an upload waits for ran on the upload's own stream
        assert max(s["upload_after"]) in (-1, t - inflight)
    assert _lib.lib().davo_track_ring(0, 0, None, None) == -1 and _lib.lib().davo_track_ring(5, 0, None, None) == -1
    assert _lib.lib().davo_track_ring(1, -1, None, None) == -1


def holds_at(steps, u, place):
    """the push whose frame `place' held when push u gathered"""
    R = steps[0]["R"]
    return max(v for v in range(u + 1) if v % R == place)


# ---- the Tracker's chain ----------------------------------------------------------------------------------------------------
class FakeEngine:
    """Engine.track_* with poses from a list; delivery lags `lag' pushes behind"""

    def __init__(self, poses, lanes, lag):
        self.poses, self.lanes, self.lag, self.t, self.outs, self.delivered, self.ended = poses, lanes, lag, 0, [], 0, False

    def track_begin(self, lanes, policy):
        assert lanes == self.lanes and policy == "trajectory"

    def track_push(self, frames, flow2, seg, out, hold=0, depth=None):
        self.t += 1
        if self.t < 3:
            return 0
        self.outs.append(out)
        self._deliver(len(self.outs) - self.lag)
        return self.lanes

    def _deliver(self, upto):
        while self.delivered < upto:
            self.outs[self.delivered][...] = self.poses[self.delivered]
            self.delivered += 1

    def pending(self):
        return len(self.outs) - self.delivered

    def wait(self):
        self._deliver(len(self.outs))

    def track_end(self):
        self.ended = True


@pytest.mark.parametrize("lag", [0, 3])
def test_the_incremental_chain_is_stitch_trajectory_to_the_bit(lag):
    """997 random windows on two lanes, one window at a time (pose_vec2mat, np.linalg.inv and np.dot per window) against
    stitch_trajectory on each lane's whole pose array: the same float64 matrices, bit for bit"""
    rng = np.random.default_rng(20261021)
    n, lanes = 997, 2
    poses = rng.standard_normal((n, lanes, 2, 6)).astype(np.float32) * np.float32(0.2)
    poses[5, 0, 1, :3] = 4.0                               # past pi: euler2mat clips
    fake = FakeEngine(poses, lanes, lag)
    tr = davo_amd.Tracker(fake, lanes)
    seen = 0
    for t in range(n + 2):
        got = tr.push(None, None, None)
        assert len(got) == max(0, t - 1 - lag) >= seen
        seen = len(got)
        assert len(tr.trajectory(1)) == (seen + 2 if seen else 1)
    tr.close()
    assert fake.ended and len(tr.poses) == n
    for lane in range(lanes):
        ref = S.stitch_trajectory(poses[:, lane])
        traj = tr.trajectory(lane)
        assert len(traj) == len(ref) == n + 2
        for a, b in zip(traj, ref):
            assert a.dtype == b.dtype == np.float64 and np.array_equal(a.view(np.uint64), b.view(np.uint64))
        assert np.array_equal(tr.pose(lane), ref[-1])
    assert np.array_equal(np.stack(tr.poses), poses)


# ---- the per-push helper ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True])
def test_pushes_round_trip_against_the_window_layout(depth):
    H, W, n = 16, 20, 7
    fr = synth.make_frames(n, H, W, depth=depth)
    win = davo_amd.windows_from_frames(*fr)
    pushes = F.track_pushes(*fr)
    assert len(pushes) == n
    for t, p in enumerate(pushes):
        assert p[0].shape == (1, H, W, 3) and p[2].shape == (1, H, W, 1) and (p[1] is None) == (t < 2)
        assert (p[3] is None) == (not depth)
    # put back together: the frame arrays, and through windows_from_frames the window batch
    back = (np.concatenate([p[0] for p in pushes]), np.concatenate([p[1] for p in pushes[2:]]), np.concatenate([p[2] for p in pushes]))
    if depth:
        back += (np.concatenate([p[3] for p in pushes]),)
    for a, b in zip(back, fr):
        assert np.array_equal(a, b)
    for a, b in zip(davo_amd.windows_from_frames(*back), win):
        assert np.array_equal(a, b)
    # from the window batch: the same pushes; window t - 2 of the batch is what push t completes
    for p, q in zip(F.track_pushes_from_windows(*win), pushes):
        for a, b in zip(p, q):
            assert (a is None and b is None) or np.array_equal(a, b)
    for t in range(2, n):
        w = davo_amd.windows_from_frames(*(np.concatenate([pushes[u][k] for u in (range(t - 2, t + 1) if k != 1 else [t])])
                                           for k in range(4 if depth else 3)))
        for a, b in zip(w, win):
            assert np.array_equal(a[0], b[t - 2])
    bad = [a.copy() for a in win]
    bad[0][3, 0, 0, 0] ^= 1                                # windows that are not consecutive are named, not pushed
    with pytest.raises(ValueError, match="window"):
        F.track_pushes_from_windows(*bad)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------
def test_online_flag():
    from davo_amd import run_kitti_pose as G
    ap = G.build_parser()
    assert ap.parse_args(["--output_dir", "o"]).online is False
    a = ap.parse_args(["--output_dir", "o", "--online", "--labels", "u8", "--flow", "f16", "--depth", "f16", "--flip"])
    assert a.online and a.flip and (a.labels, a.flow, a.depth) == ("u8", "f16", "f16")
    G.check_online(ap, a)                                  # accepted
    for extra in (["--gpus", "2"], ["--batch_size", "4"], ["--synthetic", "12"], ["--sync_driver"]):
        with pytest.raises(SystemExit) as exc:
            G.main(["--output_dir", "o", "--online", "--concat_img_dir", "nowhere"] + extra)
        assert exc.value.code == 2, extra


def test_online_gpus_2_is_refused_with_a_message(capsys):
    from davo_amd import run_kitti_pose as G
    with pytest.raises(SystemExit):
        G.main(["--output_dir", "o", "--online", "--gpus", "2", "--concat_img_dir", "nowhere"])
    assert "one GPU" in capsys.readouterr().err
