"""Online tracking on the host (include/davo_hip.h "Online tracking"): a thin wrapper over ``Engine.track_begin / track_push /
track_end`` that also keeps every lane's camera pose, chained the reference's way, and the driver of ``run_kitti_pose --online``.

The library keeps the last frames on the device and yields the poses of the window each new frame completes; the chain of 4x4
matrices stays here, where the reference's float32 ``pose_vec2mat`` and LAPACK inverse are reproduced (test_kitti_pose.py:141-149):
the first window contributes T(tgt->src0), every window inv(T(tgt->src1)), one window at a time - the matrices
``sequence.stitch_trajectory`` computes for the whole pose array at once, to the bit (tests/test_track.py keeps that true)."""
import collections
import time

import numpy as np

from . import sequence as S


class Tracker:
    """``lanes`` video streams in lockstep through one engine.  ``push`` takes one new frame per lane and returns the poses delivered
    so far; ``pose(lane)`` / ``trajectory(lane)`` are the lane's camera pose and path over the windows chained so far (float64 4x4,
    first = identity); ``close`` delivers and chains the rest and ends the session.  Pushes are streamed (Engine.track_push with
    ``hold``), so a window's poses arrive a push or more after the frame that completes it; ``flush`` waits for all of them.
    Other streamed submits on the same engine between pushes delay what ``push`` sees as delivered, nothing else."""

    def __init__(self, engine, lanes=1, policy="trajectory", hold=0):
        engine.track_begin(lanes, policy)
        self.engine, self.lanes, self.hold = engine, int(lanes), int(hold)
        self.poses = []                                           # [S,2,6] per delivered window, in window order
        self._issued = collections.deque()                        # pose arrays of the pushes not chained yet
        self._cam = [np.eye(4).astype(float) for _ in range(self.lanes)]           # test_kitti_pose.py:118
        self._traj = [[c] for c in self._cam]
        self._open = True

    def push(self, frames, flow2, seg, depth=None):
        """``frames`` u8 [S,H,W,3], ``flow2`` [S,2,H,W,2] (None for the first two frames), ``seg`` [S,H,W,1], ``depth`` [S,H,W,1]
        for a depth-source variant (Engine.track_push).  -> the list of [S,2,6] pose arrays delivered so far, one per window."""
        out = np.empty((self.lanes, 2, 6), np.float32)
        if self.engine.track_push(frames, flow2, seg, out, self.hold, depth=depth):
            self._issued.append(out)
        self._chain(len(self._issued) - self.engine.pending())
        return self.poses

    def _chain(self, n):
        """the oldest n issued windows have been delivered: their poses onto every lane's chain (test_kitti_pose.py:141-149)"""
        for _ in range(max(n, 0)):
            p = self._issued.popleft()
            for s in range(self.lanes):
                if not self.poses:                                                    # the session's first window: T(tgt->src0) too
                    self._step(s, S.pose_vec2mat(p[s:s + 1, 0])[0])                   # :144
                self._step(s, np.linalg.inv(S.pose_vec2mat(p[s:s + 1, 1]))[0])        # :142,145
            self.poses.append(p)

    def _step(self, lane, m):
        self._cam[lane] = np.dot(self._cam[lane], m)                                  # :147-149
        self._traj[lane].append(self._cam[lane])

    def flush(self):
        """wait for every push issued so far and chain it"""
        self.engine.wait()
        self._chain(len(self._issued))
        return self.poses

    def pose(self, lane=0):
        return self._cam[lane]

    def trajectory(self, lane=0):
        return list(self._traj[lane])

    def close(self):
        if self._open:
            self._open = False
            try:
                self.flush()
            finally:
                self.engine.track_end()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def run_online(engine, load_windows, sequences, before_sequence=None, hold=0):
    """``run_kitti_pose --online``: every sequence of ``sequences`` = [(seq, n_frames), ...] one frame per push through a Tracker
    of one lane under the trajectory policy - window 0 both pairs, every later window tgt->src1 alone, batch 1: the launches and
    the selection of ``--batch_size 1 --pairs trajectory``, hence its file.  ``load_windows(seq, w)`` gives window w of the dump,
    ``(img, flow, seg[, depth])`` with a leading axis of 1; window 0 yields three pushes, every later window one (its src1 frame),
    after its src0 and tgt have been checked against the two frames pushed before (a dump whose windows are not consecutive is a
    ValueError naming the window).  A generator of ``(seq, traj, poses, timing)`` like sequence.run_sequences."""
    from .frames import track_pushes_from_windows
    for k, (seq, n_frames) in enumerate(sequences):
        timing = {"load_wait_s": 0.0, "forward_s": 0.0, "gather_s": 0.0}
        try:
            if before_sequence is not None:
                before_sequence(k, seq, n_frames, None)
            tr = Tracker(engine, 1, "trajectory", hold)
            try:
                last = None                                               # the window before: its (tgt, src1) are this one's (src0, tgt)
                for w in range(n_frames - 2):
                    t0 = time.perf_counter()
                    parts = load_windows(seq, w)
                    pushes = track_pushes_from_windows(*parts)
                    if last is not None:
                        for j in (0, 1):                                   # (frame, no flow, label map, depth plane) of src0, then of tgt
                            for a, b in zip(last[j], pushes[j]):
                                if a is not None and not np.array_equal(a, b, equal_nan=a.dtype.kind == "f"):
                                    raise ValueError("window %d of sequence %.2d does not start with the last two frames of window %d: "
                                                     "the dump's windows are not consecutive windows of one video" % (w, seq, w - 1))
                    t1 = time.perf_counter()
                    for p in (pushes if last is None else pushes[2:]):
                        tr.push(*p)
                    last = [(p[0], None, p[2], p[3]) for p in pushes[1:]]
                    timing["load_wait_s"] += t1 - t0
                    timing["forward_s"] += time.perf_counter() - t1
                t1 = time.perf_counter()
                tr.close()
                timing["drain_s"] = time.perf_counter() - t1
                timing["streamed"] = True
            except BaseException:
                try:
                    tr.close()
                except Exception:                                          # noqa: BLE001 - the first failure is the one to report
                    pass
                raise
        except Exception as exc:
            raise S.SequenceError(seq, exc) from exc
        t1 = time.perf_counter()
        poses = np.concatenate([p for p in tr.poses]) if tr.poses else np.zeros((0, 2, 6), np.float32)
        traj = tr.trajectory(0)
        timing.update(stitch_s=time.perf_counter() - t1, windows_this_rank=n_frames - 2)
        yield seq, traj, poses, timing
