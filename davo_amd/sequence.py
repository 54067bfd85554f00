"""Sequence driver around the pose path: window sharding across GPUs, the one pose gather,
and the trajectory stitch + KITTI writer that follow the path in the reference's test driver.

Reference: ``test_kitti_pose.py:75-154`` (driver; hot loop ``:133-145``, chain ``:147-149``,
writer ``:150-153``), ``utils/geo_utils.py:12-63,93-119`` (``euler2mat`` clips to [-pi,pi],
R = Rx.Ry.Rz; ``pose_vec2mat`` on ``[rz,ry,rx,tx,ty,tz]``), ``utils/common_utils.py:8-28``.

The windows of a sequence are independent (each ``[2,6]`` output depends only on its own
3 frames), so ranks take contiguous window ranges and run them with no data-path collective;
the only exchange is one all-gather of ``[n,2,6]`` float32 before the sequential 4x4 chain
(48 B per window: 218 KB for KITTI seq 00 — latency only, on RCCL over xGMI; davo_amd/comm.py).
"""
import os

import time

import numpy as np


# ---- geometry (utils/geo_utils.py) --------------------------------------------------------
def euler2mat(z, y, x, dtype=np.float32):
    """R = Rx(x).Ry(y).Rz(z) with angles clipped to [-pi,pi] (geo_utils.py:12-63).
    The reference evaluates this in a float32 TF graph (test_kitti_pose.py:122-123)."""
    z = np.clip(np.asarray(z, dtype), -np.pi, np.pi)
    y = np.clip(np.asarray(y, dtype), -np.pi, np.pi)
    x = np.clip(np.asarray(x, dtype), -np.pi, np.pi)
    n = z.shape[0]
    cz, sz, cy, sy, cx, sx = np.cos(z), np.sin(z), np.cos(y), np.sin(y), np.cos(x), np.sin(x)
    zmat = np.zeros((n, 3, 3), dtype); ymat = np.zeros((n, 3, 3), dtype); xmat = np.zeros((n, 3, 3), dtype)
    zmat[:, 0, 0] = cz; zmat[:, 0, 1] = -sz; zmat[:, 1, 0] = sz; zmat[:, 1, 1] = cz; zmat[:, 2, 2] = 1
    ymat[:, 0, 0] = cy; ymat[:, 0, 2] = sy; ymat[:, 1, 1] = 1; ymat[:, 2, 0] = -sy; ymat[:, 2, 2] = cy
    xmat[:, 0, 0] = 1; xmat[:, 1, 1] = cx; xmat[:, 1, 2] = -sx; xmat[:, 2, 1] = sx; xmat[:, 2, 2] = cx
    return np.matmul(np.matmul(xmat, ymat), zmat)


def pose_vec2mat(vec, dtype=np.float32):
    """[n,6] ``[rz,ry,rx,tx,ty,tz]`` -> [n,4,4] (geo_utils.py:93-119)."""
    vec = np.asarray(vec, dtype).reshape(-1, 6)
    n = vec.shape[0]
    m = np.zeros((n, 4, 4), dtype)
    m[:, :3, :3] = euler2mat(vec[:, 0], vec[:, 1], vec[:, 2], dtype)
    m[:, :3, 3] = vec[:, 3:6]
    m[:, 3, 3] = 1
    return m


def mat2pose_vec(m):
    """Inverse of pose_vec2mat for |ry| < pi/2 (float64): with R = Rx.Ry.Rz,
    R[0,2] = sin y, R[0,1] = -cos y sin z, R[1,2] = -sin x cos y."""
    m = np.asarray(m, np.float64).reshape(-1, 4, 4)
    y = np.arcsin(np.clip(m[:, 0, 2], -1.0, 1.0))
    z = np.arctan2(-m[:, 0, 1], m[:, 0, 0])
    x = np.arctan2(-m[:, 1, 2], m[:, 2, 2])
    return np.concatenate([np.stack([z, y, x], -1), m[:, :3, 3]], -1)


# ---- stitch + writer (test_kitti_pose.py:136-153) -----------------------------------------
def stitch_trajectory(poses, mat_dtype=np.float32):
    """poses [Nw,2,6] (row 0 = tgt->src0, row 1 = tgt->src1 of window w, tgt = frame w+1)
    -> list of Nw+2 float64 4x4 camera poses, first = identity.

    First window contributes T(tgt->src0); every window contributes inv(T(tgt->src1))
    (test_kitti_pose.py:141-145); the chain is float64 (``np.eye(4).astype(float)``, :118)."""
    poses = np.asarray(poses, np.float32)
    if poses.shape[0] == 0:
        return [np.eye(4).astype(float)]
    # all windows' matrices at once (the per-window form of :141-145 spent 19 us of interpreter time per window: 87 ms of a
    # 0.96 s KITTI seq-00 run); same float32 elementwise arithmetic and the same LAPACK inverse per matrix
    first = pose_vec2mat(poses[:1, 0], mat_dtype)[0]                               # :144
    steps = [first] + list(np.linalg.inv(pose_vec2mat(poses[:, 1], mat_dtype)))    # :142,145
    prev = np.eye(4).astype(float)
    out = [prev]
    for p in steps:                                                                # :147-149
        prev = np.dot(prev, p)
        out.append(prev)
    return out


def write_kitti_poses(path, mats):
    """first 3 rows, 12 x str(float) per line (test_kitti_pose.py:150-153)."""
    with open(path, "w") as f:
        for p in mats:
            f.write("%s\n" % " ".join([str(float(x)) for x in np.asarray(p)[:3, :].reshape(12)]))


def read_kitti_poses(path):
    a = np.loadtxt(path).reshape(-1, 3, 4)
    m = np.tile(np.eye(4), (a.shape[0], 1, 1))
    m[:, :3, :] = a
    return m


def relative_pose_vectors(abs_poses):
    """Ground-truth poses -> the [Nw,2,6] tensor a perfect network would emit, i.e. the inverse
    of stitch_trajectory: M(tgt->src0) = P_w^-1 P_{w+1}, M(tgt->src1) = P_{w+2}^-1 P_{w+1}."""
    P = np.asarray(abs_poses, np.float64)
    nw = P.shape[0] - 2
    out = np.zeros((nw, 2, 6))
    for w in range(nw):
        out[w, 0] = mat2pose_vec(np.linalg.inv(P[w]).dot(P[w + 1]))[0]
        out[w, 1] = mat2pose_vec(np.linalg.inv(P[w + 2]).dot(P[w + 1]))[0]
    return out


# ---- window sharding + gather --------------------------------------------------------------
def is_valid_sample(n_frames, tgt_idx, seq_length=3):
    """utils/common_utils.py:16-28 for a single drive."""
    off = int((seq_length - 1) / 2)
    return tgt_idx - off >= 0 and tgt_idx + off < n_frames


def shard_windows(n_windows, world, rank):
    """contiguous range of rank: [r*ceil(Nw/R), min((r+1)*ceil(Nw/R), Nw))"""
    per = -(-n_windows // world)
    lo = min(rank * per, n_windows)
    return lo, min(lo + per, n_windows)


def _pad_batch(img, flow, seg, batch_size):
    n = img.shape[0]
    if n < batch_size:
        pad = batch_size - n
        img = np.concatenate([img, np.repeat(img[-1:], pad, 0)])
        flow = np.concatenate([flow, np.repeat(flow[-1:], pad, 0)])
        seg = np.concatenate([seg, np.repeat(seg[-1:], pad, 0)])
    return img, flow, seg, n


def _pad_parts(parts, batch_size):
    """_pad_batch for a batch of three or four arrays (a depth-source variant's batches carry the depth planes)"""
    n = parts[0].shape[0]
    if n < batch_size:
        parts = tuple(np.concatenate([p, np.repeat(p[-1:], batch_size - n, 0)]) for p in parts)
    return tuple(parts), n


class PoseStream:
    """The library's streaming entry point (include/davo_hip.h: davo_submit / davo_wait) as run_shard's ``stream``: batches
    are issued without waiting for their poses, so the H2D copy and the kernels of batch n+1 run while batch n computes and
    while the loader is asked for batch n+2 - what tf.data's prefetch does for the reference's loop
    (test_kitti_pose.py:133-145, data_loader.py:321-324).  ``hold``: batches whose input arrays the source keeps valid after
    yielding the next one (0 for davo_amd.loader's loaders; arrays that are never recycled can take 8: no copy is waited for).
    ``inflight``: slots = streams the batches rotate through; a slot's stream runs copy -> kernels -> pose copy in order, so at
    batch 1 (44 us of copy latency in front of 127 us of kernels) more slots keep the GPU busier: 8.8 k windows/s with two, 10.6 k with
    three, 12.4 k with four (the library's maximum) on 799 windows; at batch 32 three are best (f16x3 from page-locked host memory:
    14.7 k / 23.1 k / 26.7 k / 22.6 k triplets/s with one to four slots - four forwards of 3,000-workgroup launches at once break up
    the launch plan's whole rounds; float32 8.9 k from two slots on = the HBM-resident rate).  Default: four up to batch 2, else three."""

    def __init__(self, engine, inflight=None, hold=0):
        self.engine, self.hold = engine, hold
        if inflight is None:            # measured: profiles/r05ac_config1_b1.json (batch 1), profiles/r05af_host_api.log (batch 32)
            inflight = 4 if engine.max_batch <= 2 else 3
        engine.set_inflight(inflight)

    def submit(self, img, flow, seg, out, depth=None, pairs=None):
        """``pairs`` ('both' | 'src0' | 'src1'; None = leave the engine's selection alone): the pairs this batch runs.  The switch
        goes through davo_set_pairs ahead of the submit, so by the ABI's ordering it applies to this batch and the later ones;
        the batches already in flight keep theirs."""
        if pairs is not None and pairs != self.engine.pairs:
            self.engine.set_pairs(pairs)
        self.engine.submit(img, flow, seg, out, self.hold, depth=depth)

    def submit_frames(self, frames, flow2, seg, out, depth=None, pairs=None):
        """submit on the frame layout (Engine.submit_frames; davo_amd/frames.py): each frame crosses the link once per batch."""
        if pairs is not None and pairs != self.engine.pairs:
            self.engine.set_pairs(pairs)
        self.engine.submit_frames(frames, flow2, seg, out, self.hold, depth=depth)

    def drain(self):
        self.engine.synchronize()


PAIRS_MODES = ("both", "trajectory")


def batch_pairs(mode, s):
    """The pair selection of the batch that starts at window ``s`` of its sequence.  'trajectory': stitch_trajectory reads
    row 0 of window 0 and row 1 of every window (test_kitti_pose.py:143-145), so the batch that contains window 0 - the first
    batch of the rank that owns it - runs both pairs and every other batch of every rank runs tgt->src1 alone; no batch
    boundary moves.  'both' -> None: the calls are made as they always were."""
    if mode not in PAIRS_MODES:
        raise ValueError("pairs must be one of %s, got %r" % (", ".join(PAIRS_MODES), mode))
    if mode == "both":
        return None
    return "both" if s == 0 else "src1"


def run_shard(infer_fn, load_windows, lo, hi, batch_size, timing=None, stream=None, pairs="both"):
    """Run windows [lo,hi) in batches; the last batch is padded by repeating its last window
    and the padded outputs are dropped (the reference's complete_batch_size,
    utils/common_utils.py:8-13, would append duplicate poses for B>1; parity is defined on
    B=1 semantics).

    ``stream`` (a PoseStream) replaces ``infer_fn``: batches are submitted and their poses collected at the end, so input
    wait, copies and kernels overlap instead of adding up; the poses are the same bits (same kernels on the same batches).

    A depth-source variant's batches are ``(img, flow, seg, depth)``: ``infer_fn`` then takes four arrays and ``stream.submit``
    gets ``depth=``; every other variant sees the three-array calls it always did.

    ``pairs``: 'both' (default) or 'trajectory' (batch_pairs).  With 'trajectory' every call carries the batch's selection as
    ``pairs='both' | 'src1'`` - to ``infer_fn`` and to ``stream.submit`` alike; the rows a batch did not select come back as
    exact zeros, which stitch_trajectory never reads.  With 'both' no call gets the argument.

    ``load_windows`` is either a callable ``(s, e) -> (img, flow, seg)`` or an iterable of
    ``(s, e, (img, flow, seg))`` in window order (davo_amd.loader.ThreadedWindowLoader: the next
    batches are decoded while this one is on the GPU).  ``timing`` (a dict) receives the seconds spent waiting for
    input and inside ``infer_fn``."""
    batch_pairs(pairs, lo)                                # an unknown mode fails before anything is loaded
    out = np.zeros((hi - lo, 2, 6), np.float32)
    tails = []                                            # streamed partial batches: (padded poses, where they go)
    if callable(load_windows):
        batches = ((s, min(s + batch_size, hi), load_windows(s, min(s + batch_size, hi))) for s in range(lo, hi, batch_size))
    else:
        batches = iter(load_windows)
    t_load = t_fwd = 0.0
    while True:
        t0 = time.perf_counter()
        item = next(batches, None)                       # with a prefetching loader: the time the GPU side WAITED for input
        t1 = time.perf_counter()
        t_load += t1 - t0
        if item is None:
            break
        s, e, parts = item
        parts, n = _pad_parts(parts, batch_size)
        extra = {"depth": parts[3]} if len(parts) == 4 else {}
        sel = batch_pairs(pairs, s)
        if sel is not None:
            extra["pairs"] = sel
        if stream is None:
            out[s - lo:e - lo] = np.asarray(infer_fn(*parts, **({"pairs": sel} if sel is not None else {})))[:n]
        elif n == batch_size:
            stream.submit(*parts[:3], out[s - lo:e - lo], **extra)     # delivered straight into its rows of `out`
        else:
            full = np.empty((batch_size, 2, 6), np.float32)
            stream.submit(*parts[:3], full, **extra)
            tails.append((full, s - lo, n, parts))                      # the padded copies stay alive until the drain
        t_fwd += time.perf_counter() - t1
    if stream is not None:
        t1 = time.perf_counter()
        stream.drain()
        for full, at, n, _ in tails:
            out[at:at + n] = full[:n]
        t_drain = time.perf_counter() - t1
    if timing is not None:
        timing["load_wait_s"] = timing.get("load_wait_s", 0.0) + t_load
        # synchronous driver: H2D copies + kernels + D2H of the poses (davo_forward).  Streamed: the time inside davo_submit - issuing
        # the batch and waiting for ITS H2D copy, while the previous batches compute - and drain_s, the wait for the last batches
        timing["forward_s"] = timing.get("forward_s", 0.0) + t_fwd
        if stream is not None:
            timing["drain_s"] = timing.get("drain_s", 0.0) + t_drain
            timing["streamed"] = True
    return out


def gather_poses(local, n_windows, world, rank, comm=None):
    """All ranks -> [Nw,2,6] on every rank: one all-gather of equal padded counts.

    ``comm`` is the run's communicator: ``davo_amd.comm.RcclComm`` (librccl through the C ABI,
    include/davo_hip.h: davo_allgather_poses) in the product; anything with the same
    ``allgather(local, n_per_rank) -> (all, ms)`` in the CPU tests of the sharding logic."""
    if world == 1 and comm is None:
        return np.asarray(local, np.float32)
    if comm is None:
        raise ValueError("world size %d needs a communicator (davo_amd.comm.RcclComm)" % world)
    per = -(-n_windows // world)
    full, _ = comm.allgather(np.ascontiguousarray(local, np.float32), per)
    # rank r's slot holds its hi-lo windows first; slots are in rank order = window order
    parts = []
    for r in range(world):
        lo, hi = shard_windows(n_windows, world, r)
        parts.append(full[r * per:r * per + (hi - lo)])
    return np.concatenate(parts, 0)


def run_sequence(infer_fn, load_windows, n_frames, batch_size, rank=0, world=1, comm=None, timing=None, emulate=None, stream=None,
                 pairs="both"):
    """The driver loop of test_kitti_pose.py:133-149, sharded: returns the Nf 4x4 poses on
    every rank (the stitch is cheap and sequential; rank 0 writes the file).  ``timing`` (a dict) receives this
    rank's seconds per stage: load_wait_s, forward_s, gather_s, stitch_s.

    ``emulate=(r, R)`` (measurement aid, one process): do exactly what rank r of R would do - its window shard, the gather
    (through ``comm`` at its real world size, normally 1), the stitch of the whole sequence - with the other ranks' windows left
    at zero motion.  ``stream`` (a PoseStream): the shard runs through the library's streaming entry point (run_shard).
    ``pairs='trajectory'``: only the pairs the stitch reads are run (batch_pairs); the trajectory is the both-pairs one bit for
    bit, and the returned ``poses`` hold zeros in the rows that were not run."""
    n_windows = n_frames - 2
    lo, hi = shard_windows(n_windows, *((world, rank) if emulate is None else (emulate[1], emulate[0])))
    if hasattr(load_windows, "for_range"):               # a loader factory: build this rank's prefetching loader
        load_windows = load_windows.for_range(lo, hi, batch_size)
    local = run_shard(infer_fn, load_windows, lo, hi, batch_size, timing, stream, pairs)
    t0 = time.perf_counter()
    if emulate is None:
        poses = gather_poses(local, n_windows, world, rank, comm)
    else:
        poses = np.zeros((n_windows, 2, 6), np.float32)
        poses[lo:hi] = gather_poses(local, hi - lo, world, rank, comm)
    t1 = time.perf_counter()
    traj = stitch_trajectory(poses)
    if timing is not None:
        timing.update(gather_s=t1 - t0, stitch_s=time.perf_counter() - t1, windows_this_rank=hi - lo)
    return traj, poses


def run_frames(engine_or_stream, load_frames, n_frames, batch_size, pairs="both"):
    """run_sequence for a caller that holds frames, not windows (include/davo_hip.h "Frame sequences"): the n_frames - 2 windows
    of a sequence in batches of ``batch_size`` through the frame-layout entry points - ``Engine.forward_frames``, or a PoseStream's
    ``submit_frames`` (batches then overlap, and are drained at the end).  ``load_frames(lo, hi)`` returns the frames [lo, hi + 2)
    and the flow of the windows [lo, hi): ``(frames, flow2, seg)``, or ``(frames, flow2, seg, depth)`` for a depth-source variant;
    with a stream the arrays stay valid as its ``hold`` says.  A short last batch is issued short - nothing is padded.
    ``pairs``: 'both' or 'trajectory' (batch_pairs: the batch with window 0 runs both pairs, every other one tgt->src1 alone; the
    engine is left on the last batch's selection).  Returns ``(traj, poses)`` like run_sequence."""
    n_windows = n_frames - 2
    batch_pairs(pairs, 0)                                 # an unknown mode fails before anything is loaded
    streamed = hasattr(engine_or_stream, "drain")
    poses = np.zeros((max(n_windows, 0), 2, 6), np.float32)
    for lo in range(0, n_windows, batch_size):
        hi = min(lo + batch_size, n_windows)
        parts = tuple(load_frames(lo, hi))
        extra = {"depth": parts[3]} if len(parts) == 4 else {}
        sel = batch_pairs(pairs, lo)
        if streamed:
            if sel is not None:
                extra["pairs"] = sel
            engine_or_stream.submit_frames(*parts[:3], poses[lo:hi], **extra)      # delivered straight into its rows
        else:
            if sel is not None and engine_or_stream.pairs != sel:
                engine_or_stream.set_pairs(sel)
            poses[lo:hi] = engine_or_stream.forward_frames(*parts[:3], **extra)
    if streamed:
        engine_or_stream.drain()
    return stitch_trajectory(poses), poses


# ---- several sequences in one launch (run_inference.sh and kitti_benchmark/pose_kitti_eval.sh:28-37 loop over 00-10) ------
def parse_seq_list(text):
    """``--test_seq``: comma-separated sequence numbers and inclusive ranges, "0,2,5-7" -> [0, 2, 5, 6, 7].  The order is kept
    as given; an empty item, a reversed range, a negative number or a sequence named twice is a ValueError."""
    out = []
    for item in str(text).split(","):
        item = item.strip()
        lo, dash, hi = item.partition("-")
        if not lo.strip().isdigit() or (dash and not hi.strip().isdigit()):
            raise ValueError("sequence list `%s': `%s' is neither a sequence number nor a range a-b" % (text, item))
        lo, hi = int(lo), int(hi) if dash else int(lo)
        if hi < lo:
            raise ValueError("sequence list `%s': the range `%s' runs backwards" % (text, item))
        for q in range(lo, hi + 1):
            if q in out:
                raise ValueError("sequence list `%s': sequence %d is named twice" % (text, q))
            out.append(q)
    return out


def parse_frame_counts(text, n_sequences):
    """``--synthetic``: one frame count for every sequence, or a comma list with one count per sequence -> [n_frames, ...]"""
    items = [x.strip() for x in str(text).split(",")]
    if not all(x.isdigit() for x in items):
        raise ValueError("frame counts `%s': not a list of whole numbers" % text)
    counts = [int(x) for x in items]
    if len(counts) == 1:
        counts *= n_sequences
    if len(counts) != n_sequences:
        raise ValueError("frame counts `%s': %d counts for %d sequences" % (text, len(counts), n_sequences))
    return counts


class SequenceError(RuntimeError):
    """A sequence of a several-sequence run failed; ``seq`` is its number, ``__cause__`` what went wrong."""

    def __init__(self, seq, cause):
        super().__init__("sequence %.2d failed: %s: %s" % (seq, type(cause).__name__, cause))
        self.seq = seq


def run_sequences(infer_fn, sequences, source, batch_size, rank=0, world=1, comm=None, emulate=None, stream=None,
                  before_sequence=None, pairs="both"):
    """run_sequence over several sequences, one after another, on one engine, one communicator and one stream: a generator of
    ``(seq, traj, poses, timing)`` per sequence, in the order of ``sequences`` = [(seq, n_frames), ...].  Every sequence is
    sharded over the ranks on its own (shard_windows(n_frames - 2, world, rank); a rank whose shard of a short sequence is empty
    still takes part in its gather) and batched on its own: no batch straddles two sequences, and a sequence's batches - hence
    its launch plans and its bits - are those of a run of that sequence alone.  A streamed run drains at every sequence's end:
    the gather needs the poses.  ``timing`` is that sequence's own dict, as run_sequence fills it.  ``pairs`` is run_sequence's: with 'trajectory' the both-pairs
    batch repeats at every sequence's first batch.

    ``source(k, seq, n_frames, lo, hi)`` gives the k-th sequence's ``load_windows`` for this rank's shard [lo, hi) - anything
    run_sequence takes; it is asked when the sequence's turn comes.  ``before_sequence(k, seq, n_frames, load_windows)`` runs in
    front of each sequence (the product resets the range state and calibrates there) and may return a ``load_windows`` to use
    instead - one it has taken the first batch from and put it back, say.

    The caller consumes a sequence's result (writes its file) before asking for the next one, so what it does in between runs
    while the loader's workers are already decoding the next sequence.  If a sequence fails, the stream is drained first - nothing
    is delivered later into arrays that are gone - and a SequenceError naming it is raised from the failure; sequences already
    yielded stay as they are.  Closing the loader and the communicator is the caller's."""
    for k, (seq, n_frames) in enumerate(sequences):
        timing = {}
        try:
            lo, hi = shard_windows(n_frames - 2, *((world, rank) if emulate is None else (emulate[1], emulate[0])))
            load = source(k, seq, n_frames, lo, hi)
            if before_sequence is not None:
                replaced = before_sequence(k, seq, n_frames, load)
                load = load if replaced is None else replaced
            traj, poses = run_sequence(infer_fn, load, n_frames, batch_size, rank, world, comm, timing, emulate, stream, pairs)
        except Exception as exc:
            if stream is not None:
                try:
                    stream.drain()                        # the failed shard's output array is still alive here (the traceback holds it)
                except Exception:                         # noqa: BLE001 - the first failure is the one to report
                    pass
            raise SequenceError(seq, exc) from exc
        yield seq, traj, poses, timing


# ---- on-disk inputs (data_loader.py:241-325; doc/preprocessing.md:50-114) -------------------
class kitti_window_loader:
    """Loader factory over the reference's dump (davo_amd/loader.py): ``for_range(lo, hi, B)`` gives the
    threaded, prefetching batch iterator of a rank's shard; calling it ``(s, e)`` loads one batch inline."""

    def __init__(self, concat_img_dir, seq, n_frames, H, W, workers=4, prefetch=2, alloc=None, decode_procs=0, procs=0,
                 pin=None, unpin=None, seg_planes=None, hold=0, depth=False, labels="f32", flow="f32"):
        self.depth = depth        # a depth-source variant: batches are (img, flow, seg, depth); "f16" (instead of True): float16 depth batches
        self.labels = labels      # "u8": every loader below yields uint8 label batches (davo_amd/loader.py)
        self.flow = flow          # "f16": every loader below yields float16 flow batches (davo_amd/loader.py)
        self.dir, self.seq, self.n_frames, self.H, self.W = concat_img_dir, seq, n_frames, H, W
        self.workers, self.prefetch, self.alloc, self.decode_procs = workers, prefetch, alloc, decode_procs
        self.procs, self.pin, self.unpin, self.seg_planes = procs, pin, unpin, seg_planes
        self.hold = hold          # batches the process loader keeps valid beyond the one being asked for (PoseStream(hold=...)); the threaded loader gives 0

    def prestart(self, lo, hi, batch_size):
        """Build this rank's process loader now and let it start filling batches: the workers fork, attach the buffers and
        decode the first batches behind the caller's GPU set-up instead of in front of the first batch.  for_range hands it out."""
        if self.procs > 0:
            ld = self.for_range(lo, hi, batch_size)
            if hasattr(ld, "start"):
                self._early = ((lo, hi, batch_size), ld.start())

    def for_range(self, lo, hi, batch_size):
        from . import loader as L
        early = getattr(self, "_early", None)
        if early is not None and early[0] == (lo, hi, batch_size):
            self._early = None
            return early[1]
        if self.procs > 0:      # worker processes fill shared (page-locked) batch buffers: davo_amd/loader.py, ProcessWindowLoader
            try:
                return L.ProcessWindowLoader(self.dir, self.seq, self.H, self.W, lo, hi, batch_size, self.procs, self.prefetch,
                                             pin=self.pin, unpin=self.unpin, hold=self.hold, depth=self.depth, labels=self.labels, flow=self.flow,
                                             seg_planes=L.SEG_PLANES_SOURCES if self.seg_planes is None else self.seg_planes)
            except L.ShmBudgetError as e:      # e.g. a container with the usual 64 MB /dev/shm: decode threads into pinned buffers instead
                import sys
                print("davo_amd: %s - falling back to the threaded loader" % e, file=sys.stderr)
        return L.kitti_loader(self.dir, self.seq, self.H, self.W, lo, hi, batch_size, self.workers, self.prefetch, self.alloc, self.decode_procs,
                              depth=self.depth, labels=self.labels, flow=self.flow)

    def __call__(self, s, e):
        return self.load_inline(self.seq, s, e)

    def load_inline(self, seq, s, e):
        """windows [s, e) of sequence ``seq``, loaded in this process"""
        from .loader import load_window
        parts = [load_window(self.dir, seq, w + 1, self.H, self.W, self.depth, self.labels, self.flow) for w in range(s, e)]
        return tuple(np.stack([p[k] for p in parts]) for k in range(4 if self.depth else 3))

    # several sequences from one worker pool (``seq`` and ``n_frames`` of the constructor are not used by these)
    def prestart_segments(self, segments, batch_size):
        """prestart for a run over several sequences: ``segments`` = [(seq, lo, hi), ...], this rank's shard of every sequence
        in the order they will run.  ONE process loader serves them all (davo_amd/loader.py: ProcessWindowLoader(segments=...)):
        its workers fork, its buffers are created and page-locked once, and it decodes sequence k+1 behind sequence k's tail.
        for_segment hands the segments out."""
        if self.procs > 0 and getattr(self, "_multi", None) is None:
            from . import loader as L
            try:
                ld = L.ProcessWindowLoader(self.dir, None, self.H, self.W, None, None, batch_size, self.procs, self.prefetch,
                                           pin=self.pin, unpin=self.unpin, hold=self.hold, depth=self.depth, segments=segments, labels=self.labels, flow=self.flow,
                                           seg_planes=L.SEG_PLANES_SOURCES if self.seg_planes is None else self.seg_planes)
                self._multi = ((list(segments), batch_size), ld.start())
            except L.ShmBudgetError as e:      # as for_range: the threaded loader, built per sequence
                import sys
                print("davo_amd: %s - falling back to the threaded loader" % e, file=sys.stderr)
                self._multi = ((list(segments), batch_size), None)

    @property
    def segment_loader(self):
        """the process loader that serves the segments (None: the threaded loader is built per sequence)"""
        return (getattr(self, "_multi", None) or (None, None))[1]

    def for_segment(self, k, segments, batch_size):
        """The batch iterator of segment k of ``segments`` (see prestart_segments, which this calls if nobody has): the process
        loader's ``segment(k)``, or - ``procs`` = 0, or /dev/shm too small - a threaded loader for that segment alone."""
        self.prestart_segments(segments, batch_size)
        multi = getattr(self, "_multi", None)
        if multi is not None and multi[0] != (list(segments), batch_size):
            raise ValueError("for_segment: not the segments the loader was started with")
        if multi is not None and multi[1] is not None:
            return multi[1].segment(k)
        from . import loader as L
        seq, lo, hi = segments[k]
        return L.kitti_loader(self.dir, seq, self.H, self.W, lo, hi, batch_size, self.workers, self.prefetch, self.alloc, self.decode_procs,
                              depth=self.depth, labels=self.labels, flow=self.flow)

    def close(self):
        """stop and unmap the several-segment loader, if one was built"""
        multi, self._multi = getattr(self, "_multi", None), None
        if multi is not None and multi[1] is not None:
            multi[1].close()


def synthetic_window_loader(H, W, seed=None, depth=False, labels="f32", flow="f32"):
    from . import synth

    def load(s, e):
        parts = synth.make_inputs(e - s, H, W, seed=synth.SEED if seed is None else seed, first_window=s, labels=labels, flow=flow)
        if depth:
            parts += (synth.make_depth(e - s, H, W, seed=synth.SEED if seed is None else seed, first_window=s,
                                       fmt="f16" if depth == "f16" else "f32"),)
        return parts
    return load
