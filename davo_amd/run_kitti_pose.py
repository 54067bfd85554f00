"""Sequence inference driver — the counterpart of the reference's ``test_kitti_pose.py``
(flags ``:20-29``, main ``:75-154``): runs the pose path over a KITTI odometry sequence and
writes ``<seq>-pred_kitti_pose.txt``.

    python -m davo_amd.run_kitti_pose --test_seq 3 --concat_img_dir DUMP --ckpt_file W.npz \
        --output_dir out --version v1-...                    # one GPU
    python -m davo_amd.run_kitti_pose ... --batch_size 64 --gpus 8     # windows sharded over 8 GPUs
    python -m davo_amd.run_kitti_pose --test_seq 0-10 ...              # eleven sequences, one launch: one context, one
                                                                       # communicator, one loader pool; a file per sequence

With ``--gpus N`` the command starts N ranks of itself, one per GPU (davo_amd/launch.py; a launcher that
sets RANK / LOCAL_RANK / WORLD_SIZE itself, e.g. ``python -m torch.distributed.run``, works too); the ranks'
poses meet in one RCCL all-gather (davo_amd/comm.py) and rank 0 writes the trajectory.

``--ckpt_file`` is a TF V2 checkpoint as the reference's Saver wrote it (prefix, ``.index`` file or the
directory holding ``checkpoint``; davo_amd/tf_checkpoint.py reads it without TensorFlow) or an ``.npz``
keyed by the TF variable names (SURVEY table W); with
``--synthetic N`` the inputs and weights are the seeded synthetic ones (no KITTI dump or
checkpoint exists offline) and N is the frame count (801 = seq 03, 4541 = seq 00).
"""
import argparse
import os
import sys
import time

_T_IMPORT = time.time()          # before numpy and the package: the first mark of the start-up split (--report)

import numpy as np               # noqa: E402

from . import sequence as S              # noqa: E402
from .davo import DAVO                   # noqa: E402
from .version import FLAGSHIP_VERSION    # noqa: E402


_FIRST_MAIN = True


def _process_start_time():
    """wall-clock time this process was created: its age from /proc (start time in clock ticks since boot against the uptime, 10 ms
    resolution - btime in /proc/stat is whole seconds and put up to a second of error into round 5's first start-up splits)"""
    try:
        ticks = int(open("/proc/self/stat").read().rsplit(")", 1)[1].split()[19])
        uptime = float(open("/proc/uptime").read().split()[0])
        return time.time() - (uptime - ticks / os.sysconf("SC_CLK_TCK"))
    except (OSError, ValueError, IndexError):
        return None


def loader_seg_planes(cfg):
    """Label planes the window loader decodes: the source frames' only (its default, None), unless the variant masks the
    target frame by its own table (-segmask_all-static, the with-target class-table sources), which reads all three."""
    return (0, 1, 2) if cfg.tgt_attended else None


def check_checkpoint(path):
    """--ckpt_file names something that can be opened: an .npz, or a TF V2 checkpoint's prefix / .index file / directory (the
    file itself is read later, behind the GPU set-up).  Raises FileNotFoundError / ValueError with the path."""
    if not path:
        raise ValueError("--ckpt_file is required without --synthetic")
    if path.endswith(".npz"):
        if not os.path.isfile(path):
            raise FileNotFoundError("no checkpoint %s" % path)
        return
    from .tf_checkpoint import resolve_checkpoint
    index = resolve_checkpoint(path) + ".index"
    if not os.path.isfile(index):
        raise FileNotFoundError("no checkpoint %s (%s is missing)" % (path, index))


def sequences_to_run(a):
    """The run's sequences from the parsed flags, validated without touching a GPU: -> ([(seq, n_frames), ...], synthetic).
    Every <dump>/NN exists, every sequence has a window (three frames), the checkpoint is there; ValueError / FileNotFoundError
    name what is not."""
    seqs = S.parse_seq_list(a.test_seq)
    counts = S.parse_frame_counts(a.synthetic, len(seqs)) if a.synthetic is not None else [0]
    synthetic = any(counts)                                  # "--synthetic 0" is "not synthetic", as it has always been
    if not synthetic:
        if not a.concat_img_dir:
            raise ValueError("--concat_img_dir (or --synthetic N) is required")
        counts = []
        for q in seqs:
            d = os.path.join(a.concat_img_dir, "%.2d" % q)
            if not os.path.isdir(d):
                raise FileNotFoundError("sequence %.2d: no directory %s" % (q, d))
            counts.append(sum(1 for f in os.listdir(d) if f.endswith(".jpg")) + 2 * int((a.seq_length - 1) / 2))   # test_kitti_pose.py:81-82
        check_checkpoint(a.ckpt_file)
    for q, n in zip(seqs, counts):
        if n < 3:
            raise ValueError("sequence %.2d has %d frames: a window needs three" % (q, n))
    return list(zip(seqs, counts)), synthetic


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch_size", type=int, default=1)          # test_kitti_pose.py:21
    ap.add_argument("--img_height", type=int, default=128)
    ap.add_argument("--img_width", type=int, default=416)
    ap.add_argument("--seq_length", type=int, default=3)
    ap.add_argument("--test_seq", default="9",
                    help="a sequence number, or several for one launch: comma-separated numbers and inclusive ranges, e.g. 0,2,5-7 or "
                         "0-10.  They run one after another, in this order, on one GPU context, one communicator and one loader worker "
                         "pool; each gets its own NN-pred_kitti_pose.txt, byte for byte the file of a launch of its own")
    ap.add_argument("--concat_img_dir", default=None)
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--ckpt_file", default=None)
    ap.add_argument("--version", default=FLAGSHIP_VERSION)
    ap.add_argument("--synthetic", default=None,
                    help="frame count of a synthetic sequence: one count for every sequence of --test_seq, or a comma list with one per sequence")
    ap.add_argument("--gpus", type=int, default=1, help="GPUs of this node to shard the windows over (one rank per GPU)")
    ap.add_argument("--no_calibrate", action="store_true",
                    help="skip the activation-range calibration of the f16x3 arithmetic (include/davo_hip.h: davo_calibrate)")
    ap.add_argument("--loader_threads", type=int, default=4, help="decode/read threads of the input pipeline (as data_loader.py:283-288; more threads contend on the GIL)")
    ap.add_argument("--decode_procs", type=int, default=0,
                    help="(threaded loader) extra JPEG decode processes; 0 = decode in the loader threads")
    ap.add_argument("--loader_procs", type=int, default=-1,
                    help="worker processes that decode the strips and read the .npy planes straight into shared, page-locked batch "
                         "buffers (davo_amd/loader.py: ProcessWindowLoader).  -1 = this rank's CPU share minus two, at most 16; "
                         "0 = the threaded loader (--loader_threads)")
    ap.add_argument("--force_comm", action="store_true",
                    help="build the RCCL communicator and run the pose all-gather at world size 1 too (exercises the multi-GPU path on one GPU)")
    ap.add_argument("--emulate_shard", default=None, metavar="r/R",
                    help="measurement aid: do what rank r of R would do (its window shard, the gather, the whole stitch) in this one process")
    ap.add_argument("--report", default=None, help="write the run's time split (load wait / forward / gather / stitch / write) as JSON here")
    ap.add_argument("--calibrate_on_first_windows", action="store_true",
                    help="calibrate every rank on windows 0..7 of the sequence (loaded inline) instead of on its own first batch: the storage "
                         "scales, and so the trajectory's last bits, then do not depend on the number of GPUs")
    ap.add_argument("--sync_driver", action="store_true",
                    help="one synchronous davo_forward per batch (input wait + copy + kernels + pose copy add up) instead of the streaming "
                         "entry point (davo_submit: three batches in flight (four up to batch 2), copies and input wait overlapped with the kernels)")
    ap.add_argument("--pairs", choices=S.PAIRS_MODES, default="both",
                    help="both: every window runs tgt->src0 and tgt->src1, as the reference does.  trajectory: only what the trajectory "
                         "reads (test_kitti_pose.py:143-145) - both pairs for the batch that holds a sequence's window 0, tgt->src1 alone "
                         "for every other batch: half the arithmetic and 55 %% of the input bytes; the written file is the same")
    ap.add_argument("--labels", choices=("f32", "u8"), default="f32",
                    help="f32: the label maps cross the link as the reference's float32.  u8: as uint8 class ids (include/davo_hip.h: "
                         "davo_set_label_format) - a quarter of the label bytes in the loader's buffers, over the link and in the staging "
                         "sets; uint8 -seglabel.npy files are read as they are, float32 ones converted by the loader's workers "
                         "(davo_amd.labels_to_u8).  The written file is the same")
    ap.add_argument("--flow", choices=("f32", "f16"), default="f32",
                    help="f32: the optical flow crosses the link as float32.  f16: as IEEE binary16 (include/davo_hip.h: "
                         "davo_set_flow_format) - half the flow bytes in the loader's buffers, over the link and in the staging sets; "
                         "float16 -flownet2.npy files are read as they are, float32 ones rounded by the loader's workers "
                         "(davo_amd.flow_to_f16).  The written file is that of a float32 run on the rounded flow, to the byte")
    ap.add_argument("--flip", action="store_true",
                    help="run the left-right mirrored sequence: every window is mirrored on the device as it is staged (include/davo_hip.h: "
                         "davo_set_flip; the training loader's --data_flip rule, davo_amd.flip_windows) - for a flip-trained checkpoint, or "
                         "to evaluate against kitti_benchmark's poses-flip/NN-flip.txt.  The loaders deliver the dump as it is; the file "
                         "names written are the same NN-pred_kitti_pose.txt")
    ap.add_argument("--depth", choices=("f32", "f16"), default="f32",
                    help="f32: the depth planes of a depth-source version cross the link as float32.  f16: as IEEE binary16 "
                         "(include/davo_hip.h: davo_set_depth_format) - half the depth bytes in the loader's buffers, over the link and in "
                         "the staging sets; float16 -monodepth2_depth.npy files are read as they are, float32 ones rounded by the "
                         "loader's workers (davo_amd.depth_to_f16).  The written file is that of a float32 run on the rounded planes, "
                         "to the byte.  A version that reads no depth ignores the option's files")
    ap.add_argument("--online", action="store_true",
                    help="feed the dump one frame per push through a tracking session (include/davo_hip.h: davo_track_push; "
                         "davo_amd.Tracker, one lane): the library keeps the two frames before on the device and every frame crosses the "
                         "link once.  Runs what --batch_size 1 --pairs trajectory runs - window 0 both pairs, then tgt->src1 alone - and "
                         "writes its file, byte for byte; combines with --labels, --flow, --depth and --flip.  One GPU, a dump on disk")
    return ap


def check_online(ap, a):
    """--online's refusals, before anything is started"""
    if not a.online:
        return
    if a.gpus > 1:
        ap.error("--online --gpus %d: a tracking session runs on one GPU (multi-rank tracking is not built)" % a.gpus)
    if a.synthetic is not None and any(S.parse_frame_counts(a.synthetic, 1)):
        ap.error("--online --synthetic: the synthetic windows are drawn one by one and share no frames; write a dump of a frame "
                 "sequence (davo_amd.synth.make_frames, davo_amd.windows_from_frames) and run it with --concat_img_dir")
    if a.batch_size != 1:
        ap.error("--online pushes one frame at a time: --batch_size must be 1, got %d" % a.batch_size)
    if a.emulate_shard or a.force_comm or a.sync_driver:
        ap.error("--online does not combine with --emulate_shard, --force_comm or --sync_driver")


def main(argv=None):
    ap = build_parser()
    a = ap.parse_args(argv)
    check_online(ap, a)
    # start-up split (wall clock).  Only the first main() of a process can say what the process start cost
    global _FIRST_MAIN
    fresh, _FIRST_MAIN = _FIRST_MAIN, False
    marks = [("interpreter_up", _T_IMPORT), ("imports_done", time.time())] if fresh else [("main_entered", time.time())]

    def mark(name):
        marks.append((name, time.time()))

    # what is to run, checked before anything is started - ranks, loader workers, the GPU context: a missing <dump>/NN of the
    # eighth sequence is found now, not after the seven before it have run
    try:
        sequences, synthetic = sequences_to_run(a)
    except ValueError as exc:
        ap.error(str(exc))
    except FileNotFoundError as exc:
        raise SystemExit("davo_amd.run_kitti_pose: %s" % exc)
    from .version import parse_version
    if a.pairs != "both" and parse_version(a.version).posenn == "triplet":
        # one pass of the three-frame PoseNN yields both poses of a window: there is no single pair to leave out
        ap.error("--pairs %s: version `%s' is the three-frame PoseNN (`-dilatedPoseNN' without `-sharedNN'), whose one pass per window "
                 "yields both poses; it runs with --pairs both only" % (a.pairs, a.version))
    from .comm import RcclComm, world_from_env, preload_in_background
    rank, local_rank, world = world_from_env()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # the parent only starts the ranks and waits; it never touches a GPU
        from .launch import spawn_ranks
        raise SystemExit(spawn_ranks(["-m", "davo_amd.run_kitti_pose"] + list(sys.argv[1:] if argv is None else argv), a.gpus))
    if a.gpus > 1 and world != a.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (a.gpus, world))
    device_index = local_rank
    emulate = tuple(int(x) for x in a.emulate_shard.split("/")) if a.emulate_shard else None
    shard_of = lambda n_frames: S.shard_windows(n_frames - 2, *((world, rank) if emulate is None else (emulate[1], emulate[0])))   # noqa: E731
    need_comm = world > 1 or a.force_comm
    # Start-up is a rank's whole run on a sharded sequence (a 568-window shard is 0.1 s of work), so everything that does not depend
    # on each other starts at once: librccl loads on a thread of its own (573 MB to map: most of a second, needed only at the
    # gather), the input pipeline's workers fork and its buffers are created and page-locked on another, while this thread reads
    # the checkpoint and builds the GPU context.  (Round 4 did these one after the other: 2.9 s from process start to the first
    # batch in a fresh process, 1.7 s of it the communicator: profiles/r05b_config4_scene_streamed.json.)  All of it is paid once
    # per launch, however many sequences the launch runs.
    if need_comm:
        preload_in_background()
    import threading
    loader_thread = None
    gpu_ready = threading.Event()
    H, W = a.img_height, a.img_width
    load = weights = None
    from .version import parse_version
    needs_depth = parse_version(a.version).needs_depth           # a depth source: <dump>/SS/FFFFFF-monodepth2_depth.npy beside the other files
    if needs_depth and a.depth == "f16":
        needs_depth = "f16"                                       # the loaders' ``depth`` argument: float16 depth batches
    # this rank's shard of every sequence, in running order: the segments of the one loader
    segments = [(seq, ) + shard_of(n_frames) for seq, n_frames in sequences]
    if not synthetic:
        if a.online:
            a.loader_procs = 0                      # windows are read inline, one per push
        if a.loader_procs != 0:
            # the fork server the loader's workers come from starts importing numpy / Pillow now (davo_amd/loader.py: worker_context);
            # it is a spawned interpreter that never touches a GPU, and its 0.2 s of imports pass behind HIP's initialisation
            from .loader import warm_workers
            warm_workers()
        from .davo import pinned_empty, pin_array, unpin_array    # batches are decoded straight into page-locked memory
        procs = a.loader_procs
        if procs < 0:
            cores = len(os.sched_getaffinity(0))
            try:
                q, period = open("/sys/fs/cgroup/cpu.max").read().split()
                if q != "max":
                    cores = min(cores, max(1, int(int(q) / int(period))))
            except (OSError, ValueError):
                pass
            procs = max(1, min(16, cores - 2))
        tgt_planes = loader_seg_planes(parse_version(a.version))
        load = S.kitti_window_loader(a.concat_img_dir, sequences[0][0], sequences[0][1], H, W,
                                     alloc=lambda shape, dtype: pinned_empty(shape, dtype, device_index),
                                     workers=a.loader_threads, decode_procs=a.decode_procs, procs=procs,
                                     pin=lambda arr: (gpu_ready.wait(), pin_array(arr, device_index)), unpin=unpin_array,
                                     seg_planes=tgt_planes, hold=0 if a.sync_driver else 1, depth=needs_depth, labels=a.labels, flow=a.flow)
        # the loader's buffers are created and its workers start filling them on a thread of its own, before anything else: the
        # workers need no GPU.  Page-locking the buffers (1.4 GB at batch 64: 0.3 s) follows on the loader's own thread, entry by
        # entry, once the context below exists: HIP serialises hipHostRegister with the context's own allocations, and pinning
        # beside them made the context 0.25 s slower (profiles/r05an_config4_scene_shard_nocomm.json against r05ao).
        if not a.online:
            loader_thread = threading.Thread(target=load.prestart_segments, args=(segments, a.batch_size), name="davo-loader-start")
            loader_thread.start()
        # ... and the checkpoint is read and parsed (0.06-0.1 s of file and numpy work, no GPU) on a third
        from .tf_checkpoint import load_weights
        ckpt = {}

        def read_checkpoint():
            try:
                ckpt["weights"] = load_weights(a.ckpt_file)        # TF V2 checkpoint (prefix / .index / directory) or .npz
            except BaseException as exc:                           # noqa: BLE001 - re-raised by the main thread below
                ckpt["error"] = exc
        weights_thread = threading.Thread(target=read_checkpoint, name="davo-checkpoint-read")
        weights_thread.start()
    comm = None
    try:
        # the GPU context: the communicator's thread needs it, and HIP's own initialisation (0.2-0.4 s) is on every path
        from . import _lib
        try:
            _lib.lib()
            mark("library_loaded")
            system = DAVO(version=a.version, device=device_index)
            if a.labels == "u8":
                system.use_u8_labels()
            if a.flow == "f16":
                system.use_f16_flow()
            if a.depth == "f16":
                system.use_f16_depth()
            system.setup_inference(H, W, "davo", a.seq_length, a.batch_size, **({"flip": True} if a.flip else {}))
            mark("gpu_context_created")
        finally:
            gpu_ready.set()                        # also on failure: the loader's pinning thread must not wait for ever
        # the communicator is not needed before the gather: the id exchange and ncclCommInitRank (1.5-1.7 s, most of it inside HIP's
        # code-object loading, which other HIP calls queue behind) run on a second thread from here on (collective; fails loudly at the
        # gather, no other transport)
        comm = RcclComm.from_env_async(system.engine) if need_comm else None

        if synthetic:
            from . import synth
            load = S.synthetic_window_loader(H, W, depth=needs_depth, labels=a.labels, flow=a.flow)     # the same seeded windows whatever the sequence's number
            weights = synth.make_weights(a.version)
        else:
            weights_thread.join()
            if "error" in ckpt:
                raise ckpt["error"]
            weights = ckpt["weights"]
        mark("inputs_and_weights_ready")
        system.load_weights(weights)
        mark("weights_on_gpu")
        def infer(*parts, pairs=None):                 # (img, flow, seg[, depth]); pairs: the batch's selection under --pairs trajectory
            if pairs is not None and pairs != system.engine.pairs:
                system.engine.set_pairs(pairs)
            return system.inference(None, "pose", inputs=parts)["pose"]
        if loader_thread is not None:
            loader_thread.join()
            loader_thread = None
        mark("loader_started")
        # streamed: a batch of the process loader stays valid while the next one is asked for (hold = 1) - across a sequence boundary
        # too - so davo_submit does not wait for its own copy; the threaded loader and the synthetic windows give no such promise
        # (hold = 0).  One stream serves the whole run
        process_loader = not synthetic and load.segment_loader is not None
        stream = None if a.sync_driver or a.online else S.PoseStream(system.engine, hold=1 if process_loader else 0)
        if a.online:
            system.engine.set_inflight(4)       # the slots PoseStream gives a batch-1 run: the same launch plans
        clock = {}

        def source(k, seq, n_frames, lo, hi):
            # this rank's prefetching loader (started above) hands out the sequence's segment; it is closed only after the last
            # trajectory is written - unpinning and unmapping ~1 GB of batch buffers takes 0.15 s
            return load if synthetic else load.for_segment(k, segments, a.batch_size)

        def before_sequence(k, seq, n_frames, ld):
            """every sequence starts from a new context's range state and is calibrated as a launch of its own would calibrate it:
            its trajectory does not depend on the sequences before it"""
            if k:
                system.engine.reset_range_state()
            batches = None
            if not a.no_calibrate:
                lo, hi = shard_of(n_frames)
                if a.calibrate_on_first_windows or synthetic or not hasattr(ld, "__iter__") or lo >= hi:
                    # windows 0..7 of the sequence on every rank: the storage scales - and with them the trajectory's last bits - do not
                    # depend on the world size.  Loaded inline: Pillow's import and eight decodes in front of this rank's first batch
                    n8 = min(a.batch_size, 8, n_frames - 2)
                    system.calibrate(load(0, n8) if synthetic else load.load_inline(seq, 0, n8))
                else:
                    # the first eight windows of THIS rank's first batch, which its loader's workers are decoding anyway (round 5: the inline
                    # load was 0.35 s of a rank's 0.8 s start-up, most of it importing Pillow into this process).  The scales are exact
                    # powers of two with 64x headroom: ranks that calibrate on different windows agree to float32 rounding
                    # (test_calibration_is_neutral_for_a_well_ranged_checkpoint), not to the bit: --calibrate_on_first_windows restores that
                    import itertools
                    it = iter(ld)
                    first = next(it)
                    n8 = min(8, first[1] - first[0])
                    system.calibrate(tuple(x[:n8] for x in first[2]))
                    batches = itertools.chain([first], it)
            if k == 0:
                mark("calibrated_first_forward_done")
                clock["wall"] = time.perf_counter()            # "first batch ready": where the first sequence's wall_s starts
            clock["t0"] = time.perf_counter()
            clock["range"] = system.engine.range_stats()
            return batches

        entries = []
        if a.online:
            from .track import run_online
            results = run_online(system.engine, lambda seq, w: load.load_inline(seq, w, w + 1), sequences, before_sequence)
        else:
            results = S.run_sequences(infer, sequences, source, a.batch_size, rank, world, comm, emulate, stream, before_sequence, a.pairs)
        for seq, traj, poses, timing in results:
            dt = time.perf_counter() - clock["t0"]
            if rank != 0:
                continue
            n_windows = len(traj) - 2
            os.makedirs(a.output_dir, exist_ok=True)
            out = os.path.join(a.output_dir, "%.2d-pred_kitti_pose.txt" % seq)   # :116
            tw = time.perf_counter()
            S.write_kitti_poses(out, traj)
            now = time.perf_counter()
            timing["write_s"] = now - tw
            stats = system.engine.range_stats()
            timing.update(total_s=dt + timing["write_s"], windows=n_windows, windows_per_s=n_windows / dt,
                          range_recovery={key: stats[key] - clock["range"][key] for key in stats})     # this sequence's own
            entries.append(dict(timing, seq=seq, wall_s=now - clock["wall"]))   # from the previous trajectory written (or the first batch ready)
            clock["wall"] = now
            print("Done. Please check %s  (%d windows on %d GPU(s) in %.2f s incl. input generation/IO: input wait %.2f, forward %.2f, "
                  "gather %.3f, stitch %.2f, write %.2f%s)" % (out, n_windows, world, dt, timing["load_wait_s"], timing["forward_s"],
                                                               timing["gather_s"], timing["stitch_s"], timing["write_s"],
                                                               "; streamed: forward = time inside davo_submit, drain %.3f" % timing["drain_s"]
                                                               if "drain_s" in timing else ""))
        if rank == 0:
            t_proc = _process_start_time()
            names = [m[0] for m in marks]
            times = [m[1] for m in marks]
            startup = {"%s_s" % names[i]: times[i] - times[i - 1] for i in range(1, len(marks))}
            if t_proc is not None and fresh:
                startup["process_start_to_interpreter_up_s"] = times[0] - t_proc
                startup["process_start_to_first_batch_s"] = times[-1] - t_proc
            startup["first_batch_to_trajectory_written_s"] = time.time() - times[-1]       # several sequences: to the last one's
            if getattr(comm, "t_ready", None) is not None and t_proc is not None and fresh:
                startup["process_start_to_communicator_ready_s"] = comm.t_ready - t_proc      # built on a second thread; the gather waited for it
                startup["process_start_to_trajectory_written_s"] = time.time() - t_proc
            run_wide = dict(startup={k: round(v, 4) for k, v in startup.items()}, world=world, batch_size=a.batch_size,
                            note="rank 0's seconds; load_wait_s = time the GPU side waited for the input pipeline, forward_s = H2D + kernels + "
                                 "pose D2H inside DAVO.inference (streamed: the time inside davo_submit), gather_s = the RCCL all-gather incl. staging and the "
                                 "wait for the communicator, which is built on a second thread from the moment the GPU context exists")
            if a.pairs != "both":          # the default run's report is the one it has always been
                run_wide["pairs"] = a.pairs
            if a.labels != "f32":
                run_wide["labels"] = a.labels
            if a.flow != "f32":
                run_wide["flow"] = a.flow
            if a.depth != "f32":
                run_wide["depth"] = a.depth
            if a.flip:
                run_wide["flip"] = True
            if a.online:
                run_wide["online"] = True
            if len(entries) == 1:          # one sequence: the report it has always had
                report = {k: v for k, v in entries[0].items() if k not in ("seq", "wall_s")}
                report.update(run_wide)
            else:                          # several: the run's totals, and every sequence's own split under "sequences"
                report = dict(run_wide, windows=sum(e["windows"] for e in entries), total_s=sum(e["wall_s"] for e in entries),
                              sequences=entries)
                report["note"] += "; sequences[i].wall_s = from the previous trajectory written (the first batch ready, for the first) to " \
                                  "this one written, total_s = their sum; range_recovery = that sequence's own re-issues"
            if a.report:
                import json
                rounded = lambda d: {k: (round(v, 4) if isinstance(v, float) else v) for k, v in d.items()}      # noqa: E731
                if "sequences" in report:
                    report["sequences"] = [rounded(e) for e in report["sequences"]]
                with open(a.report, "w") as f:
                    json.dump(rounded(report), f)
    except BaseException:
        # a sequence failed (S.SequenceError names it; run_sequences has drained the stream) or the set-up did: the workers stop and
        # /dev/shm is cleaned, the communicator goes - without the barrier the other ranks may never reach.  Files written stay.
        if loader_thread is not None:
            loader_thread.join()
        if hasattr(load, "close"):
            load.close()
        if comm is not None:
            try:
                comm.close()
            except Exception:                  # noqa: BLE001 - the failure being raised is the one to report
                pass
        raise
    if hasattr(load, "close"):
        load.close()
    if comm is not None:
        comm.barrier()
        comm.close()


if __name__ == "__main__":
    main()
