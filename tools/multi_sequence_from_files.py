#!/usr/bin/env python
"""Several sequences in one launch against one process per sequence ("Several sequences in one launch").

Three sequences of KITTI seq 00's shape (4541 frames -> 4539 windows of 128x416, batch 64, photograph-like strips; 640 distinct
windows on disk, the rest and the other two sequences are links to them: same decode work, warm page cache) run

  arm "one_launch":      python -m davo_amd.run_kitti_pose --test_seq 0,1,2 ...          one process
  arm "per_sequence":    python -m davo_amd.run_kitti_pose --test_seq N ...  for N in 0,1,2   three processes, from --baseline
                         (a checkout of the commit to compare against, its library built; default: this tree)

in alternating order, --rounds times after one unrecorded warm-up of each arm, in each of three set-ups: one GPU without a
communicator, with --force_comm, and as rank 0 of 8 (--emulate_shard 0/8 --force_comm: a 568-window shard per sequence).
Writes one JSON per arm and set-up into --out and prints the comparison: every sequence after the first of the one launch
(its wall_s: previous trajectory written -> this one written) against what the same sequence costs a process of its own from
its first batch on (first_batch_to_trajectory_written_s) and from the process's start.

    python tools/multi_sequence_from_files.py --out profiles [--baseline PATH] [--rounds 3] [--tag r06]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, REAL, H, W, B = 4541, 642, 128, 416, 64
SEQS = (0, 1, 2)


def write_dump(d):
    import numpy as np
    from davo_amd import loader as L, synth, parse_version, FLAGSHIP_VERSION
    L.write_synthetic_dump(d, 0, REAL, H, W, images="scene")
    for w in range(REAL - 2, N - 2):
        for src, dst in zip(L.window_paths(d, 0, (w % (REAL - 2)) + 1), L.window_paths(d, 0, w + 1)):
            os.symlink(src, dst)
    for seq in SEQS[1:]:
        os.makedirs(os.path.join(d, "%.2d" % seq))
        for w in range(N - 2):
            for src, dst in zip(L.window_paths(d, 0, (w % (REAL - 2)) + 1), L.window_paths(d, seq, w + 1)):
                os.symlink(src, dst)
    np.savez(os.path.join(d, "w.npz"), **synth.make_weights(parse_version(FLAGSHIP_VERSION)))


def launch(root, d, seqs, extra):
    """one process of run_kitti_pose from the tree at ``root`` -> (its report, the wall clock around the process)"""
    report = os.path.join(d, "report.json")
    cli = ["--concat_img_dir", d, "--ckpt_file", os.path.join(d, "w.npz"), "--output_dir", os.path.join(d, "out"), "--test_seq", seqs,
           "--batch_size", str(B), "--report", report] + extra
    t0 = time.perf_counter()
    subprocess.run([sys.executable, "-m", "davo_amd.run_kitti_pose"] + cli, cwd=root, check=True, stdout=subprocess.DEVNULL, timeout=300)
    wall = time.perf_counter() - t0
    r = json.load(open(report))
    r.pop("note", None)
    return r, round(wall, 3)


def one_launch(d):
    return lambda extra: dict(zip(("report", "process_wall_s"), launch(ROOT, d, ",".join(str(s) for s in SEQS), extra)))


def per_sequence(d, baseline):
    def arm(extra):
        t0 = time.perf_counter()
        runs = [dict(zip(("report", "process_wall_s"), launch(baseline, d, str(s), extra))) for s in SEQS]
        return {"processes": runs, "all_processes_wall_s": round(time.perf_counter() - t0, 3)}
    return arm


def median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--baseline", default=ROOT)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tag", default="multiseq")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    setups = (("nocomm", []), ("comm", ["--force_comm"]), ("shard0of8_comm", ["--emulate_shard", "0/8", "--force_comm"]))
    with tempfile.TemporaryDirectory(dir="/tmp") as d:
        t0 = time.perf_counter()
        write_dump(d)
        print("dump written in %.1f s" % (time.perf_counter() - t0), flush=True)
        arms = {"one_launch": one_launch(d), "per_sequence": per_sequence(d, os.path.abspath(a.baseline))}
        for name, extra in setups:
            rounds = {k: [] for k in arms}
            for k in arms:                                        # warm-up: page cache, the runtime's own caches
                arms[k](extra)
            for rnd in range(a.rounds):
                for k in (("one_launch", "per_sequence") if rnd % 2 == 0 else ("per_sequence", "one_launch")):
                    rounds[k].append(arms[k](extra))
            for k in arms:
                with open(os.path.join(a.out, "%s_%s_%s.json" % (a.tag, k, name)), "w") as f:
                    json.dump({"tool": "tools/multi_sequence_from_files.py", "setup": name, "arm": k, "flags": extra, "frames_per_sequence": N,
                               "batch_size": B, "sequences": list(SEQS), "rounds": rounds[k],
                               "baseline": "this tree" if os.path.abspath(a.baseline) == ROOT else "the commit compared against"}, f, indent=1)
            print("== %s" % name)
            for i, s in enumerate(SEQS):
                wall = [r["report"]["sequences"][i]["wall_s"] for r in rounds["one_launch"]]
                fb = [r["processes"][i]["report"]["startup"]["first_batch_to_trajectory_written_s"] for r in rounds["per_sequence"]]
                pw = [r["processes"][i]["process_wall_s"] for r in rounds["per_sequence"]]
                st = [r["processes"][i]["report"]["startup"].get("process_start_to_trajectory_written_s") for r in rounds["per_sequence"]]
                seq_split = rounds["one_launch"][-1]["report"]["sequences"][i]
                print("seq %.2d: one launch wall_s %s (median %.3f) | own process: first batch -> written %s (median %.3f), start -> written %s, "
                      "process wall %s | bound 1.1 x %.3f = %.3f: %s | last round's split: load_wait %.3f forward %.3f drain %.3f gather %.3f "
                      "stitch %.3f write %.3f" % (s, wall, median(wall), fb, median(fb), st, pw, median(fb), 1.1 * median(fb),
                                                  "first sequence (carries no bound)" if i == 0 else ("within" if median(wall) <= 1.1 * median(fb) else "EXCEEDED"),
                                                  seq_split["load_wait_s"], seq_split["forward_s"], seq_split.get("drain_s", 0.0), seq_split["gather_s"],
                                                  seq_split["stitch_s"], seq_split["write_s"]), flush=True)
            print("whole job: one launch %s s, three processes %s s" % ([r["process_wall_s"] for r in rounds["one_launch"]],
                                                                          [r["all_processes_wall_s"] for r in rounds["per_sequence"]]), flush=True)


if __name__ == "__main__":
    main()
