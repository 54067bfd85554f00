#!/usr/bin/env python
"""Generate tests/golden/kitti_eval/ from the REFERENCE's own KITTI devkit evaluator (kitti_benchmark/cpp/test_odometry_all.cpp).

Runs where the reference is present and its evaluator has been built into oracle/_ref/ (oracle/Makefile); only data travels:
for sequences 03, 04, 07 and 10 the ground truth and the ORB-SLAM2 stereo trajectories the reference ships (data fixtures,
gzipped, byte for byte), and what the compiled evaluator wrote for them (errors/SS.txt and SS-stats.txt).  tests/test_kitti_eval.py
checks the numpy restatement (davo_amd/kitti_eval.py) against those outputs.

    python tests/golden/make_kitti_eval_golden.py REFERENCE_DIR [EVALUATOR]      # rewrites tests/golden/kitti_eval/
"""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "kitti_eval")
SEQUENCES = (3, 4, 7, 10)


def write_gz(src, dst):
    with open(src, "rb") as f:
        data = f.read()
    with open(dst, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as g:
        g.write(data)


def main():
    ref = os.path.join(sys.argv[1], "kitti_benchmark", "data", "odometry")
    binary = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "oracle", "_ref", "test_odometry_all")
    work = tempfile.mkdtemp(prefix="kitti_eval_golden_")
    try:
        os.makedirs(os.path.join(work, "data", "odometry"))
        os.symlink(os.path.join(ref, "poses"), os.path.join(work, "data", "odometry", "poses"))
        res = os.path.join(work, "results", "orb")
        os.makedirs(os.path.join(res, "data"))
        for s in range(11):                                   # the evaluator walks sequences 00..10
            shutil.copy(os.path.join(ref, "poses_from_ORBSLAM2-S", "%02d-ORB-SLAM2-S.txt" % s), os.path.join(res, "data", "%02d.txt" % s))
        subprocess.run([binary, "orb"], cwd=work, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, check=False)
        os.makedirs(OUT, exist_ok=True)
        for s in SEQUENCES:
            write_gz(os.path.join(ref, "poses", "%02d.txt" % s), os.path.join(OUT, "gt_%02d.txt.gz" % s))
            write_gz(os.path.join(res, "data", "%02d.txt" % s), os.path.join(OUT, "orb_%02d.txt.gz" % s))
            shutil.copy(os.path.join(res, "errors", "%02d.txt" % s), os.path.join(OUT, "errors_%02d.txt" % s))
            shutil.copy(os.path.join(res, "%02d-stats.txt" % s), os.path.join(OUT, "stats_%02d.txt" % s))
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print("wrote", OUT)


if __name__ == "__main__":
    main()
