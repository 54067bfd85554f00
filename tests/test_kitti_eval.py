"""Row f4: the numpy restatement of the KITTI devkit evaluator vs the reference's own C++ program on trajectories the
reference ships (ORB-SLAM2 stereo results + ground truth).  What the compiled evaluator wrote for four sequences is stored
with its inputs under tests/golden/kitti_eval/ (tests/golden/make_kitti_eval_golden.py), so the check needs nothing
outside the repository."""
import os

import numpy as np

from davo_amd import kitti_eval as K
from davo_amd import sequence as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GT03 = os.path.join(ROOT, "tests", "golden", "kitti_gt_poses_03.txt")
EVAL_GOLDEN = os.path.join(ROOT, "tests", "golden", "kitti_eval")


def test_perfect_trajectory_has_zero_error():
    gt = K.load_poses(GT03)
    err = K.calc_sequence_errors(gt, gt.copy())
    assert err.shape[1] == 5 and err.shape[0] > 50
    assert np.all(err[:, 1] < 1e-3) and np.all(err[:, 2] < 1e-6)      # acos(1-eps) noise only
    assert set(err[:, 3]) <= set(float(x) for x in K.LENGTHS)
    # a stitched perfect prediction evaluates to ~0 drift: f1 (stitch) and f4 (evaluator) agree
    traj = np.array(S.stitch_trajectory(S.relative_pose_vectors(gt), mat_dtype=np.float64))
    err2 = K.calc_sequence_errors(np.linalg.inv(gt[0]) @ gt, traj)
    assert err2[:, 2].max() < 1e-5


def test_known_drift():
    gt = K.load_poses(GT03)
    res = gt.copy()
    res[:, :3, 3] *= 1.05                                              # 5 % scale error
    t_rel, r_rel = K.summary({"03": K.calc_sequence_errors(gt, res)})["03"]
    assert 4.5 < t_rel < 5.5 and r_rel < 1e-2


def test_matches_reference_evaluator():
    checked = 0
    for s in (3, 4, 7, 10):
        ref = np.loadtxt(os.path.join(EVAL_GOLDEN, "errors_%02d.txt" % s)).reshape(-1, 5)
        mine = K.calc_sequence_errors(K.load_poses(os.path.join(EVAL_GOLDEN, "gt_%02d.txt.gz" % s)),
                                      K.load_poses(os.path.join(EVAL_GOLDEN, "orb_%02d.txt.gz" % s)))
        assert mine.shape == ref.shape, (s, mine.shape, ref.shape)
        assert np.array_equal(mine[:, 0], ref[:, 0]) and np.array_equal(mine[:, 3], ref[:, 3])
        assert np.abs(mine[:, 1] - ref[:, 1]).max() < 2e-6          # the file is written with %f (6 decimals)
        assert np.abs(mine[:, 2] - ref[:, 2]).max() < 2e-6
        assert np.abs(mine[:, 4] - ref[:, 4]).max() < 1e-3
        stats = np.loadtxt(os.path.join(EVAL_GOLDEN, "stats_%02d.txt" % s))
        t_mean, r_mean = K.sequence_stats(mine)
        assert abs(stats[0] - t_mean) < 2e-6 and abs(stats[1] - r_mean) < 2e-6
        checked += 1
    assert checked >= 3
