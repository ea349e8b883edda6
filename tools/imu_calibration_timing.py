"""Times the build of the reduced system with free IMU blocks (hs_set_imu_constancy / hs_reduced_system) on configs[2] and on a
replay-shaped stereo-inertial window (40 control points, 400 inertial rows), each with every IMU block constant (the launches of a handle
that never calls the entry point: the yardstick k_border_pb + k_border_bb is read off this run), with T_bs alone free and with all five blocks
free. Wall time per call here; the per-kernel device split comes from running ONE case under rocprofv3 --kernel-trace --stats.
usage: python tools/imu_calibration_timing.py [repeats] [window: configs2 | replay] [flags: constant | T_bs | all]   (default: every case)"""
import copy
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import hyperslam_amd as ha  # noqa: E402
from hyperslam_amd import synthetic  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
only_window = sys.argv[2] if len(sys.argv) > 2 else None
only_flags = sys.argv[3] if len(sys.argv) > 3 else None

FLAGS = {"constant": None, "T_bs": np.array([0, 1, 1, 1, 1], np.uint8), "all": np.zeros(5, np.uint8)}


def replay_shaped():
    w = synthetic.small_inertial(order=4, n_cp=40, n_landmarks=150, obs_pairs=3, n_inertial=400, seed=3)
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(36, np.uint8)]
    return w


for wname, make in (("configs2", synthetic.config2), ("replay", replay_shaped)):
    if only_window not in (None, wname):
        continue
    base = make()
    for fname, flags in FLAGS.items():
        if only_flags not in (None, fname):
            continue
        w = copy.copy(base)
        w.imu_constant = flags
        with ha.Problem(w) as p:
            p.reduced_system(1e4)
            t = time.perf_counter()
            for _ in range(reps):
                p.reduced_system(1e4)
            dt = (time.perf_counter() - t) / reps
            print(f"{wname} IMU blocks {fname}: dim {p.dim_pose()}: hs_reduced_system {1e3 * dt:.3f} ms wall per call (device build + copy-out to the host)",
                  flush=True)
