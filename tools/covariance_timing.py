"""Times hs_compute_covariance on configs[1] (128 control points, 5k landmarks; the leading k control points held constant to fix
the gauge) and on a replay-shaped window with an IMU (40 control points, bias splines, gravity; frozen prefix). Wall time per call here; the
per-kernel device split comes from running it under rocprofv3 --kernel-trace --stats. usage: python tools/covariance_timing.py [repeats]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import hyperslam_amd as ha  # noqa: E402
from hyperslam_amd import synthetic  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def frozen(w):
    w.cp_constant = np.r_[np.ones(w.order, np.uint8), np.zeros(w.n_cp - w.order, np.uint8)]
    return w


def replay_imu():
    w = frozen(synthetic.small_inertial(order=4, n_cp=40, n_landmarks=150, obs_pairs=3, n_inertial=400))
    with ha.Problem(w) as p:  # (drop trailing bias control points no inertial row reaches: free coordinates without information)
        used = int(p.linearize(ha.HS_INERTIAL, True)["first_bias"].max()) + int(w.imu["bias_order"])
    w.imu["bias_g"], w.imu["bias_a"] = w.imu["bias_g"][:used], w.imu["bias_a"][:used]
    return w


for name, w in (("configs[1]", frozen(synthetic.config1())), ("replay-shaped + IMU", replay_imu())):
    with ha.Problem(w) as p:
        p.compute_covariance()
        t = time.perf_counter()
        for _ in range(reps):
            p.compute_covariance()
        dt = (time.perf_counter() - t) / reps
        print(f"{name}: n_cp {w.n_cp}, band {p.lib.band_blocks(p.h)} blocks, dim {p.dim_pose()}, {len(w.landmarks)} landmarks: "
              f"hs_compute_covariance {1e3 * dt:.3f} ms wall per call", flush=True)
