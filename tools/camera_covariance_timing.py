"""Times hs_compute_covariance with free camera blocks (hs_set_camera_covariance) on the two windows of
tools/covariance_timing.py: configs[1] (128 control points, 5k landmarks, frozen prefix) with 22 camera columns (camera 1 fully free,
camera 0's intrinsics and distortion), and the replay-shaped window with an IMU (40 control points) with T_bs of camera 0 free. `constant`
leaves every camera block constant and does not touch the switch (the numbers to compare with; it also runs on a library that predates the
switch). Wall time per call here; the per-kernel device split comes from one run per window and mode under rocprofv3 --kernel-trace --stats.
usage: python tools/camera_covariance_timing.py <configs1|replay> <constant|free> [repeats]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import hyperslam_amd as ha  # noqa: E402
from hyperslam_amd import synthetic  # noqa: E402

which, mode = sys.argv[1], sys.argv[2]
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20


def frozen(w):
    w.cp_constant = np.r_[np.ones(w.order, np.uint8), np.zeros(w.n_cp - w.order, np.uint8)]
    return w


def replay_imu():
    w = frozen(synthetic.small_inertial(order=4, n_cp=40, n_landmarks=150, obs_pairs=3, n_inertial=400))
    with ha.Problem(w) as p:  # (drop trailing bias control points no inertial row reaches: free coordinates without information)
        used = int(p.linearize(ha.HS_INERTIAL, True)["first_bias"].max()) + int(w.imu["bias_order"])
    w.imu["bias_g"], w.imu["bias_a"] = w.imu["bias_g"][:used], w.imu["bias_a"][:used]
    return w


if which == "configs1":
    w, free = frozen(synthetic.config1()), [[1, 0, 0], [0, 0, 0]]  # flags [T_bs, intrinsics, distortion] per camera, non-zero = constant
else:
    w, free = replay_imu(), [[0, 1, 1], [1, 1, 1]]
with ha.Problem(w) as p:
    if mode == "free":
        p.set_camera_constancy(np.array(free, np.uint8))
        p.set_camera_covariance(True)
    p.compute_covariance()
    t = time.perf_counter()
    for _ in range(reps):
        p.compute_covariance()
    dt = (time.perf_counter() - t) / reps
    print(f"{which} {mode}: n_cp {w.n_cp}, band {p.lib.band_blocks(p.h)} blocks, dim {p.dim_pose()}, {len(w.landmarks)} landmarks: "
          f"hs_compute_covariance {1e3 * dt:.3f} ms wall per call ({reps + 1} calls in all)", flush=True)
