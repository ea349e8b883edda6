"""Times hs_compute_covariance with free IMU blocks (hs_set_imu_covariance) on the replay-shaped window with an IMU of
tools/covariance_timing.py (40 control points, 44 bias / gravity unknowns): `t` frees T_bs (6 IMU columns), `tgas` frees T_bs, i_g, i_a and
S_g (27). `constant` leaves every IMU block constant and does not touch the switch (the numbers to compare with; it also runs on a library
that predates the switch). `sample` times hs_sample_sensor_covariance (IMU, T_bs free) and hs_sample_covariance at 64 stamps. Wall time per
call here; the per-kernel device split comes from one run per mode under rocprofv3 --kernel-trace --stats.
usage: python tools/imu_covariance_timing.py <constant|t|tgas|sample> [repeats]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import hyperslam_amd as ha  # noqa: E402
from hyperslam_amd import synthetic  # noqa: E402

mode = sys.argv[1]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
FREE = {"t": [0, 1, 1, 1, 1], "tgas": [0, 0, 0, 0, 1], "sample": [0, 1, 1, 1, 1]}  # flags [T_bs, i_g, i_a, S_g, X_a], non-zero = constant


def replay_imu():
    w = synthetic.small_inertial(order=4, n_cp=40, n_landmarks=150, obs_pairs=3, n_inertial=400)
    w.cp_constant = np.r_[np.ones(w.order, np.uint8), np.zeros(w.n_cp - w.order, np.uint8)]
    with ha.Problem(w) as p:  # (drop trailing bias control points no inertial row reaches: free coordinates without information)
        used = int(p.linearize(ha.HS_INERTIAL, True)["first_bias"].max()) + int(w.imu["bias_order"])
    w.imu["bias_g"], w.imu["bias_a"] = w.imu["bias_g"][:used], w.imu["bias_a"][:used]
    return w


w = replay_imu()
with ha.Problem(w) as p:
    if mode != "constant":
        p.set_imu_constancy(np.array(FREE[mode], np.uint8))
        p.set_imu_covariance(True)
    p.compute_covariance()
    head = f"replay {mode}: n_cp {w.n_cp}, band {p.lib.band_blocks(p.h)} blocks, dim {p.dim_pose()}, {len(w.landmarks)} landmarks: "
    if mode == "sample":
        lo, hi = w.valid_range()
        stamps = np.linspace(lo, hi, 66)[1:-1]
        for name, call in (("hs_sample_sensor_covariance (IMU)", lambda: p.sample_sensor_covariance(ha.HS_SENSOR_IMU, 0, stamps)),
                           ("hs_sample_covariance", lambda: p.sample_covariance(stamps))):
            call()
            t = time.perf_counter()
            for _ in range(reps):
                call()
            print(head + f"{name} at {len(stamps)} stamps {1e3 * (time.perf_counter() - t) / reps:.3f} ms wall per call ({reps + 1} calls in all)", flush=True)
    else:
        t = time.perf_counter()
        for _ in range(reps):
            p.compute_covariance()
        print(head + f"hs_compute_covariance {1e3 * (time.perf_counter() - t) / reps:.3f} ms wall per call ({reps + 1} calls in all)", flush=True)
