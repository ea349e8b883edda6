"""Times the build of the reduced system with free camera blocks (hs_reduced_system) on configs[1] with camera 1 fully free and
camera 0's intrinsics and distortion free (22 camera columns), and on configs[2] with camera 0's T_bs free, against the same windows with
every camera constant. Wall time per call here; the per-kernel device split comes from running it under rocprofv3 --kernel-trace --stats.
usage: python tools/calibration_timing.py [repeats]"""
import copy
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import hyperslam_amd as ha  # noqa: E402
from hyperslam_amd import synthetic  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20


def with_flags(w, free):
    w = copy.copy(w)
    c = np.ones((len(w.cam_T_bs), 3), np.uint8)
    for cam, block in free:
        c[cam, block] = 0
    w.cam_constant = c
    return w


c1, c2 = synthetic.config1(), synthetic.config2()
cases = (("configs[1] constant cameras", c1), ("configs[1] 22 camera columns", with_flags(c1, [(1, 0), (1, 1), (1, 2), (0, 1), (0, 2)])),
         ("configs[2] constant cameras", c2), ("configs[2] camera 0 T_bs", with_flags(c2, [(0, 0)])))
for name, w in cases:
    with ha.Problem(w) as p:
        p.reduced_system(1e4)
        t = time.perf_counter()
        for _ in range(reps):
            p.reduced_system(1e4)
        dt = (time.perf_counter() - t) / reps
        print(f"{name}: dim {p.dim_pose()}: hs_reduced_system {1e3 * dt:.3f} ms wall per call (device build + copy-out to the host)", flush=True)
