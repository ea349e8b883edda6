"""Times hs_solve with free camera blocks (hs_set_camera_estimation) on the two shapes §13 measured the build on: configs[1] with
camera 1 fully free and camera 0's intrinsics and distortion free (22 camera columns), and configs[2] with camera 0's T_bs free, against the
same windows with every camera constant. Wall time per LM iteration here; the per-kernel device split comes from running it under
rocprofv3 --kernel-trace --stats (one case per run: `only` selects it).
usage: python tools/calibration_solve_timing.py [repeats] [only: c1const | c1free | c2const | c2free]"""
import copy
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import hyperslam_amd as ha  # noqa: E402
from hyperslam_amd import synthetic  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
only = sys.argv[2] if len(sys.argv) > 2 else None


def with_flags(w, free):
    w = copy.copy(w)
    c = np.ones((len(w.cam_T_bs), 3), np.uint8)
    for cam, block in free:
        c[cam, block] = 0
    w.cam_constant = c
    return w


cases = (("c1const", "configs[1] constant cameras", synthetic.config1, None),
         ("c1free", "configs[1] 22 camera columns", synthetic.config1, [(1, 0), (1, 1), (1, 2), (0, 1), (0, 2)]),
         ("c2const", "configs[2] constant cameras", synthetic.config2, None),
         ("c2free", "configs[2] camera 0 T_bs", synthetic.config2, [(0, 0)]))
for key, name, make, free in cases:
    if only and key != only:
        continue
    w = make() if free is None else with_flags(make(), free)
    with ha.Problem(w) as p:
        if free is not None:
            p.set_camera_estimation(True)
        p.snapshot()
        s = p.solve(5)  # (first call: allocations, kernel objects)
        wall, iters = 0.0, 0
        for _ in range(reps):
            p.restore()
            t = time.perf_counter()
            s = p.solve(5)
            wall += time.perf_counter() - t
            iters += s["num_iterations"]
        print(f"{key}: {name}: dim {p.dim_pose()}: {s['num_iterations']} iterations, {s['num_successful_steps']} successful, cost {s['initial_cost']:.6g} -> "
              f"{s['final_cost']:.6g}; {1e3 * wall / iters:.4f} ms wall per LM iteration over {reps} solves, {iters} iterations in all", flush=True)
