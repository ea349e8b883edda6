"""Times hs_solve with free IMU blocks (hs_set_imu_estimation) on the shapes §14 measured the build on: configs[2] with T_bs free and
with T_bs + i_g + i_a free (18 columns, 122 border unknowns), and the replay-shaped stereo-inertial window (40 control points, 400 inertial rows)
with T_bs free, against the same windows with every IMU block constant. The constant cases call neither hs_set_imu_constancy nor
hs_set_imu_estimation, so they also run on a library that lacks the entry points (HS_LIBRARY=<the parent commit's build>: the baseline).
Wall time per LM iteration here; the per-kernel device split comes from running ONE case under rocprofv3 --kernel-trace --stats.
usage: python tools/imu_calibration_solve_timing.py [repeats] [case: c2const | c2T_bs | c2tga | rpconst | rpT_bs]   (default: every case)
       python tools/imu_calibration_solve_timing.py split <kernel_stats.csv> <LM iterations in the run>   (the per-iteration split of one run)"""
import copy
import csv
import sys
import time

import numpy as np

BUILD = ("k_imucal_rows", "k_imucal_pi", "k_imucal_bb", "k_imucal_ii", "k_imucal_finish")
GROUPS = (("factorisation", ("k_band_factor", "k_dense_factor", "k_dense_solve_mx", "k_factor_decoupled_rows", "k_dense_border_init")),
          ("border chain", ("k_border_forward", "k_border_schur", "k_border_solve", "k_border_apply")),
          ("sweeps", ("k_band_backward",)),
          ("update", ("k_update_visual", "k_backsub_retract", "k_cost_", "k_pack_decision", "k_decide", "k_commit")),
          ("candidate + commit", ("k_imucal_candidate", "k_imucal_commit")))


def split(path, iterations):
    rows = [(r["Name"], int(r["Calls"]), float(r["TotalDurationNs"]) / 1e3) for r in csv.DictReader(open(path))]
    rows = [r for r in rows if "hs::" in r[0]]
    per = lambda keys: sum(t for n, _, t in rows if any(("hs::" + k) in n for k in keys)) / iterations  # noqa: E731
    total, build = sum(t for _, _, t in rows) / iterations, per(BUILD)
    print(f"  kernel time {total:.1f} us per LM iteration ({iterations} iterations), of which the five section-14 build kernels {build:.1f} us")
    solve = 0.0
    for name, keys in GROUPS:
        solve += per(keys)
        print(f"    solve side, {name:20s} {per(keys):9.2f} us")
    print(f"    solve side, together             {solve:9.2f} us;   linearisation, build and finalisation (the rest) {total - build - solve:.2f} us")
    for n, calls, t in sorted(rows, key=lambda r: -r[2])[:24]:
        print(f"    {n[:78]:78s} calls {calls:5d}  avg {t / calls:9.2f} us  per iteration {t / iterations:9.2f} us")


if len(sys.argv) > 1 and sys.argv[1] == "split":
    split(sys.argv[2], int(sys.argv[3]))
    sys.exit(0)

sys.path.insert(0, ".")
import hyperslam_amd as ha  # noqa: E402
from hyperslam_amd import synthetic  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
only = sys.argv[2] if len(sys.argv) > 2 else None


def replay_shaped():
    w = synthetic.small_inertial(order=4, n_cp=40, n_landmarks=150, obs_pairs=3, n_inertial=400, seed=3)
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(36, np.uint8)]
    return w


cases = (("c2const", "configs[2] constant IMU blocks", synthetic.config2, None),
         ("c2T_bs", "configs[2] T_bs free", synthetic.config2, [0, 1, 1, 1, 1]),
         ("c2tga", "configs[2] T_bs + i_g + i_a free", synthetic.config2, [0, 0, 0, 1, 1]),
         ("rpconst", "replay-shaped constant IMU blocks", replay_shaped, None),
         ("rpT_bs", "replay-shaped T_bs free", replay_shaped, [0, 1, 1, 1, 1]))
for key, name, make, flags in cases:
    if only and key != only:
        continue
    w = copy.copy(make())
    with ha.Problem(w) as p:
        if flags is not None:
            p.set_imu_constancy(np.array(flags, np.uint8))
            p.set_imu_estimation(True)
        p.snapshot()
        warm = p.solve(5)["num_iterations"]  # (first call: allocations, kernel objects)
        wall, iters = 0.0, 0
        for _ in range(reps):
            p.restore()
            t = time.perf_counter()
            s = p.solve(5)
            wall += time.perf_counter() - t
            iters += s["num_iterations"]
        print(f"{key}: {name}: dim {p.dim_pose()}: {s['num_iterations']} iterations, {s['num_successful_steps']} successful, cost {s['initial_cost']:.6g} -> "
              f"{s['final_cost']:.6g}; {1e3 * wall / max(iters, 1):.4f} ms wall per LM iteration over {reps} solves; LM iterations in this run: {warm + iters}", flush=True)
