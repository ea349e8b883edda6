"""Front-end timing: hs_tracker_process on the 752 x 480 stereo sequence of tests/klt_scenes.py (150 tracks, levels 0..3).

Prints one JSON line: host wall time of hs_tracker_process (synchronous: it returns with the message on the host), and the kernel
launches and host synchronisations per frame of tracker.hpp's launch sequence. The device time per frame is the sum of the k_klt_* kernel
durations of `rocprofv3 --kernel-trace --stats -- python tools/time_tracker.py` divided by the frames (--kernel-trace-csv sums a trace)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-trace-csv", help="sum the k_klt_* durations of a rocprofv3 kernel trace instead of running")
    a = ap.parse_args()
    if a.kernel_trace_csv:
        import csv
        rows = [r for r in csv.DictReader(open(a.kernel_trace_csv)) if "k_klt_" in r["Kernel_Name"]]
        total = sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows)
        print(json.dumps({"metric": "klt_kernels", "frames": a.frames, "kernels": len(rows), "device_ms_per_frame": 1e-6 * total / a.frames}))
        return
    import hyperslam_amd as ha
    import klt_scenes as S
    scene = S.StereoPlane(0)
    frames = [scene.frame(k) for k in range(a.frames)]
    wall, n_tracks = [], []
    with ha.Tracker(S.WIDTH, S.HEIGHT) as t:
        for k, (L, R) in enumerate(frames):
            t0 = time.perf_counter()
            m = t.process(float(k), L, R)
            t1 = time.perf_counter()
            if k >= a.warmup and m is not None:
                wall.append(1e3 * (t1 - t0))
                n_tracks.append(len(m["ids"]))
    levels = 4
    launches = (levels + 1) + 3 + 4 + 3  # pyramids of the new pair, old-track passes, corners, new-track passes
    print(json.dumps({"metric": "klt_frame", "frames": len(wall), "tracks_per_frame": float(np.mean(n_tracks)),
                      "wall_ms_per_frame": float(np.median(wall)),
                      "launches_per_frame": launches, "host_syncs_per_frame": 3}))


if __name__ == "__main__":
    main()
