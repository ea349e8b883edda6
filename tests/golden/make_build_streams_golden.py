"""Records what the emulated fused build (tests/emul/build_harness) delivers on the windows whose J_p'J_p tiles get up to sixteen record
streams, as data: tests/golden/build_streams.npz. The stream sums of phase 3 (kernels_build.hpp) are specified as a fixed tree of additions,
((s0 + s1) + (s2 + s3)) + ..., so a change of HOW the tree is evaluated must reproduce these arrays bit for bit
(tests/test_emulated_build_stream_sums.py). The file was written with a harness compiled from the sources before the recursive halving.

usage: python tests/golden/make_build_streams_golden.py path/to/build_harness
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from hyperslam_amd import synthetic  # noqa: E402
import test_emulated_build as teb  # noqa: E402

# (name, arguments of synthetic.small_visual, arguments of run_emulated_build)
WINDOWS = [
    ("crowded_k4", dict(order=4, n_cp=14, n_landmarks=36, obs_pairs=5, span=0.05), {}),
    ("crowded_k6", dict(order=6, n_cp=16, n_landmarks=36, obs_pairs=4, span=0.15), {}),
    ("stereo_k4", dict(order=4, n_cp=14, n_landmarks=40, obs_pairs=3), {}),
    ("small_chunks", dict(order=4, n_cp=16, n_landmarks=12, obs_pairs=20, span=0.6), dict(R=64, L=3)),
]

if __name__ == "__main__":
    out = {}
    for name, wkw, rkw in WINDOWS:
        o = teb.run_emulated_build(sys.argv[1], synthetic.small_visual(**wkw), **rkw)
        for key in ("S", "g", "Y"):
            out[name + "." + key] = o[key]
    np.savez_compressed(os.path.join(HERE, "build_streams.npz"), **out)
