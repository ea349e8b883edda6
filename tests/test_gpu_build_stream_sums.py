"""GPU tests: the fused build on windows whose J_p'J_p tiles get up to sixteen record streams from the per-chunk deal (every observation of a
landmark inside one or two knot intervals), so that every level of the recursive halving of the stream sums (kernels_build.hpp, phase 3) runs
on the device — v_swap under EXEC, the DPP exchanges of lane ^ 1, 2, 4, 8, the additions under the lane condition and the spread write of
the finished tiles — against the oracle. Tolerances: those of the fused-build tests of test_gpu_parity.py. The CPU emulation pins the same
windows bit for bit (tests/test_emulated_build_stream_sums.py)."""
import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

pytestmark = pytest.mark.gpu

WINDOWS = {
    "crowded_k4": dict(order=4, n_cp=14, n_landmarks=36, obs_pairs=5, span=0.05),
    "crowded_k6": dict(order=6, n_cp=16, n_landmarks=36, obs_pairs=4, span=0.15),
    "crowded_k5": dict(order=5, n_cp=16, n_landmarks=40, obs_pairs=5, span=0.1),
}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


@pytest.fixture(autouse=True)
def fused_build(monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", "fused")


@pytest.mark.parametrize("name", list(WINDOWS))
def test_reduced_system_crowded_segments(name, hip, oracle):
    w = synthetic.small_visual(**WINDOWS[name])
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        Sg, gg = g.reduced_system(1e4)
        Sc, gc = c.reduced_system(1e4)
        assert rel(Sg, Sc) < 1e-9, rel(Sg, Sc)
        assert rel(gg, gc) < 1e-9, rel(gg, gc)
        assert np.array_equal(Sg, Sg.T)


@pytest.mark.parametrize("name", list(WINDOWS))
def test_solve_crowded_segments(name, hip, oracle):
    w = synthetic.small_visual(**WINDOWS[name])
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        sg, sc = g.solve(5), c.solve(5)
        assert sg["num_iterations"] == sc["num_iterations"] and sg["termination"] == sc["termination"]
        for ig, ic in zip(sg["iterations"], sc["iterations"]):
            assert ig["step_is_successful"] == ic["step_is_successful"]
            assert abs(ig["cost"] - ic["cost"]) <= 1e-6 * abs(ic["cost"]) + 1e-8 * sc["initial_cost"], (name, ig["iteration"], ig["cost"], ic["cost"])
        assert rel(g.control_points(), c.control_points()) < 1e-6
        assert rel(g.landmarks(), c.landmarks()) < 1e-6
