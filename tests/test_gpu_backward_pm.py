"""The backward sweep with one phase per super-step on premultiplied blocks (k_band_backward_pm, the default) against the two-phase sweep
it replaces (k_band_backward_sb behind the product switch backward_sb, HS_DEBUG_FLAGS=4294967296) and against the oracle, on windows whose reduced
system is factored from both ends: configs[1]'s band at half its length, a short band, and a bordered (stereo-inertial) one.
Tolerances: tests/test_gpu_parity.py::test_solve_trajectory's (the bar of the HIP path against the oracle); the two sweeps differ in rounding
only — (U Winv) y instead of U (Winv y) — so they are held to the same bar against each other."""
import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import switches, synthetic

pytestmark = pytest.mark.gpu

TWO_PHASE = switches.flags("backward_sb")


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


def windows():
    yield "visual_bw13", synthetic.small_visual(order=4, n_cp=64, n_landmarks=300), False
    yield "visual_short_band", synthetic.small_visual(order=4, n_cp=24, n_landmarks=100, span=0.2), False
    w = synthetic.small_inertial(order=4, n_cp=72, n_landmarks=300, obs_pairs=3, n_inertial=600, seed=33)  # test_gpu_inertial.test_two_ended_bordered_solve
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(72 - 4, np.uint8)]
    yield "stereo_inertial", w, True


def state(p, imu):
    out = [p.control_points().copy(), p.landmarks().copy()]
    if imu:
        bg, ba = p.bias()
        out += [p.gravity().copy(), bg.copy(), ba.copy()]
    return out


def check_trajectory(sa, sb, name):
    """test_gpu_parity.test_solve_trajectory's comparison of two solve summaries."""
    assert sa["num_iterations"] == sb["num_iterations"]
    assert sa["num_successful_steps"] == sb["num_successful_steps"]
    assert sa["termination"] == sb["termination"]
    for ia, ib in zip(sa["iterations"], sb["iterations"]):
        assert ia["step_is_successful"] == ib["step_is_successful"]
        assert abs(ia["cost"] - ib["cost"]) <= 1e-6 * abs(ib["cost"]) + 1e-8 * sb["initial_cost"], (name, ia["iteration"], ia["cost"], ib["cost"])
        for k in ("radius", "step_norm", "relative_decrease"):
            assert abs(ia[k] - ib[k]) <= 1e-5 * max(abs(ib[k]), 1e-12), (name, ia["iteration"], k, ia[k], ib[k])


@pytest.mark.parametrize("name,w,imu", list(windows()), ids=[n for n, *_ in windows()])
def test_one_phase_sweep_against_two_phase_and_oracle(name, w, imu, hip, oracle, monkeypatch):
    monkeypatch.delenv("HS_DEBUG_FLAGS", raising=False)
    with ha.Problem(w, lib=hip) as p:
        bw = p.lib.band_blocks(p.h)
        # launch_factor's rule for the factorisation from both ends, whose sweeps are the ones under test (6 (bw - 1) <= 96 follows)
        assert w.n_cp >= 4 * bw and bw <= 16, (bw, w.n_cp)
        p.snapshot()
        s_new = p.solve(5)
        new = state(p, imu)
        p.restore()
        s_again = p.solve(5)  # the same launch sequence from the same point: the same bits
        for x, y in zip(state(p, imu), new):
            assert np.array_equal(x, y)
        assert [it["cost"] for it in s_again["iterations"]] == [it["cost"] for it in s_new["iterations"]]
    monkeypatch.setenv("HS_DEBUG_FLAGS", TWO_PHASE)
    with ha.Problem(w, lib=hip) as p:
        s_old = p.solve(5)
        old = state(p, imu)
    monkeypatch.delenv("HS_DEBUG_FLAGS")
    with ha.Problem(w, lib=oracle) as c:
        s_ref = c.solve(5)
        ref = state(c, imu)
    print(name, "bw", bw, "final cost one-phase %.17g two-phase %.17g oracle %.17g" % (s_new["final_cost"], s_old["final_cost"], s_ref["final_cost"]))
    for what, sa, a, sb, b in (("one-phase / two-phase", s_new, new, s_old, old), ("one-phase / oracle", s_new, new, s_ref, ref),
                               ("two-phase / oracle", s_old, old, s_ref, ref)):
        print(name, what, ["%.2e" % rel(x, y) for x, y in zip(a, b)])
        check_trajectory(sa, sb, name + " " + what)
        for x, y in zip(a, b):
            assert rel(x, y) < 1e-6, (name, what)
