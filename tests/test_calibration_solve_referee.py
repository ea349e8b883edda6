"""Pins the numpy LM referee of tests/calibration_solve_referee.py (CPU only, no GPU).

With every camera block constant the referee reproduces the oracle's own solve(5): identical decisions, and costs, radii, step norms,
relative decreases and end points at the bars below. Both sides are fp64 restatements of the same rules on the same rows; they differ in
the order of every sum and in the linear algebra (the oracle: envelope Cholesky of the system formed in fp64; the referee: a refined LU of the
system formed in extended precision), and an LM trajectory amplifies that from one iteration to the next. Measured worst case over the six
windows below (five iterations each): cost 2.4e-8 of (|cost| + 1e-2 initial cost), radius / step norm / relative decrease 6.5e-8 relative, end
points 3.3e-8 relative. The bars are ten times that: 2.4e-7, 6.5e-7 and 3.3e-7 — below the device bars of tests/test_gpu_calibration_solve.py
(1e-6, 1e-5, 1e-6), so the referee is good enough to judge the device.

With free camera blocks the referee's first step is computed two ways — landmarks eliminated by Schur complement, then back-substituted; and
the full damped, scaled normal equations with the landmarks in one dense solve — which must agree to 1e-10 relative. This pins the formula
the device implements: dl = S_l V^-1 (S_l b_l - S_l H_lp y_p - S_l H_lc y_c)."""
import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import calibration_solve_referee as sref
from test_calibration_referee import windows as constant_windows

COST_BAR, RECORD_BAR, POINT_BAR = 2.4e-7, 6.5e-7, 3.3e-7


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def windows():
    yield from constant_windows()
    # far enough from the optimum that steps are rejected (tests/test_gpu_edge_cases.py::perturbed_visual)
    w, _ = synthetic._visual_window(1, 4, 20, 120, 3, bearing=False, lm_noise=0.5, span=1.0)
    w.control_points = w.control_points.copy()
    w.control_points[:, 4:7] += 0.3 * np.random.default_rng(1).standard_normal((20, 3))
    yield "rejected_steps", w


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
def test_constant_cameras_reproduce_the_oracle_solve(name, w, oracle):
    with ha.Problem(w, lib=oracle) as c:
        sc = c.solve(5)
        cp, lm = c.control_points(), c.landmarks()
        state = (c.bias(), c.gravity()) if w.imu is not None else None
    sr, wf = sref.solve(w, oracle, 5)
    decisions = [it["step_is_successful"] for it in sc["iterations"]]
    if name == "rejected_steps":
        assert 0 in decisions[1:] and 1 in decisions[1:], decisions
    assert [it["step_is_successful"] for it in sr["iterations"]] == decisions
    assert [it["step_is_valid"] for it in sr["iterations"]] == [it["step_is_valid"] for it in sc["iterations"]]
    for f in ("num_iterations", "num_successful_steps", "termination"):
        assert sr[f] == sc[f], f
    worst = {"cost": 0.0, "record": 0.0}
    for ir, ic in zip(sr["iterations"], sc["iterations"]):
        worst["cost"] = max(worst["cost"], abs(ir["cost"] - ic["cost"]) / (abs(ic["cost"]) + 1e-2 * sc["initial_cost"]))
        for k in ("radius", "step_norm", "relative_decrease", "gradient_max_norm"):
            worst["record"] = max(worst["record"], abs(ir[k] - ic[k]) / max(abs(ic[k]), 1e-12))
    worst["point"] = max(rel(wf.control_points, cp), rel(wf.landmarks, lm))
    if state is not None:
        worst["point"] = max(worst["point"], rel(wf.imu["bias_g"], state[0][0]), rel(wf.imu["bias_a"], state[0][1]), rel(wf.gravity, state[1]))
    print(name, worst)
    assert worst["cost"] <= COST_BAR and worst["record"] <= RECORD_BAR and worst["point"] <= POINT_BAR, worst
    assert abs(sr["final_cost"] - sc["final_cost"]) <= COST_BAR * (sc["final_cost"] + 1e-2 * sc["initial_cost"])


@pytest.mark.parametrize("name,w", list(sref.free_camera_windows()), ids=[n for n, _ in sref.free_camera_windows()])
def test_first_step_with_free_cameras_two_ways(name, w, oracle):
    sysm = sref.System(w, oracle)
    assert sysm.nc > 0
    s, sl = sysm.scaling()
    for radius in (1e4, 3e2):
        dx, dl = sysm.step_schur(s, sl, radius)
        fx, fl = sysm.step_full(s, sl, radius)
        assert np.abs(dx[sysm.P0:]).max() > 0.0  # (the camera coordinates move)
        assert rel(dx, fx) < 1e-10 and rel(dl, fl) < 1e-10, (radius, rel(dx, fx), rel(dl, fl))
        assert rel(dx[sysm.P0:], fx[sysm.P0:]) < 1e-10
    # the model cost change of the step: -(J step).(r + J step / 2) against -g.step / 2 + step'D^2 step / 2 in scaled coordinates, which is
    # what the device forms (equal for the exact solution of the damped system)
    S, g, D = sysm.scaled_system(s, sl, 1e4)
    dx, dl = sysm.step_schur(s, sl, 1e4)
    step_x, step_l = dx / s, dl / sl
    d2 = float(step_x @ (D * step_x))
    for l, (_, d) in sysm.landmark_blocks(sl, 1e4).items():
        d2 += float(step_l[l] @ (np.asarray(d, float) * step_l[l]))
    alt = -0.5 * (sysm.gx @ dx + np.einsum("li,li->", sysm.bl, dl)) + 0.5 * d2
    mcc = sysm.model_cost_change(dx, dl)
    assert mcc > 0 and abs(alt - mcc) <= 1e-9 * mcc, (alt, mcc)
