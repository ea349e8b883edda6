"""CPU tests (no GPU): the at-rest windows of tests/degenerate_windows.py are well posed for the oracle alone, take the series branches of the
rotation helpers, and the emulated fused build (tests/emul/build_harness.cpp: the product's kernel sources on the host) agrees with the
oracle on them.

What the windows can and cannot do, measured with the oracle: a solve moves the free control points off the rest rotation at once. With
0.5 px of pixel noise the largest relative rotation of two consecutive control points after five iterations is 1.5e-1 rad at order 4 and
2.0 rad at order 6 (40 landmarks x 3 pairs; 7e-3 and 1.7e-1 with 40 pairs; 2000 unit-weight priors change nothing against pixels that weigh
458 per radian); without pixel noise it is 1.7e-4 / 1.1e-2 / 6.4e-3 rad after one iteration at orders 4 / 5 / 6. The coefficients of a
B-spline fitted to observations are not smooth even when the curve is, and the last control points of a window are barely observed. So only
the pairs among the K constant control points stay below 1e-4 rad through a solve. The series branches run for every pair in the FIRST
linearisation of a solve, in linearize / reduced_system / covariance, and in every iteration only on the `held` windows (rotations
constant), which is what test_series_branches_before_and_after_a_solve pins."""
import numpy as np
import pytest

import degenerate_windows as dw
import hyperslam_amd as ha
from test_emulated_build import _check, harness, run_emulated_build  # noqa: F401  (harness: the fixture that builds build_harness)


def all_windows():
    for k in dw.ORDERS:
        for amp in dw.AMPS:
            for bearing in (False, True):
                yield f"small_k{k}_{amp}{'_bearing' if bearing else ''}", dw.small(k, amp, bearing=bearing)
        yield f"small_k{k}_thresholds_flip", dw.small(k, "thresholds", flip=True)
        for amp in ("0", "thresholds"):
            yield f"imu_k{k}_{amp}", dw.with_imu(k, amp)
        yield f"held_k{k}", dw.held(k)
    for amp in ("0", "thresholds"):
        yield f"long_k4_{amp}", dw.long_window(amp)


@pytest.mark.parametrize("name,w", list(all_windows()), ids=[n for n, _ in all_windows()])
def test_windows_are_well_posed(name, w, oracle):
    """Five LM iterations of the oracle, all successful, the final cost below the initial one; the constant control points do not move."""
    with ha.Problem(w, lib=oracle) as p:
        if w.imu is not None:
            p.set_inertial_jacobian(ha.HS_INERTIAL_EXACT)
        s = p.solve(5)
        cp = p.control_points()
    assert s["num_iterations"] == 5 and s["num_successful_steps"] == 5, [it["step_is_successful"] for it in s["iterations"][1:]]
    assert s["final_cost"] < s["initial_cost"]
    assert np.array_equal(cp[:w.order], w.control_points[:w.order])


@pytest.mark.parametrize("order", dw.ORDERS)
def test_series_branches_before_and_after_a_solve(order, oracle):
    """Before a solve every pair of the `0` and `1e-9` windows is in the t2 < 1e-8 branch, and the `thresholds` windows have pairs on both
    sides. After the oracle's solve: every pair of the `held` windows still is, in every iteration; of the free windows only the pairs among
    the K constant control points are (module docstring)."""
    for amp in ("0", "1e-9"):
        for w in (dw.small(order, amp), dw.small(order, amp, flip=True), dw.with_imu(order, amp), dw.visual_only(order, amp)):
            assert dw.pairs_below_t2(w.control_points).all()
    below = dw.pairs_below_t2(dw.small(order, "thresholds").control_points)
    assert below.sum() >= 4 and (~below).sum() >= 4
    for amp in ("0", "1e-9"):
        w = dw.held(order, amp)
        for n in range(1, 6):
            with ha.Problem(w, lib=oracle) as p:
                s = p.solve(n)
                cp = p.control_points()
            assert s["num_successful_steps"] == n and dw.pairs_below_t2(cp).all()
            assert np.array_equal(cp[:, :4], w.control_points[:, :4]) and not np.array_equal(cp[order:, 4:7], w.control_points[order:, 4:7])
        w = dw.small(order, amp)
        with ha.Problem(w, lib=oracle) as p:
            p.solve(5)
            after = dw.pairs_below_t2(p.control_points())
        assert after[:order - 1].all()
        print(f"order {order} amp {amp}: {int(after.sum())} of {len(after)} pairs below 1e-4 rad after five iterations")


def test_flip_negates_the_odd_control_points_only():
    a, b = dw.small(5, "thresholds"), dw.small(5, "thresholds", flip=True)
    assert np.array_equal(a.control_points[0::2], b.control_points[0::2]) and np.array_equal(a.control_points[1::2, 4:], b.control_points[1::2, 4:])
    assert np.array_equal(a.control_points[1::2, :4], -b.control_points[1::2, :4])
    c = dw.negate_odd_control_points(a)
    assert np.array_equal(c.control_points, b.control_points) and np.array_equal(a.pixels, b.pixels)


def test_imu_measures_a_body_at_rest(oracle):
    """At the true state (rest pose, true biases, true gravity) the inertial residuals of the at-rest window are its sensor noise and nothing
    else, whatever the IMU's extrinsics, intrinsics, sensitivity and offsets: within five sigma, the mean within one."""
    from hyperslam_amd import synthetic
    for identity in (False, True):
        w = dw.at_rest(order=4, n_inertial=200, identity_imu=identity, seed=3)
        q0, p0 = dw.rest_pose()
        w.control_points[:, :4], w.control_points[:, 4:7] = q0, p0
        w.imu["bias_g"][:, :3], w.imu["bias_a"][:, :3] = dw.BIAS_G, dw.BIAS_A
        w.gravity = np.array([0.0, 0.0, -synthetic.GRAVITY_NORM])
        with ha.Problem(w, lib=oracle) as p:
            p.set_inertial_jacobian(ha.HS_INERTIAL_EXACT)
            r = p.linearize(ha.HS_INERTIAL, robustify=False)["r"]
        sg, sa = synthetic.GYRO_NOISE_DENSITY * np.sqrt(synthetic.IMU_RATE), synthetic.ACCEL_NOISE_DENSITY * np.sqrt(synthetic.IMU_RATE)
        assert r.shape == (200, 6)
        assert np.abs(r[:, :3]).max() < 5 * sg and np.abs(r[:, 3:]).max() < 5 * sa
        assert np.abs(r[:, :3].mean(0)).max() < sg / 3 and np.abs(r[:, 3:].mean(0)).max() < sa / 3
        assert r[:, :3].std() > sg / 2 and r[:, 3:].std() > sa / 2


# ---- the emulated fused build on at-rest windows ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("bearing", [False, True])
@pytest.mark.parametrize("order", dw.ORDERS)
def test_emulated_fused_build_at_rest(harness, oracle, order, bearing, flip):  # noqa: F811
    for amp in ("0", "thresholds"):
        out = _check(harness, oracle, dw.visual_only(order, amp, flip=flip, bearing=bearing), tol=1e-9)
        assert out["n_chunk"] >= 2


@pytest.mark.parametrize("order", dw.ORDERS)
def test_emulated_full_iteration_at_rest(harness, oracle, order):  # noqa: F811
    """One whole LM iteration of the product's kernel chain on the CPU against the oracle's first iteration (the bars of
    test_emulated_full_iteration_matches_oracle)."""
    w = dw.visual_only(order, "0", flip=order == 5)
    out = run_emulated_build(harness, w, full=True)
    u = out["upd"]
    assert u[0] <= 1e-12 and u[1] == 0.0, u[:2]
    cost_after, cost_change, gmax, step_norm, rel_dec, radius, valid, ok, st_cost, accepted, done, dcp = u[-12:]
    with ha.Problem(w, lib=oracle) as p:
        s = p.solve(1)
    r = s["iterations"][0]
    assert s["num_iterations"] == 1 and valid == r["step_is_valid"] == 1 and ok == r["step_is_successful"] and accepted == ok and dcp == 0.0
    for got, name in ((cost_after, "cost"), (cost_change, "cost_change"), (gmax, "gradient_max_norm"), (step_norm, "step_norm"), (rel_dec, "relative_decrease"),
                      (radius, "radius")):
        assert abs(got - r[name]) <= 1e-9 * max(abs(r[name]), 1e-300), (name, got, r[name])
    assert abs(st_cost - s["final_cost"]) <= 1e-9 * s["final_cost"]
