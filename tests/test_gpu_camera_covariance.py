"""Covariance of free camera blocks on the GPU (hs_set_camera_covariance / hs_compute_covariance / hs_get_covariance /
hs_get_covariance_cross) against the dense numpy referee of tests/camera_covariance_referee.py — the full J'J over control
points, border, free camera coordinates and landmarks, inverted densely — on the windows that module names; their admissibility (condition
numbers, the camera blocks' response to a perturbation of the referee's input) is asserted on the CPU by
tests/test_camera_covariance_referee.py. Every comparison is at bar(cond) = max(1e-8, cond * 1e-14) of the window's referee; Sigma_cc and the
camera columns of the control-point / border cross block are compared relative to THEIR OWN max-norm (they are up to 1e-6 of the whole Sigma)."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha

import camera_covariance_referee as ccr
from camera_covariance_referee import bar, rel

pytestmark = pytest.mark.gpu

HS_ERR_STATE, HS_ERR_NUMERIC = 3, 4


def compare(w, R, cov, bw):
    """Every block of `cov` (Problem.covariance()) against the referee R of window w."""
    Sigma, tol, nc, n_cp = R["Sigma"], bar(R["cond"]), R["nc"], w.n_cp
    blocks = np.stack([Sigma[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n_cp)])
    band = np.zeros((n_cp, bw, 6, 6))
    for i in range(n_cp):
        for j in range(min(bw, n_cp - i)):
            band[i, j] = Sigma[6 * i:6 * i + 6, 6 * (i + j):6 * (i + j) + 6]
    B, X = Sigma[6 * n_cp:, 6 * n_cp:], Sigma[:6 * n_cp, 6 * n_cp:]
    got_X = cov["control_point_border"].reshape(6 * n_cp, -1)
    ok = ~np.isnan(R["lm_cov"])
    figures = dict(control_points=rel(cov["control_points"], blocks), band=rel(cov["control_point_band"], band), border=rel(cov["border"], B),
                   cross=rel(got_X, X), landmarks=rel(cov["landmarks"][ok], R["lm_cov"][ok]))
    if nc:
        figures.update(camera_block=rel(cov["border"][-nc:, -nc:], B[-nc:, -nc:]), camera_cross=rel(got_X[:, -nc:], X[:, -nc:]))
    print(f"cond {R['cond']:.3g} bar {tol:.3g} " + " ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    assert np.array_equal(np.isnan(cov["landmarks"]), np.isnan(R["lm_cov"]))
    for key, value in figures.items():
        assert value < tol, (key, value, tol)


def check_window(name, hip, oracle):
    w, _ = ccr.window(name, oracle)
    R = ccr.window_referee(name, oracle)
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_covariance(True)
        assert g.dim_pose() == R["Sigma"].shape[0]
        g.compute_covariance()
        cov, bw = g.covariance(), g.lib.band_blocks(g.h)
    compare(w, R, cov, bw)
    return w, cov, bw


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


@pytest.mark.parametrize("name", ccr.BOTH_BUILD_PATHS)
def test_window_on_both_build_paths(name, build_path, hip, oracle):
    check_window(name, hip, oracle)


@pytest.mark.parametrize("name", [n for n in ccr.WINDOWS if n not in ccr.BOTH_BUILD_PATHS])
def test_window(name, hip, oracle):
    w, cov, bw = check_window(name, hip, oracle)
    if name == "D":
        lmc = np.asarray(w.landmark_constant, bool)
        assert not cov["landmarks"][lmc].any() and not cov["control_points"][:5].any() and not cov["control_point_border"][:5].any()
    if name == "F":
        assert 6 * bw > 128, bw  # (k_cov_band on its global-memory path, with camera columns)
    if name in ("rotation_constant", "translation_constant"):
        frozen = slice(0, 3) if name == "rotation_constant" else slice(3, 6)
        assert not cov["control_points"][:, frozen, :].any() and not cov["control_point_border"][:, frozen, :].any()
    if name == "I4_both":
        assert cov["border"].shape[0] == 6 * len(w.imu["bias_g"]) + 2 + 28
    if name == "W":
        assert 6 * bw > 128, bw


def test_bearing_only_intrinsics_are_rank_deficient(hip):
    """Camera 1 is seen through bearing rows only: its intrinsics columns are all zero (the build's marker 1.0 on the diagonal)."""
    w = ccr.bearing_window()
    w.cam_constant = ccr.flags(w, cam1="ti")
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_covariance(True)
        assert g.lib.compute_covariance(g.h) == HS_ERR_NUMERIC
        assert b"camera 1, intrinsics coordinate 0" in g.lib.last_error(g.h), g.lib.last_error(g.h)
        assert g.lib.get_covariance(g.h, None, None, None, None) == HS_ERR_STATE
        assert g.lib.get_covariance_cross(g.h, ha.problem._d(np.zeros(1))) == HS_ERR_STATE


def test_switch_off_refuses_as_before(hip, oracle):
    w, _ = ccr.window("A", oracle)
    refusal = r"\(3\).*hs_compute_covariance: free camera blocks \(hs_set_camera_constancy\) are not supported$"
    with ha.Problem(w, lib=hip) as g:
        with pytest.raises(ha.problem.HsError, match=refusal):
            g.compute_covariance()
        g.set_camera_estimation(True)  # (an independent switch)
        with pytest.raises(ha.problem.HsError, match=refusal):
            g.compute_covariance()
        g.set_camera_covariance(True)
        g.compute_covariance()
        g.set_camera_covariance(False)
        with pytest.raises(ha.problem.HsError, match=refusal):
            g.compute_covariance()


def plain_windows(oracle):
    from test_gpu_covariance import inertial_window
    yield ccr.constant_cameras(ccr.window("A", oracle)[0])
    yield inertial_window(4, oracle)


def test_switch_on_without_free_cameras_is_bit_identical(hip, oracle):
    for w in plain_windows(oracle):
        with ha.Problem(w, lib=hip) as a, ha.Problem(w, lib=hip) as b:
            b.set_camera_covariance(True)
            a.compute_covariance()
            b.compute_covariance()
            ca, cb = a.covariance(), b.covariance()
            assert set(ca) == set(cb)
            for key in ca:
                assert np.array_equal(ca[key], cb[key], equal_nan=True), key
            b.set_camera_covariance(False)  # (no free camera coordinate: the switch does not touch the handle)
            assert b.lib.get_covariance(b.h, None, None, None, None) == 0


@pytest.mark.parametrize("name", ["A", "I4_both"])
def test_two_calls_bit_identical(name, hip, oracle):
    w, _ = ccr.window(name, oracle)
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_covariance(True)
        g.compute_covariance()
        a = g.covariance()
        g.compute_covariance()
        b = g.covariance()
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_solve_after_covariance_is_unchanged(hip, oracle):
    w, _ = ccr.window("A", oracle)
    with ha.Problem(w, lib=hip) as a, ha.Problem(w, lib=hip) as b:
        for g in (a, b):
            g.set_camera_estimation(True)
        a.set_camera_covariance(True)
        a.compute_covariance()
        sa, sb = a.solve(5), b.solve(5)
        assert sa["final_cost"] == sb["final_cost"] and sa["iterations"] == sb["iterations"]
        assert np.array_equal(a.control_points(), b.control_points())
        assert np.array_equal(a.landmarks(), b.landmarks())
        for x, y in zip(a.cameras(), b.cameras()):
            assert np.array_equal(x, y)


def test_stale_after_changes(hip, oracle):
    w, _ = ccr.window("A", oracle)
    with ha.Problem(w, lib=hip) as g:
        cross = np.zeros((w.n_cp, 6, 14))
        get = lambda: (g.lib.get_covariance(g.h, None, None, None, None), g.lib.get_covariance_cross(g.h, ha.problem._d(cross)))  # noqa: E731
        g.set_camera_covariance(True)
        g.set_camera_estimation(True)
        assert get() == (HS_ERR_STATE, HS_ERR_STATE)
        g.compute_covariance()
        assert get() == (0, 0) and cross.any()
        T, I, D = g.cameras()
        I2 = I * (1.0 + 1e-3)
        assert g.lib.set_cameras(g.h, len(T), ha.problem._d(T), ha.problem._d(I2), ha.problem._d(D)) == 0
        assert get() == (HS_ERR_STATE, HS_ERR_STATE)
        g.compute_covariance()
        g.set_camera_constancy(ccr.flags(w, cam1="t"))
        assert get() == (HS_ERR_STATE, HS_ERR_STATE)
        g.set_camera_constancy(ccr.flags(w, cam1="tid"))
        g.compute_covariance()
        g.set_camera_covariance(False)
        assert get() == (HS_ERR_STATE, HS_ERR_STATE)
        g.set_camera_covariance(True)
        assert get() == (HS_ERR_STATE, HS_ERR_STATE)
        g.compute_covariance()
        assert get() == (0, 0)
        g.solve(2)
        assert get() == (HS_ERR_STATE, HS_ERR_STATE)
        g.compute_covariance()
        assert get() == (0, 0)


def test_cross_block_of_an_imu_border_without_the_switch(hip, oracle):
    """hs_get_covariance_cross is not tied to the switch: control points x (bias splines, gravity) against the referee of
    tests/test_gpu_covariance.py."""
    from test_gpu_covariance import inertial_window, referee
    w = inertial_window(4, oracle)
    Sigma, _, cond = referee(w, oracle)
    with ha.Problem(w, lib=hip) as g:
        g.compute_covariance()
        cov = g.covariance()
    n = 6 * w.n_cp
    got = cov["control_point_border"]
    assert got.shape == (w.n_cp, 6, Sigma.shape[0] - n)
    err = rel(got.reshape(n, -1), Sigma[:n, n:])
    print(f"cond {cond:.3g} bar {bar(cond):.3g} cross {err:.3g}")
    assert err < bar(cond), (err, bar(cond))
    assert not got[:w.order].any()  # (the frozen prefix)


def test_covariance_after_estimation_is_taken_at_the_estimate(hip, oracle):
    w, _ = ccr.window("A", oracle)
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_estimation(True)
        g.set_camera_covariance(True)
        g.solve(5)
        g.compute_covariance()
        cov, bw = g.covariance(), g.lib.band_blocks(g.h)
        we = copy.copy(w)
        we.control_points, we.landmarks = g.control_points(), g.landmarks()
        we.cam_T_bs, we.cam_intrinsics, we.cam_distortion = g.cameras()
    assert not np.array_equal(we.cam_intrinsics, w.cam_intrinsics) and not np.array_equal(we.cam_T_bs, w.cam_T_bs)
    R = ccr.referee(we, oracle)
    R0 = ccr.window_referee("A", oracle)
    assert rel(R["Sigma"], R0["Sigma"]) > bar(R["cond"])  # (the estimate is another point: the referee at the initial cameras would not pass)
    compare(we, R, cov, bw)
