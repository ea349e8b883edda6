"""Covariance of free IMU blocks and of sensor poses on the GPU (hs_set_imu_covariance / hs_compute_covariance / hs_get_covariance /
hs_get_covariance_cross / hs_sample_sensor_covariance) against the dense numpy referee of tests/imu_covariance_referee.py —
the full J'J over control points, border, free IMU coordinates, free camera coordinates and landmarks, inverted densely — on the windows that
module names; their admissibility (condition numbers, the IMU blocks' response to a perturbation of the referee's input) is asserted on the
CPU by tests/test_imu_covariance_referee.py. Every comparison is at bar(cond) = max(1e-8, cond * 1e-14) of the window's referee; Sigma_ii, the
IMU columns of the cross block and the camera blocks are compared relative to THEIR OWN max-norm.

Without hs_set_imu_covariance every test here that switches it on fails: the entry point is missing and hs_compute_covariance refuses."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha

import imu_covariance_referee as imr
from imu_covariance_referee import bar, rel

pytestmark = pytest.mark.gpu

HS_ERR_INVALID, HS_ERR_STATE, HS_ERR_NUMERIC = 1, 3, 4
REFUSAL = r"\(3\).*hs_compute_covariance: free IMU blocks \(hs_set_imu_constancy\) are not supported; hs_reduced_system builds their system"


def compare(w, R, cov, bw):
    """Every block of `cov` (Problem.covariance()) against the referee R of window w."""
    Sigma, tol, ni, nc, n_cp = R["Sigma"], bar(R["cond"]), R["ni"], R["nc"], w.n_cp
    blocks = np.stack([Sigma[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n_cp)])
    band = np.zeros((n_cp, bw, 6, 6))
    for i in range(n_cp):
        for j in range(min(bw, n_cp - i)):
            band[i, j] = Sigma[6 * i:6 * i + 6, 6 * (i + j):6 * (i + j) + 6]
    n, P0 = 6 * n_cp, R["P0"]
    B, X = Sigma[n:, n:], Sigma[:n, n:]
    got_X = cov["control_point_border"].reshape(n, -1)
    i0, i1 = P0 - n, P0 - n + ni  # the IMU columns inside the border
    ok = ~np.isnan(R["lm_cov"])
    figures = dict(control_points=rel(cov["control_points"], blocks), band=rel(cov["control_point_band"], band),
                   bias_gravity=rel(cov["border"][:i0, :i0], B[:i0, :i0]), border=rel(cov["border"], B), cross=rel(got_X, X),
                   landmarks=rel(cov["landmarks"][ok], R["lm_cov"][ok]))
    if ni:
        figures.update(imu_block=rel(cov["border"][i0:i1, i0:i1], B[i0:i1, i0:i1]), imu_cross=rel(got_X[:, i0:i1], X[:, i0:i1]))
    if nc:
        figures.update(camera_block=rel(cov["border"][-nc:, -nc:], B[-nc:, -nc:]), camera_cross=rel(got_X[:, -nc:], X[:, -nc:]))
    print(f"cond {R['cond']:.3g} bar {tol:.3g} " + " ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    assert np.array_equal(np.isnan(cov["landmarks"]), np.isnan(R["lm_cov"]))
    for key, value in figures.items():
        assert value < tol, (key, value, tol)


def switched_on(w, hip):
    g = ha.Problem(w, lib=hip)
    g.set_imu_covariance(True)
    if w.cam_constant is not None:
        g.set_camera_covariance(True)
    return g


def check_window(name, hip, oracle):
    w, R = imr.window(name, oracle), imr.window_referee(name, oracle)
    with switched_on(w, hip) as g:
        assert g.dim_pose() == R["Sigma"].shape[0]
        g.compute_covariance()
        cov, bw = g.covariance(), g.lib.band_blocks(g.h)
    compare(w, R, cov, bw)
    return w, R, cov


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


@pytest.mark.parametrize("name", imr.BOTH_BUILD_PATHS)
def test_window_on_both_build_paths(name, build_path, hip, oracle):
    check_window(name, hip, oracle)


@pytest.mark.parametrize("name", [n for n in imr.WINDOWS if n not in imr.BOTH_BUILD_PATHS])
def test_window(name, hip, oracle):
    w, R, cov = check_window(name, hip, oracle)
    nbi = 6 * len(w.imu["bias_g"]) + 2
    assert cov["border"].shape[0] == nbi + R["ni"] + R["nc"]
    assert not cov["control_points"][:w.order].any() and not cov["control_point_border"][:w.order].any()  # (the frozen prefix)


def sensor_cases(name, oracle):
    """(kind, index, T_bs, first column of its T_bs in Sigma or -1) of every sensor of a window, a plain one added."""
    w = copy.copy(imr.window(name, oracle))
    q = np.array([0.1, -0.2, 0.3, 1.0])
    w.sensor_T_bs = np.r_[q / np.linalg.norm(q), 0.3, -0.1, 0.2][None, :]
    R = imr.window_referee(name, oracle)
    cam_cols, _ = imr.camera_columns(w)
    imu_free = not np.asarray(w.imu_constant)[0]
    cases = [(ha.HS_SENSOR_IMU, 0, w.imu["T_bs"], R["P0"] if imu_free else -1), (ha.HS_SENSOR_PLAIN, 0, w.sensor_T_bs[0], -1)]
    for c in range(len(w.cam_T_bs)):
        cases.append((ha.HS_SENSOR_CAMERA, c, w.cam_T_bs[c], R["P0"] + R["ni"] + cam_cols[c, 0] if cam_cols[c, 0] >= 0 else -1))
    return w, R, cases


@pytest.mark.parametrize("name", ["k4_t", "k5_t", "k4_ga_cam1tid", "k6_ga"])
def test_sensor_pose_covariance(name, hip, oracle):
    """The IMU (free T_bs: k4_t, k5_t; constant: the others), a free camera (camera 1 of k4_ga_cam1tid), constant cameras and a plain sensor."""
    w, R, cases = sensor_cases(name, oracle)
    lo, hi = w.valid_range()
    stamps = np.r_[lo + 1e-3, hi - 1e-3, np.linspace(lo, hi, 9)[1:-1]]
    tol = bar(R["cond"])
    free_seen = 0
    with switched_on(w, hip) as g:
        g.compute_covariance()
        body = g.sample_covariance(stamps)
        for kind, index, T_bs, ecol in cases:
            got = g.sample_sensor_covariance(kind, index, stamps)
            want = imr.sensor_pose_covariance(R["Sigma"], w, oracle, T_bs, stamps, ecol)
            err = max(rel(a, b) for a, b in zip(got, want))  # (per stamp: each 6 x 6 relative to its own max-norm)
            print(f"{name}: kind {kind} index {index} T_bs column {ecol}: {err:.3g} (bar {tol:.3g})")
            assert err < tol, (kind, index, err, tol)
            assert np.array_equal(got, g.sample_sensor_covariance(kind, index, stamps))
            if ecol >= 0:
                free_seen += 1
                without = imr.sensor_pose_covariance(R["Sigma"], w, oracle, T_bs, stamps, -1)
                assert max(rel(a, b) for a, b in zip(want, without)) > 10.0 * tol  # (the border terms are what is being checked)
        assert free_seen == (1 if name != "k6_ga" else 0)
        # an identity T_bs is the body pose, bit for bit
        assert g.lib.set_sensors(g.h, 1, ha.problem._d(np.array([[0, 0, 0, 1, 0, 0, 0.0]]))) == 0
        g.compute_covariance()
        assert np.array_equal(g.sample_sensor_covariance(ha.HS_SENSOR_PLAIN, 0, stamps), g.sample_covariance(stamps))
        assert np.array_equal(g.sample_covariance(stamps), body)
        out = np.zeros((1, 6, 6))
        bad = lambda kind, index, t: g.lib.sample_sensor_covariance(g.h, kind, index, 1, ha.problem._d(np.array([t])), ha.problem._d(out))  # noqa: E731
        assert bad(3, 0, stamps[0]) == HS_ERR_INVALID and bad(-1, 0, stamps[0]) == HS_ERR_INVALID
        assert bad(ha.HS_SENSOR_IMU, 1, stamps[0]) == HS_ERR_INVALID and bad(ha.HS_SENSOR_CAMERA, 2, stamps[0]) == HS_ERR_INVALID
        assert bad(ha.HS_SENSOR_PLAIN, 1, stamps[0]) == HS_ERR_INVALID and bad(ha.HS_SENSOR_PLAIN, -1, stamps[0]) == HS_ERR_INVALID
        assert bad(ha.HS_SENSOR_IMU, 0, hi + 1.0) == HS_ERR_INVALID
        g.set_imu_covariance(False)
        assert bad(ha.HS_SENSOR_IMU, 0, stamps[0]) == HS_ERR_STATE


def test_switch_off_refuses_as_before(hip, oracle):
    w = imr.window("k4_ga_cam1tid", oracle)
    camera_refusal = r"\(3\).*hs_compute_covariance: free camera blocks \(hs_set_camera_constancy\) are not supported$"
    with ha.Problem(w, lib=hip) as g:
        with pytest.raises(ha.problem.HsError, match=REFUSAL):
            g.compute_covariance()
        g.set_imu_estimation(True)  # (independent switches)
        g.set_camera_covariance(True)
        with pytest.raises(ha.problem.HsError, match=REFUSAL):
            g.compute_covariance()
        g.set_camera_covariance(False)
        g.set_imu_covariance(True)
        with pytest.raises(ha.problem.HsError, match=camera_refusal):  # (free cameras still need their own switch)
            g.compute_covariance()
        g.set_camera_covariance(True)
        g.compute_covariance()
        g.set_imu_covariance(False)
        with pytest.raises(ha.problem.HsError, match=REFUSAL):
            g.compute_covariance()


@pytest.mark.parametrize("free", ["tx", "tgasx"])
def test_extrinsics_and_acc_offsets_both_free_are_refused(free, hip, oracle):
    w = copy.copy(imr.window("k4_t", oracle))
    w.imu_constant = imr.imu_flags(free)
    with ha.Problem(w, lib=hip) as g:
        g.set_imu_covariance(True)
        assert g.lib.compute_covariance(g.h) == HS_ERR_NUMERIC
        msg = g.lib.last_error(g.h)
        assert b"T_bs and X_a both free" in msg and b"through their sum only" in msg, msg
        assert g.lib.get_covariance(g.h, None, None, None, None) == HS_ERR_STATE
        g.set_imu_estimation(True)  # (hs_solve damps: it estimates both)
        assert g.solve(2)["iterations"]


@pytest.mark.parametrize("flags", [None, np.ones(5, np.uint8)])
def test_switch_on_without_free_imu_blocks_is_bit_identical(flags, hip, oracle):
    w = imr.constant_blocks(imr.window("k4_t", oracle))
    w.imu_constant = flags
    with ha.Problem(imr.constant_blocks(w), lib=hip) as a, ha.Problem(w, lib=hip) as b:
        b.set_imu_covariance(True)
        a.compute_covariance()
        b.compute_covariance()
        ca, cb = a.covariance(), b.covariance()
        assert set(ca) == set(cb)
        for key in ca:
            assert np.array_equal(ca[key], cb[key], equal_nan=True), key
        b.set_imu_covariance(False)  # (no free IMU coordinate: the switch does not touch the handle)
        assert b.lib.get_covariance(b.h, None, None, None, None) == 0


@pytest.mark.parametrize("name", ["k4_tgas", "k4_ga_cam1tid"])
def test_two_calls_bit_identical(name, hip, oracle):
    w = imr.window(name, oracle)
    with switched_on(w, hip) as g:
        g.compute_covariance()
        a = g.covariance()
        g.compute_covariance()
        b = g.covariance()
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


def test_solve_after_covariance_is_unchanged(hip, oracle):
    w = imr.window("k4_tgas", oracle)
    with ha.Problem(w, lib=hip) as a, ha.Problem(w, lib=hip) as b:
        for g in (a, b):
            g.set_imu_estimation(True)
        a.set_imu_covariance(True)
        a.compute_covariance()
        sa, sb = a.solve(5), b.solve(5)
        assert sa["final_cost"] == sb["final_cost"] and sa["iterations"] == sb["iterations"]
        assert np.array_equal(a.control_points(), b.control_points()) and np.array_equal(a.landmarks(), b.landmarks())
        ia, ib = a.imu(), b.imu()
        for key in ia:
            assert np.array_equal(ia[key], ib[key]), key


def test_stale_after_changes(hip, oracle):
    w = imr.window("k4_tgas", oracle)
    with ha.Problem(w, lib=hip) as g:
        cross = np.zeros((w.n_cp, 6, g.dim_pose() - 6 * w.n_cp))
        stamp, out = np.array([0.5 * sum(w.valid_range())]), np.zeros((1, 6, 6))
        get = lambda: (g.lib.get_covariance(g.h, None, None, None, None), g.lib.get_covariance_cross(g.h, ha.problem._d(cross)),  # noqa: E731
                       g.lib.sample_sensor_covariance(g.h, ha.HS_SENSOR_IMU, 0, 1, ha.problem._d(stamp), ha.problem._d(out)))
        stale, fresh = (HS_ERR_STATE,) * 3, (0, 0, 0)
        g.set_imu_covariance(True)
        g.set_imu_estimation(True)
        assert get() == stale
        g.compute_covariance()
        assert get() == fresh and cross.any()
        m = dict(w.imu, i_g=np.asarray(w.imu["i_g"]) * (1.0 + 1e-3))
        a = [np.ascontiguousarray(m[k], dtype=np.float64) for k in ("T_bs", "i_g", "i_a", "S_g", "X_a")]
        bg, ba = np.ascontiguousarray(m["bias_g"], dtype=np.float64), np.ascontiguousarray(m["bias_a"], dtype=np.float64)
        assert g.lib.set_imu(g.h, *[ha.problem._d(x) for x in a], int(m["bias_order"]), float(m["bias_t0"]), float(m["bias_dt"]), bg.shape[0],
                             ha.problem._d(bg), ha.problem._d(ba), 0) == 0
        assert get() == stale
        g.compute_covariance()
        g.set_imu_constancy(imr.imu_flags("t"))
        assert get() == stale
        g.set_imu_constancy(imr.imu_flags("tgas"))
        g.compute_covariance()
        g.set_imu_covariance(False)
        assert get() == stale
        g.set_imu_covariance(True)
        assert get() == stale
        g.compute_covariance()
        assert get() == fresh
        g.solve(2)
        assert get() == stale
        g.compute_covariance()
        assert get() == fresh


def test_covariance_after_estimation_is_taken_at_the_estimate(hip, oracle):
    from test_gpu_imu_calibration_solve import oracle_window
    name = "k4_tgas"
    w = imr.window(name, oracle)
    lo, hi = w.valid_range()
    stamps = np.linspace(lo, hi, 7)[1:-1]
    with ha.Problem(w, lib=hip) as g:
        g.set_imu_estimation(True)
        g.set_imu_covariance(True)
        g.solve(5)
        g.compute_covariance()
        cov, bw = g.covariance(), g.lib.band_blocks(g.h)
        pose = g.sample_sensor_covariance(ha.HS_SENSOR_IMU, 0, stamps)
        we = oracle_window(w, g)
    we.imu_constant = w.imu_constant
    assert not np.array_equal(we.imu["T_bs"], w.imu["T_bs"]) and not np.array_equal(we.imu["i_a"], w.imu["i_a"])
    R, R0 = imr.referee(we, oracle), imr.window_referee(name, oracle)
    assert rel(R["Sigma"], R0["Sigma"]) > bar(R["cond"])  # (the estimate is another point: the referee at the initial values would not pass)
    compare(we, R, cov, bw)
    want = imr.sensor_pose_covariance(R["Sigma"], we, oracle, we.imu["T_bs"], stamps, R["P0"])  # (T_bs read at the estimate on the device)
    err = max(rel(a, b) for a, b in zip(pose, want))
    assert err < bar(R["cond"]), err
