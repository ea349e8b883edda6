"""CPU pins of the covariance referee with free IMU blocks (tests/imu_covariance_referee.py), and the admissibility of every window
tests/test_gpu_imu_covariance.py uses — decided from CPU quantities alone, before a device is consulted:
  * with every IMU block constant the referee equals the camera referee (tests/camera_covariance_referee.py) at 1e-10;
  * the IMU columns sit where hs_reduced_system puts them, for subsets of the five blocks;
  * T_bs and X_a both free: the scaled reduced matrix is singular (smallest eigenvalue ~1e-19 against ~1e-10 of the admissible subsets) and the
    null vector lives on the three translation columns and the nine X_a columns — why hs_compute_covariance refuses the pair on the host;
  * admissibility, by the project's two rules: cond of the Jacobi-scaled reduced matrix with the blocks free at most twice that with them
    constant, and Sigma_ii and the IMU columns of Sigma_pi, recomputed under a symmetric relative perturbation of 1e-13 (five draws, fixed
    seed), move by less than bar(cond) / 10 relative to each block's own max-norm;
  * the extrinsics Jacobian of the sensor-pose referee equals central differences through the oracle's manifold_plus(HS_MANIFOLD_SE3).
A window that fails a condition is a defect of the window choice: it is replaced, the bar is not widened (k5 "ta" was: ratio 2.02)."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import camera_covariance_referee as ccr
import imu_calibration_referee as icr
import imu_covariance_referee as imr
from imu_covariance_referee import bar, rel


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    import os
    from hyperslam_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hyperslam_hip.h")).read()
    lib = ctypes.CDLL(_lib.PRODUCT_LIB)
    for sym in ("hs_set_imu_covariance", "hs_sample_sensor_covariance"):
        assert sym + "(" in header and sym in _lib.ABI_SYMBOLS and hasattr(lib, sym), sym
    for i, name in enumerate(("HS_SENSOR_CAMERA", "HS_SENSOR_IMU", "HS_SENSOR_PLAIN")):
        assert f"#define {name} {i}\n" in header and getattr(ha, name) == i


def test_python_calls_are_refused_for_the_oracle(oracle):
    w = imr.constant_blocks(imr.window("k4_t", oracle))
    with ha.Problem(w, lib=oracle) as c:
        with pytest.raises(ha.problem.HsError, match="set_imu_covariance: not provided by this library"):
            c.set_imu_covariance(True)
        with pytest.raises(ha.problem.HsError, match="sample_sensor_covariance: not provided by this library"):
            c.sample_sensor_covariance(ha.HS_SENSOR_IMU, 0, [0.5])


@pytest.mark.parametrize("cams", [{}, dict(cam1="tid")])
def test_constant_imu_blocks_equal_the_camera_referee(cams, oracle):
    w = imr.constant_blocks(imr.window("k4_t", oracle))
    if cams:
        w.cam_constant = ccr.flags(w, **cams)
    R, C = imr.referee(w, oracle), ccr.referee(w, oracle)
    assert R["ni"] == 0 and R["Sigma"].shape == C["Sigma"].shape
    assert rel(R["Sigma"], C["Sigma"]) < 1e-10, rel(R["Sigma"], C["Sigma"])
    ok = ~np.isnan(C["lm_cov"])
    assert np.array_equal(np.isnan(R["lm_cov"]), ~ok)
    assert rel(R["lm_cov"][ok], C["lm_cov"][ok]) < 1e-10
    assert abs(R["cond"] / C["cond"] - 1.0) < 1e-6


@pytest.mark.parametrize("free", ["t", "gx", "as", "tgas"])
def test_column_layout_is_that_of_the_reduced_system(free, oracle):
    """The undamped, unscaled J'J of the assembly against tests/imu_calibration_referee.py::reduced_system (the pin of hs_reduced_system's
    column order), which scales and damps: their IMU / camera blocks agree once its scale is divided out and the radius is huge."""
    w = copy.copy(imr.window("k4_ga_cam1tid", oracle))
    w.imu_constant = imr.imu_flags(free)
    A = imr.assemble(w, oracle)
    ni = sum(icr.IMU_BLOCKS["tgasx".index(b)][1] for b in free)
    assert A["ni"] == ni and A["nc"] == 14 and A["P"] == A["P0"] + ni + 14
    S, _ = icr.reduced_system(w, oracle, radius=1e300)
    M, d = ccr.scaled_reduced(A)
    fi = np.flatnonzero(A["free"])
    tail = np.flatnonzero(fi >= A["P0"])  # IMU and camera columns inside the free ones
    got, want = M[np.ix_(tail, tail)], S[np.ix_(fi[tail], fi[tail])]
    assert rel(got, want) < 1e-9, rel(got, want)
    cross_got, cross_want = M[:, tail], S[np.ix_(fi, fi[tail])]
    assert rel(cross_got, cross_want) < 1e-9, rel(cross_got, cross_want)


@pytest.mark.parametrize("mode", [ha.HS_INERTIAL_AS_REFERENCE, ha.HS_INERTIAL_EXACT])
def test_extrinsic_translation_and_acc_offsets_are_dependent(mode, oracle):
    w = copy.copy(imr.window("k4_t", oracle))
    admissible = []
    for free in ("t", "tgas", "gasx", "x"):
        w.imu_constant = imr.imu_flags(free)
        admissible.append(imr.smallest_eigenvalue(w, oracle, mode)[0])
    for free in ("tx", "tgasx"):
        w.imu_constant = imr.imu_flags(free)
        val, v, A = imr.smallest_eigenvalue(w, oracle, mode)
        cols, _ = icr.imu_columns(w)
        twelve = A["P0"] + np.r_[cols[3:6], cols[27:36]]  # translation of T_bs, X_a
        outside = np.delete(v, twelve)
        print(f"mode {mode} {free}: smallest eigenvalue {val:.3g} (admissible subsets: {min(admissible):.3g}), null vector outside the twelve columns {np.abs(outside).max():.3g}")
        assert abs(val) < 1e-6 * min(admissible), (val, admissible)
        assert np.linalg.norm(outside) < 1e-6 * np.linalg.norm(v[twelve]), np.linalg.norm(outside)


@pytest.mark.parametrize("name", imr.WINDOWS)
def test_window_is_admissible(name, oracle):
    w = imr.window(name, oracle)
    R = imr.window_referee(name, oracle)
    cond = R["cond"]
    assert R["ni"] > 0 and np.isfinite(cond)
    cond_const = np.linalg.cond(ccr.scaled_reduced(imr.assemble(imr.constant_blocks(w), oracle))[0])
    print(f"{name}: cond {cond:.3g} (constant blocks {cond_const:.3g}, ratio {cond / cond_const:.3g})")
    assert cond <= 2.0 * cond_const, (cond, cond_const)
    pi, ii = imr.perturbation_response(R, w.n_cp)
    print(f"{name}: response of Sigma_pi {pi:.3g}, Sigma_ii {ii:.3g} to 1e-13; bar / 10 = {bar(cond) / 10:.3g}")
    assert max(pi, ii) < bar(cond) / 10.0, (pi, ii, bar(cond))
    if R["nc"]:
        pc, cc = ccr.perturbation_response(R, w.n_cp)
        print(f"{name}: response of Sigma_pc {pc:.3g}, Sigma_cc {cc:.3g}")
        assert max(pc, cc) < bar(cond) / 10.0, (pc, cc, bar(cond))


def test_extrinsics_jacobian_of_the_sensor_pose_equals_central_differences(oracle):
    """r(delta) = prior residual of the sensor Plus(T_bs, delta) against the measurement T_wb(t) o T_bs; J_e = d r / d delta at 0. The residual
    is recomputed by the oracle (hs_linearize on a window whose plain sensor is the perturbed T_bs)."""
    w = imr.window("k4_t", oracle)
    T_bs = np.asarray(w.imu["T_bs"], float)
    lo, hi = w.valid_range()
    stamps = np.array([lo + 1e-3, 0.5 * (lo + hi), hi - 1e-3])
    Js, Je, first = imr.sensor_pose_jacobians(w, oracle, T_bs, stamps)
    assert Js.shape == (3, 6, 6 * w.order) and Je.shape == (3, 6, 6)
    wp = ha.Window(order=w.order, t0=w.t0, dt=w.dt, control_points=np.array(w.control_points, float))
    with ha.Problem(wp, lib=oracle) as c:
        body = c.sample_trajectory(stamps)
        q, p = synthetic.compose(body[:, :4], body[:, 4:], np.broadcast_to(T_bs[:4], (3, 4)), np.broadcast_to(T_bs[4:], (3, 3)))
        meas = np.concatenate([q, p], -1)
        h = 1e-6
        num = np.zeros_like(Je)
        for j in range(6):
            r = []
            for sgn in (1.0, -1.0):
                delta = np.zeros(6)
                delta[j] = sgn * h
                wq = copy.copy(wp)
                wq.sensor_T_bs = c.manifold_plus(ha.HS_MANIFOLD_SE3, T_bs[None, :], delta[None, :])
                wq.prior_stamps, wq.prior_poses, wq.prior_sensor = stamps, meas, np.zeros(3, np.int32)
                with ha.Problem(wq, lib=oracle) as e:
                    r.append(e.linearize(ha.HS_PRIOR, True)["r"])
            num[:, :, j] = (r[0] - r[1]) / (2.0 * h)
    assert rel(Je, num) < 1e-8, rel(Je, num)
