"""CPU pins of the covariance referee with free camera blocks (tests/camera_covariance_referee.py), and the admissibility of every window
tests/test_gpu_camera_covariance.py uses — decided from CPU quantities alone, before a device is consulted:
  * with every camera constant the referee equals tests/test_gpu_covariance.py::referee (1e-10);
  * the block formula of DESIGN §12, Sigma_ll = S_l L^-T (I + G' Sigma_[p_l,c] G) L^-1 S_l with G = [Yh ; Y_c'], evaluated in numpy from the
    same rows, equals the landmark blocks of the full inverse at bar(cond);
  * visual-only windows have cond < 1e7; windows with an IMU a cond of at most twice that of the same window with constant cameras;
  * Sigma_cc and the camera columns of Sigma_pc, recomputed from the scaled reduced matrix under a symmetric relative perturbation of 1e-13
    (five draws, fixed seed), move by less than bar(cond) / 10 relative to each block's own max-norm — the camera blocks are up to 1e-6 of the
    whole Sigma in max-norm, so the GPU test compares them per block, and that comparison must not rest on the referee's own rounding.
A window that fails a condition is a defect of the window choice: it is replaced, the bar is not widened."""
import numpy as np
import pytest

import hyperslam_amd as ha

import camera_covariance_referee as ccr
from camera_covariance_referee import bar, rel


def test_new_symbols_are_declared_bound_and_exported():
    import ctypes
    import os
    from hyperslam_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "hyperslam_hip.h")).read()
    lib = ctypes.CDLL(_lib.PRODUCT_LIB)
    for sym in ("hs_set_camera_covariance", "hs_get_covariance_cross"):
        assert sym + "(" in header and sym in _lib.ABI_SYMBOLS and hasattr(lib, sym), sym


def test_python_switch_is_refused_for_the_oracle(oracle):
    w, _ = ccr.window("A", oracle)
    with ha.Problem(ccr.constant_cameras(w), lib=oracle) as c:
        with pytest.raises(ha.problem.HsError, match="set_camera_covariance: not provided by this library"):
            c.set_camera_covariance(True)


@pytest.mark.parametrize("name", ["D", "bearing", "rotation_constant", "translation_constant", "F"])
def test_constant_cameras_equal_the_covariance_referee(name, oracle):
    """Full dense inverse here, Schur complement and block inverse there: the same numbers. On the visual windows with a frozen prefix: 1e-10 is
    a statement about two float64 computations of cond ~1e4 .. 1e5 (with constant cameras), not about the windows with an IMU (cond 3e10 and
    more) or those whose gauge only the priors hold (A, B: the two referees agree to 3e-10 / 1e-9 there, their own rounding)."""
    from test_gpu_covariance import referee as schur_referee
    wc = ccr.constant_cameras(ccr.window(name, oracle)[0])
    R = ccr.referee(wc, oracle)
    Sigma, lm_cov, cond = schur_referee(wc, oracle)
    assert R["nc"] == 0 and R["Sigma"].shape == Sigma.shape
    assert rel(R["Sigma"], Sigma) < 1e-10, rel(R["Sigma"], Sigma)
    assert np.array_equal(np.isnan(R["lm_cov"]), np.isnan(lm_cov))
    ok = ~np.isnan(lm_cov)
    assert rel(R["lm_cov"][ok], lm_cov[ok]) < 1e-10, rel(R["lm_cov"][ok], lm_cov[ok])
    assert abs(R["cond"] / cond - 1.0) < 1e-6, (R["cond"], cond)


@pytest.mark.parametrize("name", ccr.WINDOWS)
def test_block_formula_equals_the_full_inverse(name, oracle):
    R = ccr.window_referee(name, oracle)
    got, want = ccr.block_formula(R["A"], R["Sigma"]), R["lm_cov"]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    err = rel(got[ok], want[ok])
    print(f"{name}: block formula vs full inverse {err:.3g}, bar {bar(R['cond']):.3g}")
    assert err < bar(R["cond"]), (err, bar(R["cond"]))


@pytest.mark.parametrize("name", ccr.WINDOWS)
def test_window_is_admissible(name, oracle):
    w, imu = ccr.window(name, oracle)
    R = ccr.window_referee(name, oracle)
    cond = R["cond"]
    assert R["nc"] > 0 and np.isfinite(cond)
    if imu:
        cond_const = np.linalg.cond(ccr.scaled_reduced(ccr.assemble(ccr.constant_cameras(w), oracle))[0])
        print(f"{name}: cond {cond:.3g} (constant cameras {cond_const:.3g})")
        assert cond <= 2.0 * cond_const, (cond, cond_const)
    else:
        print(f"{name}: cond {cond:.3g}")
        assert cond < 1e7, cond
    pc, cc = ccr.perturbation_response(R, w.n_cp)
    print(f"{name}: response of Sigma_pc {pc:.3g}, Sigma_cc {cc:.3g} to 1e-13; bar / 10 = {bar(cond) / 10:.3g}")
    assert max(pc, cc) < bar(cond) / 10.0, (pc, cc, bar(cond))
