"""Pins the numpy referee of tests/calibration_referee.py (CPU only, no GPU).

With every camera block constant the referee's reduced system is the oracle's own (hs_reduced_system of the CPU restatement) to 1e-10
relative; with free camera blocks its camera columns match a finite-difference Gauss-Newton check: the camera part of J'r before the
Schur complement equals the gradient of the oracle's cost along each free coordinate."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import calibration_referee as ref


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def windows():
    yield "pixel_k4", synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    yield "pixel_prior_k5", synthetic.small_visual(order=5, n_cp=18, n_landmarks=40, obs_pairs=4, seed=22, with_priors=30)
    wb = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, bearing=True, seed=9)
    wb.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(12, np.uint8)]
    yield "bearing_frozen_k4", wb
    wl = synthetic.small_visual(order=6, n_cp=20, n_landmarks=50, obs_pairs=3, seed=8)
    wl.landmark_constant = (np.arange(50) % 5 == 0).astype(np.uint8)
    yield "pixel_const_landmarks_k6", wl
    yield "inertial_k4", synthetic.small_inertial(order=4, n_cp=16)


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
def test_constant_cameras_reproduce_the_oracle(name, w, oracle):
    S, g = ref.reduced_system(w, oracle, 1e4)
    with ha.Problem(w, lib=oracle) as c:
        Sc, gc = c.reduced_system(1e4)
    assert S.shape == Sc.shape
    assert rel(S, Sc) < 1e-10, rel(S, Sc)
    assert rel(g, gc) < 1e-10, rel(g, gc)


def test_camera_columns_layout():
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    n_cam = len(w.cam_T_bs)
    w.cam_constant = np.ones((n_cam, 3), np.uint8)
    assert ref.camera_columns(w)[1] == 0
    w.cam_constant[1] = 0
    w.cam_constant[0, 1:] = 0
    cols, n = ref.camera_columns(w)
    assert n == 22
    assert list(cols[0]) == [-1] * 6 + list(range(8))
    assert list(cols[1]) == list(range(8, 22))
    w.pixel_camera = np.zeros_like(w.pixel_camera)  # camera 1 referenced by no row: left out
    assert ref.camera_columns(w)[1] == 8


@pytest.mark.parametrize("bearing", [False, True])
def test_camera_gradient_matches_finite_differences(bearing, oracle):
    """g_c before scaling and elimination is J_c' r = d cost / d x_c: checked against central differences of the oracle's cost along
    every free coordinate of camera 1 (T_bs on its SE3 manifold, intrinsics and distortion additive)."""
    w = synthetic.small_visual(order=4, n_cp=12, n_landmarks=20, obs_pairs=3, bearing=bearing, seed=3)
    n_cam = len(w.cam_T_bs)
    w.cam_constant = np.ones((n_cam, 3), np.uint8)
    w.cam_constant[1] = 0
    # constant landmarks: nothing is eliminated, the referee's camera gradient is s_c * J_c'r
    w.landmark_constant = np.ones(len(w.landmarks), np.uint8)
    S, g = ref.reduced_system(w, oracle, 1e300)
    _, nc = ref.camera_columns(w)
    assert nc == 14
    P0 = 6 * w.n_cp
    Hd = np.zeros(nc)
    # recover the unscaled gradient: g = s * J'r with s = 1 / (1 + sqrt(diag J'J)) and diag J'J from the undamped diagonal of S
    Sd = np.diag(S)[P0:]
    s = np.where(Sd == 1.0, 1.0, 0.0)
    for j in range(nc):
        if Sd[j] != 1.0:  # s^2 h = Sd (undamped at radius 1e300) with s = 1 / (1 + sqrt h): sqrt h = sqrt(Sd) / (1 - sqrt(Sd))
            r = np.sqrt(Sd[j])
            Hd[j] = (r / (1.0 - r)) ** 2
            s[j] = 1.0 / (1.0 + np.sqrt(Hd[j]))
    gc = np.where(s > 0, g[P0:] / s, 0.0)
    eps = 1e-6
    w_plain = copy.copy(w)
    w_plain.cam_constant = None
    with ha.Problem(w_plain, lib=oracle) as c:
        for j in range(nc):
            vals = []
            for sgn in (1, -1):
                w2 = copy.deepcopy(w)
                w2.cam_constant = None
                d = np.zeros(14)
                d[j] = sgn * eps
                T = c.manifold_plus(ha.HS_MANIFOLD_SE3, w.cam_T_bs[1:2], d[None, :6])[0]
                w2.cam_T_bs[1] = T
                w2.cam_intrinsics[1] = w.cam_intrinsics[1] + d[6:10]
                w2.cam_distortion[1] = w.cam_distortion[1] + d[10:14]
                with ha.Problem(w2, lib=oracle) as c2:
                    vals.append(c2.cost())
            fd = (vals[0] - vals[1]) / (2 * eps)
            assert abs(fd - gc[j]) <= 1e-5 * max(1.0, abs(gc[j])), (j, fd, gc[j])
