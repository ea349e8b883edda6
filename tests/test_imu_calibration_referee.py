"""Pins the numpy referee of tests/imu_calibration_referee.py (CPU only, no GPU).

1. With every IMU block constant it is the referee of tests/calibration_referee.py (which tests/test_calibration_referee.py pins to the oracle)
   to 1e-10 relative, with and without free cameras.
2. The column layout for every subset of the five flags.
3. The IMU part of the gradient J'r equals the derivative of the oracle's cost along each free IMU coordinate (central differences: T_bs
   through hs_manifold_plus, the rest additive) — what ties coordinates and signs to something other than the Jacobian code. In both
   Jacobian modes at the identity IMU, where they coincide; off it in HS_INERTIAL_EXACT, the mode that is the derivative of the prediction."""
import copy
import itertools

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import calibration_referee as cref
import imu_calibration_referee as ref


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def windows():
    yield "pixel_k4", synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    yield "inertial_k4", synthetic.small_inertial(order=4, n_cp=16)
    w = synthetic.small_inertial(order=6, n_cp=18, seed=5)
    w.cam_constant = np.array([[0, 1, 1], [0, 0, 0]], np.uint8)
    yield "inertial_k6_free_cameras", w
    w = synthetic.small_visual(order=5, n_cp=18, n_landmarks=40, obs_pairs=4, seed=22, with_priors=30)
    w.cam_constant = np.array([[1, 1, 1], [0, 0, 0]], np.uint8)
    yield "pixel_prior_k5_free_camera", w


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
@pytest.mark.parametrize("flags", [None, np.ones(5, np.uint8)], ids=["none", "all_set"])
def test_constant_imu_blocks_reproduce_the_camera_referee(name, w, flags, oracle):
    w = copy.copy(w)
    w.imu_constant = flags
    S, g = ref.reduced_system(w, oracle, 1e4)
    Sc, gc = cref.reduced_system(w, oracle, 1e4)
    assert S.shape == Sc.shape
    assert rel(S, Sc) < 1e-10, rel(S, Sc)
    assert rel(g, gc) < 1e-10, rel(g, gc)


def test_imu_columns_layout_for_every_subset():
    w = synthetic.small_inertial(order=4, n_cp=16)
    sizes = (6, 6, 6, 9, 9)
    for const in itertools.product((0, 1), repeat=5):
        w.imu_constant = np.array(const, np.uint8)
        cols, ni = ref.imu_columns(w)
        assert ni == sum(s for s, c in zip(sizes, const) if not c)
        want, n = [], 0
        for s, c in zip(sizes, const):
            want += [-1] * s if c else list(range(n, n + s))
            n += 0 if c else s
        assert list(cols) == want, const
    w.imu_constant = np.zeros(5, np.uint8)
    assert ref.imu_columns(w)[1] == 36
    w.imu_constant = None
    assert ref.imu_columns(w)[1] == 0
    # a window without inertial rows leaves the IMU columns out
    w.imu_constant = np.zeros(5, np.uint8)
    w.inertial_stamps, w.inertial_measurements = np.zeros(0), np.zeros((0, 6))
    assert ref.imu_columns(w)[1] == 0
    v = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    v.imu_constant = np.zeros(5, np.uint8)
    assert ref.imu_columns(v)[1] == 0


def test_columns_sit_between_gravity_and_the_cameras(oracle):
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.imu_constant = np.array([1, 0, 1, 1, 0], np.uint8)  # i_g + X_a: 15
    w.cam_constant = np.array([[0, 1, 1], [1, 1, 1]], np.uint8)  # cam0 T_bs: 6
    P0, ni, nc = ref.layout(w, oracle)
    assert (ni, nc) == (15, 6)
    S, g = ref.reduced_system(w, oracle, 1e4)
    assert S.shape == (P0 + 21, P0 + 21)
    wc = copy.copy(w)
    wc.imu_constant = None
    Sc, gc = cref.reduced_system(wc, oracle, 1e4)
    keep = np.r_[np.arange(P0), P0 + 15 + np.arange(6)]  # dropping the IMU columns leaves the camera referee's system
    assert rel(S[np.ix_(keep, keep)], Sc) < 1e-10
    assert rel(g[keep], gc) < 1e-10
    assert np.all(S[P0:P0 + 15, P0 + 15:] == 0.0)  # IMU x camera: no residual touches both
    assert np.abs(S[6 * w.n_cp:P0, P0:P0 + 15]).max() > 0.0  # bias / gravity x IMU is not zero


def perturbed(w, c, d):
    """The window with the IMU parameters moved by the 36 local coordinates d."""
    w2 = copy.copy(w)
    w2.imu = dict(w.imu)
    w2.imu_constant = None
    w2.imu["T_bs"] = c.manifold_plus(ha.HS_MANIFOLD_SE3, np.asarray(w.imu["T_bs"], float)[None, :], d[None, :6])[0]
    for key, (first, size) in zip(("i_g", "i_a", "S_g", "X_a"), ref.IMU_BLOCKS[1:]):
        w2.imu[key] = np.asarray(w.imu[key], float) + d[first:first + size]
    return w2


@pytest.mark.parametrize("identity,mode", [(True, ha.HS_INERTIAL_AS_REFERENCE), (True, ha.HS_INERTIAL_EXACT), (False, ha.HS_INERTIAL_EXACT)],
                         ids=["identity_as_reference", "identity_exact", "general_exact"])
def test_imu_gradient_matches_finite_differences(identity, mode, oracle):
    """g_i before scaling is J_i' r = d cost / d x_i (no landmark touches an IMU column: nothing is eliminated from it). Protocol and bar of
    test_camera_gradient_matches_finite_differences: eps 1e-6, 1e-5 * max(1, |g|)."""
    w = synthetic.small_inertial(order=4, n_cp=12, n_landmarks=20, obs_pairs=3, n_inertial=60, seed=3, identity=identity)
    w.imu_constant = np.zeros(5, np.uint8)
    S, g = ref.reduced_system(w, oracle, 1e300, mode)
    P0, ni, nc = ref.layout(w, oracle)
    assert (ni, nc) == (36, 0)
    # recover the unscaled gradient: g = s * J'r with s = 1 / (1 + sqrt(diag J'J)) and diag J'J from the undamped diagonal of S
    Sd = np.diag(S)[P0:]
    gi = np.zeros(ni)
    for j in range(ni):
        if Sd[j] != 1.0:  # s^2 h = Sd (undamped at radius 1e300): sqrt h = sqrt(Sd) / (1 - sqrt(Sd))
            r = np.sqrt(Sd[j])
            gi[j] = g[P0 + j] * (1.0 + r / (1.0 - r))
    eps = 1e-6
    w_plain = copy.copy(w)
    w_plain.imu_constant = None
    worst = 0.0
    with ha.Problem(w_plain, lib=oracle) as c:
        for j in range(ni):
            vals = []
            for sgn in (1, -1):
                d = np.zeros(36)
                d[j] = sgn * eps
                with ha.Problem(perturbed(w, c, d), lib=oracle) as c2:
                    vals.append(c2.cost())
            fd = (vals[0] - vals[1]) / (2 * eps)
            worst = max(worst, abs(fd - gi[j]) / max(1.0, abs(gi[j])))
            assert abs(fd - gi[j]) <= 1e-5 * max(1.0, abs(gi[j])), (j, fd, gi[j])
    print("worst relative finite-difference mismatch:", worst)
