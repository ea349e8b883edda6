"""CPU tests of tests/camera_model_referee.py, the referee of the pixel residual under a per-camera distortion model.

1. With the radial-tangential map the referee IS the oracle: rows, the five Jacobian blocks and the cost agree at 1e-12, robustified and not.
2. The numpy equidistant map, dd/dn and dd/dk against mpmath at 50 digits, absolute 1e-13, from the optical axis to plane radius 3.
3. Central differences of the referee's cost against its Jacobians (equidistant and mixed windows)."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import camera_model_referee as cmr
import camera_model_windows as cw

RHOS = (0.0, 1e-12, 1e-9, 1e-6, 1e-3, 0.1, 1.0, 2.0, 3.0)
ANGLES = (0.3, 1.9, 3.7, 5.5)
BLOCKS = ("r", "J_state", "J_landmark", "J_extrinsics", "J_intrinsics", "J_distortion")


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def equidistant_points(rhos=RHOS):
    return np.array([[r * np.cos(a), r * np.sin(a)] for r in rhos for a in ANGLES])


def test_equidistant_map_against_mpmath():
    n = equidistant_points()
    k = np.tile(cw.EQUI_DISTORTION[0], (len(n), 1))
    d, D, Dk = cmr.equidistant_map(n, k)
    worst = 0.0
    for i, (x, y) in enumerate(n):
        dv, DD, DDk = cmr.mp_equidistant(x, y, k[i])
        err = max(max(abs(float(d[i, c] - dv[c])) for c in range(2)),
                  max(abs(float(D[i, c, j] - DD[c][j])) for c in range(2) for j in range(2)),
                  max(abs(float(Dk[i, c, j] - DDk[c][j])) for c in range(2) for j in range(4)))
        worst = max(worst, err)
        assert err <= 1e-13, (x, y, err)
    print("equidistant map against mpmath: worst absolute error %.3g" % worst)
    assert np.isfinite(d).all() and np.isfinite(D).all() and np.isfinite(Dk).all()


@pytest.mark.parametrize("robustify", [False, True])
def test_radtan_referee_is_the_oracle(oracle, robustify):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3, with_priors=8)
    assert len(w.pixel_stamps) == 240
    with ha.Problem(w, lib=oracle) as o, cmr.RefereeProblem(w, oracle) as r:
        a, b = o.linearize(ha.HS_PIXEL, robustify, sensor_blocks=True), r.linearize(ha.HS_PIXEL, robustify, sensor_blocks=True)
        for key in BLOCKS + ("cost",):
            print(key, rel(b[key], a[key]))
            assert rel(b[key], a[key]) <= 1e-12, key
        assert np.array_equal(a["first_cp"], b["first_cp"])
        assert abs(r.cost() - o.cost()) <= 1e-12 * o.cost()
        assert (a["cost"] > 0.5 * 0.25).any() and (a["cost"] < 0.5 * 0.25).any()  # rows on both sides of the Huber threshold


def test_radtan_referee_drives_the_existing_referees(oracle):
    """Inside driving() the reduced-system referee opens RefereeProblems; with radial-tangential cameras it must return what it returns on the
    oracle itself."""
    import calibration_referee
    w = synthetic.small_visual(order=4, n_cp=14, n_landmarks=30, obs_pairs=3)
    w.cam_constant = np.array([[1, 0, 0], [1, 1, 1]], np.uint8)
    S0, g0 = calibration_referee.reduced_system(w, oracle)
    with cmr.driving():
        assert ha.Problem is not cmr._Base
        S1, g1 = calibration_referee.reduced_system(w, oracle)
    assert ha.Problem is cmr._Base
    assert rel(S1, S0) <= 1e-11 and rel(g1, g0) <= 1e-11


def _moved(w, which, idx, h):
    v = copy.copy(w)
    a = np.array(getattr(w, which), float).copy()
    a[idx] += h
    setattr(v, which, a)
    return v


@pytest.mark.parametrize("models", [(cw.EQUI, cw.EQUI), (cw.RADTAN, cw.EQUI)])
def test_central_differences_of_the_cost(oracle, models):
    """d cost_row / d x = J_row' r_row of the robustified rows (Ceres' corrector is exact for the gradient), row by row, for the Euclidean
    blocks: landmark, intrinsics, distortion and the translation of the extrinsics and of a control point. Huber's loss is C1 only: rows whose
    |r| lies within 0.01 of the threshold 0.5 are left out (a step of these sizes moves a pixel by far less), so the central difference is
    second order in h on every compared row; its rounding, eps * cost_row / h, stays below 1e-7 of the largest entry of a column."""
    w = cw.window(models, order=4, n_cp=12, n_landmarks=12, obs_pairs=2, seed=3)
    with cmr.RefereeProblem(w, oracle) as p:
        L = p.linearize(ha.HS_PIXEL, True, sensor_blocks=True)
        raw = p.linearize(ha.HS_PIXEL, False)["r"]
    lm, cam, first = np.asarray(w.pixel_landmark, int), np.asarray(w.pixel_camera, int), L["first_cp"]
    smooth = np.abs(np.linalg.norm(raw, axis=1) - cmr.HUBER_PIXEL) > 1e-2
    assert smooth.sum() >= 0.9 * len(raw) and (np.linalg.norm(raw, axis=1) > 0.5).any()
    grad = lambda J: np.einsum("nrc,nr->nc", J, L["r"])

    def fd(which, idx, h):
        with cmr.RefereeProblem(_moved(w, which, idx, h), oracle) as a, cmr.RefereeProblem(_moved(w, which, idx, -h), oracle) as b:
            return (a.linearize(ha.HS_PIXEL, False)["cost"] - b.linearize(ha.HS_PIXEL, False)["cost"]) / (2 * h)

    checks = []
    for l in (0, 5):
        checks += [("landmark", fd("landmarks", (l, c), 1e-6), np.where(lm == l, grad(L["J_landmark"])[:, c], 0.0)) for c in range(3)]
    for c in (0, 1):
        on = cam == c
        checks += [("intrinsics", fd("cam_intrinsics", (c, j), 1e-5), np.where(on, grad(L["J_intrinsics"])[:, j], 0.0)) for j in range(4)]
        checks += [("distortion", fd("cam_distortion", (c, j), 1e-7), np.where(on, grad(L["J_distortion"])[:, j], 0.0)) for j in range(4)]
        checks += [("t_bs", fd("cam_T_bs", (c, 4 + j), 1e-6), np.where(on, grad(L["J_extrinsics"])[:, 3 + j], 0.0)) for j in range(3)]
    for j in range(3):
        ana = np.zeros(len(lm))
        for i in range(w.order):
            ana += np.where(first + i == 5, grad(L["J_state"][:, :, 6 * i:6 * i + 6])[:, 3 + j], 0.0)
        checks.append(("p_cp", fd("control_points", (5, 4 + j), 1e-6), ana))
    for name, num, ana in checks:
        assert np.abs(ana[smooth]).max() > 0
        err = np.abs(num - ana)[smooth].max() / np.abs(ana[smooth]).max()
        assert err <= 1e-6, (name, err)


def test_windows_span_the_plane(oracle):
    """The windows of the device tests span the plane from the optical axis to beyond radius 1.5: the generated window covers the wide
    field, the axis window has rows exactly on the axis."""
    w = cw.window(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    rho = cw.plane_radii(w, oracle)
    assert rho.min() < 0.5 and rho.max() >= 1.5, (rho.min(), rho.max())
    rho = cw.plane_radii(cw.axis_window(), oracle)
    assert (rho == 0.0).sum() >= 4, np.sort(rho)[:6]


def test_oracle_raises_only_for_a_model_it_does_not_know(oracle):
    w = synthetic.small_visual(order=4, n_cp=12, n_landmarks=10, obs_pairs=2)
    w.cam_models = np.zeros(2, np.int32)
    ha.Problem(w, lib=oracle).close()
    w.cam_models = np.array([cw.RADTAN, cw.EQUI], np.int32)
    with pytest.raises(ha.HsError, match="set_camera_models: not provided by this library"):
        ha.Problem(w, lib=oracle)
