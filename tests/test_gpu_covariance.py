"""Marginal covariances on the GPU (hs_compute_covariance / hs_get_covariance / hs_sample_covariance) against numpy.

The referee is independent of every device build path: the oracle's robustified rows (hs_linearize: r, J_state, J_landmark, J_bias_*,
J_gravity, first_cp, first_bias) are assembled into J'J, constant columns dropped, landmarks eliminated by a numpy Schur complement and the
reduced matrix inverted densely; landmark blocks follow from the block inverse. Bar: 1e-8 relative max-norm, or cond * 1e-14 for a window
whose Jacobi-scaled reduced matrix has a condition number above 1e6."""
import ctypes as C
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

pytestmark = pytest.mark.gpu

HS_ERR_STATE, HS_ERR_NUMERIC = 3, 4


def referee(w, oracle):
    """Dense covariance of the reduced unknowns (control points + border) and the landmark blocks, from the oracle's rows."""
    with ha.Problem(w, lib=oracle) as c:
        k, n_cp, n_lm = w.order, w.n_cp, len(w.landmarks)
        P = c.dim_pose()
        nb = P - 6 * n_cp
        n_bias = (nb - 2) // 6 if nb else 0
        Hpp, Hll, Hpl = np.zeros((P, P)), np.zeros((n_lm, 3, 3)), np.zeros((n_lm, P, 3))

        def add_pp(idx, J):
            np.add.at(Hpp, (idx[:, :, None], idx[:, None, :]), np.einsum("nri,nrj->nij", J, J))

        for ftype, lm_of in ((ha.HS_PIXEL, w.pixel_landmark), (ha.HS_BEARING, w.bearing_landmark)):
            if c.num_residuals(ftype) == 0:
                continue
            L = c.linearize(ftype, True)
            idx = 6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :]
            Js, Jl, lm = L["J_state"], L["J_landmark"], np.asarray(lm_of)
            add_pp(idx, Js)
            np.add.at(Hll, lm, np.einsum("nri,nrj->nij", Jl, Jl))
            np.add.at(Hpl, (lm[:, None], idx), np.einsum("nri,nrj->nij", Js, Jl))
        if c.num_residuals(ha.HS_PRIOR):
            L = c.linearize(ha.HS_PRIOR, True)
            add_pp(6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :], L["J_state"])
        if c.num_residuals(ha.HS_INERTIAL):
            L = c.linearize(ha.HS_INERTIAL, True)
            kb = int(w.imu["bias_order"])
            f, fb = L["first_cp"][:, None], L["first_bias"][:, None]
            idx = np.concatenate([6 * f + np.arange(6 * k), 6 * n_cp + 3 * fb + np.arange(3 * kb), 6 * n_cp + 3 * n_bias + 3 * fb + np.arange(3 * kb),
                                  np.broadcast_to(6 * n_cp + 6 * n_bias + np.arange(2), (len(f), 2))], 1)
            add_pp(idx, np.concatenate([L["J_state"], L["J_bias_g"], L["J_bias_a"], L["J_gravity"]], 2))
    free = np.ones(P, bool)
    cpc = np.zeros(n_cp, bool) if w.cp_constant is None else np.asarray(w.cp_constant, bool)
    for i in range(n_cp):
        free[6 * i:6 * i + 3] &= not (cpc[i] or w.rotation_constant)
        free[6 * i + 3:6 * i + 6] &= not (cpc[i] or w.translation_constant)
    if nb:
        free[6 * n_cp:6 * n_cp + 6 * n_bias] = not w.imu.get("bias_constant", False)
        free[6 * n_cp + 6 * n_bias:] = not w.gravity_constant
    lmc = np.zeros(n_lm, bool) if w.landmark_constant is None else np.asarray(w.landmark_constant, bool)
    observed = np.zeros(n_lm, bool)
    observed[np.asarray(w.pixel_landmark, int)] = True
    observed[np.asarray(w.bearing_landmark, int)] = True
    act = observed & ~lmc
    Hpl[:, ~free, :] = 0.0
    Hll_inv = np.linalg.inv(Hll[act])
    W = Hpl[act] @ Hll_inv
    S = Hpp - np.tensordot(W, Hpl[act], axes=([0, 2], [0, 2]))
    Sf = S[np.ix_(free, free)]
    d = 1.0 / (1.0 + np.sqrt(np.diag(Hpp)[free]))  # the solver's Jacobi scaling
    cond = np.linalg.cond(Sf * d[:, None] * d[None, :])
    Sigma = np.zeros((P, P))
    Sigma[np.ix_(free, free)] = np.linalg.inv(Sf)
    lm_cov = np.zeros((n_lm, 3, 3))
    lm_cov[~observed] = np.nan
    lm_cov[act] = Hll_inv + np.einsum("lpi,pq,lqj->lij", W, Sigma, W)
    return Sigma, lm_cov, cond


def bar(cond):
    return max(1e-8, cond * 1e-14)


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def check_window(w, hip, oracle, landmarks=None):
    Sigma, lm_ref, cond = referee(w, oracle)
    tol = bar(cond)
    n_cp = w.n_cp
    with ha.Problem(w, lib=hip) as g:
        bw = g.lib.band_blocks(g.h)
        g.compute_covariance()
        cov = g.covariance()
    blocks = np.stack([Sigma[6 * i:6 * i + 6, 6 * i:6 * i + 6] for i in range(n_cp)])
    band = np.zeros((n_cp, bw, 6, 6))
    for i in range(n_cp):
        for j in range(min(bw, n_cp - i)):
            band[i, j] = Sigma[6 * i:6 * i + 6, 6 * (i + j):6 * (i + j) + 6]
    assert rel(cov["control_points"], blocks) < tol, (rel(cov["control_points"], blocks), tol)
    assert rel(cov["control_point_band"], band) < tol, (rel(cov["control_point_band"], band), tol)
    if Sigma.shape[0] > 6 * n_cp:
        B = Sigma[6 * n_cp:, 6 * n_cp:]
        assert rel(cov["border"], B) < tol, (rel(cov["border"], B), tol)
    sel = np.arange(len(w.landmarks)) if landmarks is None else landmarks
    got, want = cov["landmarks"][sel], lm_ref[sel]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert rel(got[ok], want[ok]) < tol, (rel(got[ok], want[ok]), tol)
    return cov


@pytest.mark.parametrize("order", [4, 5, 6])
def test_small_visual_with_priors(order, hip, oracle):
    check_window(synthetic.small_visual(order=order, n_cp=16, n_landmarks=40, with_priors=16), hip, oracle)


def inertial_window(order, oracle):
    """small_inertial with a frozen prefix (gauge) and without the trailing bias control point no inertial row reaches (a free coordinate
    without information: hs_compute_covariance would refuse the window)."""
    w = synthetic.small_inertial(order=order, n_cp=18)
    w.cp_constant = np.r_[np.ones(order, np.uint8), np.zeros(18 - order, np.uint8)]
    with ha.Problem(w, lib=oracle) as c:
        used = int(c.linearize(ha.HS_INERTIAL, True)["first_bias"].max()) + int(w.imu["bias_order"])
    w.imu["bias_g"], w.imu["bias_a"] = w.imu["bias_g"][:used], w.imu["bias_a"][:used]
    return w


@pytest.mark.parametrize("order", [4, 6])
def test_small_inertial_border(order, hip, oracle):
    check_window(inertial_window(order, oracle), hip, oracle)


@pytest.mark.parametrize("order,n_cp,obs_pairs,span", [(4, 24, 3, 1.0), (4, 64, 3, 1.0), (4, 40, 3, 2.2)])
def test_frozen_prefix_and_band_shapes(order, n_cp, obs_pairs, span, hip, oracle):
    """Sliding-window shape (frozen prefix, small system: the solver's one-launch dense path), a long window (the solver factors it from both
    ends) and long tracks (band wider than 14 control points): one natural-order factor serves them all."""
    w = synthetic.small_visual(order=order, n_cp=n_cp, n_landmarks=3 * n_cp, obs_pairs=obs_pairs, span=span, with_priors=n_cp)
    w.cp_constant = np.r_[np.ones(order, np.uint8), np.zeros(n_cp - order, np.uint8)]
    check_window(w, hip, oracle)


def test_configs1_shaped_window(hip, oracle):
    w = synthetic.config1()
    w.cp_constant = np.r_[np.ones(w.order, np.uint8), np.zeros(w.n_cp - w.order, np.uint8)]  # (gauge)
    check_window(w, hip, oracle, landmarks=np.arange(0, len(w.landmarks), 37))


def test_sample_covariance_against_prior_jacobian(hip, oracle):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, with_priors=16)
    Sigma, _, cond = referee(w, oracle)
    lo, hi = w.valid_range()
    knots = w.t0 + w.dt * np.arange(int(np.ceil((lo - w.t0) / w.dt - 1e-9)), int(np.floor((hi - w.t0) / w.dt - 1e-9)) + 1)
    knots = knots[(knots >= lo) & (knots < hi)]
    between = np.linspace(lo, hi - 1e-6, 23)
    stamps = np.r_[knots, between]
    with ha.Problem(w, lib=hip) as g:
        g.compute_covariance()
        got = g.sample_covariance(stamps)
        poses = g.sample_trajectory(stamps)
    wp = copy.deepcopy(w)
    wp.sensor_T_bs = np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]])
    wp.prior_stamps, wp.prior_poses, wp.prior_sensor = stamps, poses, np.zeros(len(stamps), np.int32)
    with ha.Problem(wp, lib=oracle) as c:
        L = c.linearize(ha.HS_PRIOR, True)
    assert np.abs(L["r"]).max() < 1e-9
    k = w.order
    for i in range(len(stamps)):
        f = 6 * L["first_cp"][i]
        J = L["J_state"][i]
        want = J @ Sigma[f:f + 6 * k, f:f + 6 * k] @ J.T
        assert rel(got[i], want) < bar(cond), (i, stamps[i], rel(got[i], want))
    with ha.Problem(w, lib=hip) as g:
        g.compute_covariance()
        assert g.lib.sample_covariance(g.h, 1, np.array([hi + w.dt]).ctypes.data_as(C.POINTER(C.c_double)),
                                       np.zeros(36).ctypes.data_as(C.POINTER(C.c_double))) == 1


def test_constant_blocks_are_zero_and_unobserved_landmarks_nan(hip, oracle):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, with_priors=16)
    w.cp_constant = np.zeros(16, np.uint8)
    w.cp_constant[[0, 1, 2, 9]] = 1
    w.landmark_constant = np.zeros(len(w.landmarks), np.uint8)
    w.landmark_constant[[3, 17]] = 1
    w.landmarks = np.r_[w.landmarks, [[1.0, 2.0, 3.0]]]  # no residual rows: not in the problem
    w.landmark_constant = np.r_[w.landmark_constant, 0].astype(np.uint8)
    cov = check_window(w, hip, oracle)
    assert not cov["control_points"][[0, 1, 2, 9]].any() and not cov["landmarks"][[3, 17]].any()
    assert np.isnan(cov["landmarks"][-1]).all()


def test_untouched_free_control_point_is_rank_deficient(hip):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, with_priors=16)
    last_segment = w.t0 + (w.n_cp - w.order + (w.order - 1) // 2) * w.dt
    keep = w.pixel_stamps < last_segment
    w.pixel_stamps, w.pixels, w.pixel_landmark, w.pixel_camera = w.pixel_stamps[keep], w.pixels[keep], w.pixel_landmark[keep], w.pixel_camera[keep]
    keep = w.prior_stamps < last_segment
    w.prior_stamps, w.prior_poses, w.prior_sensor = w.prior_stamps[keep], w.prior_poses[keep], w.prior_sensor[keep]
    with ha.Problem(w, lib=hip) as g:
        assert g.lib.compute_covariance(g.h) == HS_ERR_NUMERIC
        assert b"control point 15" in g.lib.last_error(g.h)
        assert g.lib.get_covariance(g.h, None, None, None, None) == HS_ERR_STATE


def test_stale_after_changes(hip):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, with_priors=16)
    with ha.Problem(w, lib=hip) as g:
        get = lambda: g.lib.get_covariance(g.h, None, None, None, None)  # noqa: E731
        assert get() == HS_ERR_STATE
        g.compute_covariance()
        assert get() == 0
        g.set_control_points(np.c_[w.control_points[:, :4], w.control_points[:, 4:7] + 1e-3, w.control_points[:, 7:]])
        assert get() == HS_ERR_STATE
        g.compute_covariance()
        g.append_landmarks(np.array([[0.5, 0.5, 4.0]]))
        assert get() == HS_ERR_STATE
        g.compute_covariance()
        g.solve(2)
        assert get() == HS_ERR_STATE
        g.compute_covariance()
        assert get() == 0


def test_two_calls_bit_identical(hip, oracle):
    w = inertial_window(4, oracle)
    with ha.Problem(w, lib=hip) as g:
        g.compute_covariance()
        a, sa = g.covariance(), g.sample_covariance(np.linspace(*w.valid_range(), 9)[:-1])
        g.compute_covariance()
        b, sb = g.covariance(), g.sample_covariance(np.linspace(*w.valid_range(), 9)[:-1])
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key
    assert np.array_equal(sa, sb)


@pytest.mark.parametrize("inertial", [False, True])
def test_solve_after_covariance_is_unchanged(inertial, hip, oracle):
    if inertial:
        w = inertial_window(4, oracle)
    else:
        w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, with_priors=16)
    with ha.Problem(w, lib=hip) as a, ha.Problem(w, lib=hip) as b:
        a.compute_covariance()
        sa, sb = a.solve(5), b.solve(5)
        assert sa["final_cost"] == sb["final_cost"]
        assert np.array_equal(a.control_points(), b.control_points())
        assert np.array_equal(a.landmarks(), b.landmarks())
