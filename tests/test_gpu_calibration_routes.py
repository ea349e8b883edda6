"""hs_solve with free camera blocks on EVERY one-ended route of launch_factor, against the numpy LM referee of
tests/calibration_solve_referee.py at the bars of tests/test_gpu_calibration_solve.py (check_trajectory, check_end_point: unchanged, imported).

A handle with free camera coordinates is never factored from both ends. launch_factor (csrc/host_launch.hpp) then picks, with n_eff = n_cp - f0 free
block rows behind the frozen prefix f0 and nb border columns (bias, gravity AND camera coordinates):
  k_dense_solve_mx            6 n_eff + nb + 1 <= 256 (the windows of test_gpu_calibration_solve.py but one)
  k_dense_factor              bw > 14, n_eff <= 2 bw, dense_factor_fits(n_eff, min(bw, n_eff))
  k_band_factor_la<1,3>       bw <= 14
  k_band_factor_la<1,4>       bw 15, 16
  k_band_factor<2>            bw 17 .. 21
  k_band_factor_wide          bw 22 .. 42
behind the banded ones k_band_backward_sb while 6 (bw - 1) <= 96 (bw <= 17) and k_band_backward beyond, and next to all but the first
k_border_forward (one lane per pending row: 128, 192 or 256 lanes), k_border_schur, launch_border_solve (k_border_solve_reg<R> on 16 R >= nb + 1
columns, R = 3 .. 8, the LDS k_border_solve for nb + 1 in 129 .. 138) and k_border_apply. tests/calibration_windows.py::factor_route restates these
rules; every test asserts its route from the device's own hs_band_blocks and hs_dim_pose.

Every window meets the conditioning rule of test_solve_against_referee (cond of the reduced system with free cameras at most twice the one with
constant cameras, below 1e7 without an IMU); the two numbers of each window, computed by calibration_solve_referee.condition, stand in its comment.
Wall time on an MI355X box: 0.6 .. 2.5 s per case (the IMU borders the longest), referee included; the referee is computed once per window and shared
by the two build paths."""
import numpy as np
import pytest

from hyperslam_amd import synthetic

import calibration_solve_referee as sref
import calibration_windows as cw
from calibration_solve_referee import flags
from test_gpu_calibration_solve import check_end_point, check_trajectory, estimating
from test_gpu_edge_cases import window_with_band

pytestmark = pytest.mark.gpu

LA3, LA4, BF2, WIDE, DENSE = "k_band_factor_la<1,3>", "k_band_factor_la<1,4>", "k_band_factor<2>", "k_band_factor_wide", "k_dense_factor"
SB, BACK = "k_band_backward_sb", "k_band_backward"


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


def prefix(w, f0):
    w.cp_constant = np.r_[np.ones(f0, np.uint8), np.zeros(w.n_cp - f0, np.uint8)] if f0 else None
    return w


def banded(order, bw, n_cp, f0, seed=41, **free):
    w = prefix(window_with_band(order, bw, n_cp=n_cp, seed=seed), f0)
    w.cam_constant = flags(w, **free)
    return w


def imu_border(order, bias_dt, n_inertial=1000, seed=13, **free):
    """48 control points, short tracks, an IMU whose bias splines have a control point every `bias_dt` seconds, and free camera blocks."""
    w = synthetic.small_visual(order=order, n_cp=48, n_landmarks=120, obs_pairs=3, seed=seed, span=0.5)
    synthetic.add_imu(w, synthetic.SplitMix64(77), n_inertial, bias_dt=bias_dt)
    w = prefix(w, order)
    w.cam_constant = flags(w, **free)
    return w


def route_windows():
    """(name, window, expected (factorisation, backward sweep, border solve), expected band width or None, border columns or None).
    Behind each: cond of the reduced system with free cameras / with constant cameras."""
    # --- the route matrix: one window per line of the list in the module docstring -------------------------------------------------------
    w = prefix(synthetic.small_visual(order=4, n_cp=52, n_landmarks=130, obs_pairs=3, seed=13, span=0.5), 6)
    w.cam_constant = flags(w, cam1="tid")
    yield "la3_frozen_prefix", w, (LA3, SB, "k_border_solve_reg<3>"), None, 14  # cond 2.89e4 / 2.89e4
    yield "la4_bw15", banded(4, 15, 48, 4, cam1="tid"), (LA4, SB, "k_border_solve_reg<3>"), 15, 14  # cond 8.15e4 / 8.12e4
    yield "la4_bw16_k6", banded(6, 16, 48, 6, cam1="tid"), (LA4, SB, "k_border_solve_reg<3>"), 16, 14  # cond 7.71e6 / 7.67e6
    yield "bf2_bw17_last_sb", banded(4, 17, 48, 4, cam1="tid"), (BF2, SB, "k_border_solve_reg<3>"), 17, 14  # cond 8.84e4 / 8.81e4
    yield "bf2_bw18", banded(4, 18, 48, 4, cam1="tid"), (BF2, BACK, "k_border_solve_reg<3>"), 18, 14  # cond 8.84e4 / 8.81e4
    yield "bf2_bw21", banded(4, 21, 48, 4, cam0="id", cam1="tid"), (BF2, BACK, "k_border_solve_reg<3>"), 21, 22  # cond 8.86e4 / 8.81e4
    yield "wide_bw22", banded(4, 22, 52, 4, cam1="tid"), (WIDE, BACK, "k_border_solve_reg<3>"), 22, 14  # cond 6.19e4 / 6.19e4
    yield "wide_bw42_limit", banded(4, 42, 48, 4, cam1="tid"), (WIDE, BACK, "k_border_solve_reg<3>"), 42, 14  # cond 8.81e4 / 8.78e4
    yield "dense_factor_frozen_prefix", banded(4, 24, 48, 4, cam1="tid"), (DENSE, BACK, "k_border_solve_reg<3>"), 24, 14  # cond 8.84e4 / 8.81e4
    yield "dense_factor_no_prefix", banded(4, 24, 44, 0, cam1="tid"), (DENSE, BACK, "k_border_solve_reg<3>"), 24, 14  # cond 2.79e6 / 2.77e6
    # --- an IMU border next to camera columns on a banded route: nb + 1 in (48, 64], (112, 128], (128, 138] ---------------------------------
    yield "imu_border_63_reg4", imu_border(4, 1.0, cam1="t"), (LA3, SB, "k_border_solve_reg<4>"), None, 62  # cond 5.45e8 / 5.45e8
    yield "imu_border_123_reg8_k6_both_T_bs", imu_border(6, 0.32, cam0="t", cam1="t"), (LA3, SB, "k_border_solve_reg<8>"), None, 122  # cond 1.48e10 / 1.48e10
    yield "imu_border_137_lds", imu_border(4, 0.29, cam1="tid"), (LA3, SB, "k_border_solve"), None, 136  # cond 1.59e9 / 1.59e9
    # --- options, each on a banded route -------------------------------------------------------------------------------------------------
    w = prefix(synthetic.small_visual(order=4, n_cp=48, n_landmarks=150, obs_pairs=4, bearing=True, seed=9, span=1.0), 4)
    w.cam_constant = flags(w, cam1="t")
    yield "bearing_T_bs", w, (LA3, SB, "k_border_solve_reg<3>"), None, 6  # cond 2.92e6 / 2.88e6
    w = banded(4, 18, 48, 4, cam1="tid")
    w.landmark_constant = (np.arange(len(w.landmarks)) % 5 == 0).astype(np.uint8)
    yield "constant_landmarks_bw18", w, (BF2, BACK, "k_border_solve_reg<3>"), 18, 14  # cond 9.15e4 / 9.12e4
    w = synthetic.small_visual(order=4, n_cp=48, n_landmarks=120, obs_pairs=3, seed=13, span=0.5, with_priors=48)
    w.rotation_constant = True
    w.cam_constant = flags(w, cam1="tid")
    yield "rotation_constant", w, (LA3, SB, "k_border_solve_reg<3>"), None, 14  # cond 4.19e3 / 2.80e3
    w = synthetic.small_visual(order=4, n_cp=48, n_landmarks=120, obs_pairs=3, seed=13, span=0.5, with_priors=48)
    w.translation_constant = True
    w.cam_constant = flags(w, cam1="tid")
    yield "translation_constant", w, (LA3, SB, "k_border_solve_reg<3>"), None, 14  # cond 6.48e3 / 4.83e3
    w = imu_border(4, 1.0, cam1="t")
    w.imu["bias_constant"] = True  # (T.nb > T.nc with only gravity free)
    yield "constant_bias_free_gravity", w, (LA3, SB, "k_border_solve_reg<4>"), None, 62  # cond 1.92e4 / 1.91e4


WINDOWS = list(route_windows())
IDS = [name for name, *_ in WINDOWS]


def check_route(g, w, route, bw_want, nb_want):
    """The window takes the intended kernels: launch_factor's rule (restated in calibration_windows.factor_route) on what the device reports."""
    g.cost()
    bw, nb, f0 = g.lib.band_blocks(g.h), g.dim_pose() - 6 * w.n_cp, cw.frozen_prefix(w)
    assert bw == cw.band_blocks(w)
    if bw_want is not None:
        assert bw == bw_want, bw
    if nb_want is not None:
        assert nb == nb_want, nb
    n_eff = w.n_cp - f0
    assert 6 * n_eff + nb + 1 > 256  # too large for k_dense_solve_mx (use_dense_mx: dense_mx_fits(n_eff, nb))
    factor, backward, border = route
    # the factorisation, in launch_factor's order
    if factor == DENSE:
        assert bw > 14 and n_eff <= 2 * bw and cw.dense_factor_fits(n_eff, min(bw, n_eff))
    else:
        assert not (bw > 14 and n_eff <= 2 * bw and cw.dense_factor_fits(n_eff, min(bw, n_eff)))
        assert {LA3: bw <= 14, LA4: 15 <= bw <= 16, BF2: 17 <= bw <= 21, WIDE: 22 <= bw <= 42}[factor], bw
    assert (6 * (bw - 1) <= 96) == (backward == SB), bw  # k_band_backward_sb: one lane pair per pending row, 96 pairs
    if border == "k_border_solve":
        assert 128 < nb + 1 <= 138  # the LDS border solve, at most 137 unknowns
    else:
        assert nb + 1 <= 128 and border == "k_border_solve_reg<%d>" % max(3, (nb + 1 + 15) // 16)
    assert cw.factor_route(bw, w.n_cp, f0, nb) == route


_REFEREE = {}


def referee(name, w, oracle):
    """(conditioning, referee summary, referee end point) of a window: computed once, shared by both build paths."""
    if name not in _REFEREE:
        _REFEREE[name] = (cw.conditioning(w, oracle),) + sref.solve(w, oracle, 5)
    return _REFEREE[name]


@pytest.mark.parametrize("name,w,route,bw,nb", WINDOWS, ids=IDS)
def test_route_against_referee(name, w, route, bw, nb, hip, oracle, build_path):
    (cond_free, cond_const, ok), sr, wf = referee(name, w, oracle)
    print(name, "cond(S) %.3g with free cameras, %.3g with constant cameras" % (cond_free, cond_const))
    assert ok, (cond_free, cond_const)
    with estimating(w, hip) as g:
        check_route(g, w, route, bw, nb)
        if name == "wide_bw42_limit":
            assert cw.border_forward_lanes(g.lib.band_blocks(g.h)) == 256
        sg = g.solve(5)
        check_trajectory(sg, sr, name)
        assert abs(sg["final_cost"] - sr["final_cost"]) <= 1e-6 * sr["final_cost"] + 1e-8 * sr["initial_cost"]
        check_end_point(g, wf, name)
        T, I, D = g.cameras()
        const = np.asarray(w.cam_constant, bool)
        for c in range(len(T)):
            for b, (now, was) in enumerate(((T[c], w.cam_T_bs[c]), (I[c], w.cam_intrinsics[c]), (D[c], w.cam_distortion[c]))):
                assert np.array_equal(now, was) == bool(const[c, b]), (c, b)
        if name == "constant_bias_free_gravity":
            bg, ba = g.bias()
            assert np.array_equal(bg, w.imu["bias_g"]) and np.array_equal(ba, w.imu["bias_a"])
            assert not np.array_equal(g.gravity(), w.gravity)


@pytest.mark.parametrize("name", ["wide_bw22", "imu_border_137_lds"])
def test_two_solves_are_bit_identical(name, hip, build_path):
    w = WINDOWS[IDS.index(name)][1]
    outs = []
    for _ in range(2):
        with estimating(w, hip) as g:
            s = g.solve(5)
            outs.append((s["iterations"], g.control_points(), g.landmarks(), *g.cameras()))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a, b)
