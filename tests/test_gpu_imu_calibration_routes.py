"""hs_solve with free IMU blocks on EVERY route of launch_factor such a handle can take, against the numpy LM referee of
tests/imu_calibration_solve_referee.py at the bars of tests/test_gpu_imu_calibration_solve.py (check_trajectory, check_end_point, check_imu: imported).

A handle that estimates IMU blocks is never factored from both ends. launch_factor (csrc/host_launch.hpp) picks, with n_eff = n_cp - f0 free block
rows behind the frozen prefix f0 and nb border columns (bias, gravity AND the IMU coordinates), what it picks for free camera coordinates — the list of
tests/test_gpu_calibration_routes.py, restated in tests/calibration_windows.py::factor_route, which every test here asserts on the device's own
hs_band_blocks and hs_dim_pose. One window per route, each at the smallest n_cp / band width that selects it (48 control points: 6 n_eff + nb + 1
has to pass 256 to leave k_dense_solve_mx; 52 where k_dense_factor would otherwise take a band of 22), each inside rules (a) and (b) of
test_gpu_imu_calibration_solve.py, which are asserted from the referee before the device is compared. The iteration count (3 .. 5) is the referee's."""
import numpy as np
import pytest

from hyperslam_amd import synthetic

import calibration_windows as cw
import imu_calibration_solve_referee as sref
from imu_calibration_solve_referee import IMU_NAMES, imu_flags
from test_gpu_calibration_solve import check_end_point, check_trajectory
from test_gpu_edge_cases import window_with_band
from test_gpu_imu_calibration_solve import check_imu, estimating

pytestmark = pytest.mark.gpu

MX, LA3, LA4, BF2, WIDE, DENSE = "k_dense_solve_mx", "k_band_factor_la<1,3>", "k_band_factor_la<1,4>", "k_band_factor<2>", "k_band_factor_wide", "k_dense_factor"
SB, BACK = "k_band_backward_sb", "k_band_backward"


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


def prefix(w, f0):
    w.cp_constant = np.r_[np.ones(f0, np.uint8), np.zeros(w.n_cp - f0, np.uint8)] if f0 else None
    return w


def banded(order, bw, n_cp, f0, free, n_inertial=400, bias_dt=1.0, seed=41):
    """A window with exactly `bw` band blocks, an IMU and free IMU blocks."""
    w = window_with_band(order, bw, n_cp=n_cp, seed=seed)
    synthetic.add_imu(w, synthetic.SplitMix64(77), n_inertial, bias_dt=bias_dt)
    w = prefix(w, f0)
    w.imu_constant = imu_flags(free)
    return w


def imu_border(order, bias_dt, free, f0=None, n_inertial=1000, seed=13):
    """48 control points, short tracks, an IMU whose bias splines have a control point every `bias_dt` seconds, and free IMU blocks."""
    w = synthetic.small_visual(order=order, n_cp=48, n_landmarks=120, obs_pairs=3, seed=seed, span=0.5)
    synthetic.add_imu(w, synthetic.SplitMix64(77), n_inertial, bias_dt=bias_dt)
    w = prefix(w, order if f0 is None else f0)
    w.imu_constant = imu_flags(free)
    return w


def route_windows():
    """(name, window, expected (factorisation, backward sweep, border solve), expected band width or None, border columns or None, iterations)."""
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.imu_constant = imu_flags("t")
    yield "dense_solve_mx", w, (MX, None, None), None, None, 4
    yield "la3", imu_border(4, 1.0, "t", f0=0), (LA3, SB, "k_border_solve_reg<4>"), None, 62, 4
    yield "la3_frozen_prefix", imu_border(4, 1.0, "t", f0=6), (LA3, SB, "k_border_solve_reg<4>"), None, 62, 3
    yield "la4_bw16_k6", banded(6, 16, 48, 6, "t"), (LA4, SB, "k_border_solve_reg<4>"), 16, None, 4
    yield "bf2_bw17_last_sb", banded(4, 17, 48, 4, "t"), (BF2, SB, "k_border_solve_reg<4>"), 17, None, 4
    yield "bf2_bw18", banded(4, 18, 48, 4, "t"), (BF2, BACK, "k_border_solve_reg<4>"), 18, None, 4
    yield "wide_bw22", banded(4, 22, 52, 4, "t"), (WIDE, BACK, "k_border_solve_reg<4>"), 22, None, 4
    yield "dense_factor", banded(4, 24, 48, 4, "t"), (DENSE, BACK, "k_border_solve_reg<4>"), 24, None, 4
    # the three border solvers: nb + 1 in (48, 64] (every window above), (112, 128], and the LDS one at exactly 137 unknowns, IMU columns included
    yield "border_117_reg8_k6", imu_border(6, 0.32, "t"), (LA3, SB, "k_border_solve_reg<8>"), None, 116, 4
    yield "border_137_lds", imu_border(4, 0.29, "gx"), (LA3, SB, "k_border_solve"), None, 137, 5


WINDOWS = list(route_windows())
IDS = [name for name, *_ in WINDOWS]


def check_route(g, w, route, bw_want, nb_want):
    """The window takes the intended kernels: launch_factor's rule (calibration_windows.factor_route, T.nb including ni) on what the device reports."""
    g.cost()
    bw, nb, f0 = g.lib.band_blocks(g.h), g.dim_pose() - 6 * w.n_cp, cw.frozen_prefix(w)
    assert bw == cw.band_blocks(w)
    if bw_want is not None:
        assert bw == bw_want, bw
    if nb_want is not None:
        assert nb == nb_want, nb
    assert nb == 6 * len(w.imu["bias_g"]) + 2 + int((~np.asarray(w.imu_constant, bool) * np.array([6, 6, 6, 9, 9])).sum())
    assert cw.factor_route(bw, w.n_cp, f0, nb) == route, (cw.factor_route(bw, w.n_cp, f0, nb), route)
    if route[2] == "k_border_solve":
        assert nb == cw.MAX_BORDER


_REFEREE = {}


def referee(name, w, n, oracle):
    """(rule (a), referee summary, referee end point) of a window: computed once, shared by the two build paths."""
    if name not in _REFEREE:
        _REFEREE[name] = (sref.rule_condition(w, oracle),) + sref.solve(w, oracle, n)
    return _REFEREE[name]


@pytest.mark.parametrize("name,w,route,bw,nb,n", WINDOWS, ids=IDS)
def test_route_against_referee(name, w, route, bw, nb, n, hip, oracle, build_path):
    (ok, cond_free, cond_const), sr, wf = referee(name, w, n, oracle)
    print(name, "cond(S) %.3g with free blocks, %.3g with constant blocks" % (cond_free, cond_const))
    assert ok, (cond_free, cond_const)                                           # (a)
    assert sref.rule_margin(sr), [it["relative_decrease"] for it in sr["iterations"]]  # (b)
    with estimating(w, hip) as g:
        check_route(g, w, route, bw, nb)
        sg = g.solve(n)
        check_trajectory(sg, sr, name)
        assert abs(sg["final_cost"] - sr["final_cost"]) <= 1e-6 * sr["final_cost"] + 1e-8 * sr["initial_cost"]
        check_end_point(g, wf, name)
        now = check_imu(g, wf, name)
        const = np.asarray(w.imu_constant, bool)
        moved = any(it["step_is_successful"] for it in sr["iterations"][1:])
        for b, k in enumerate(IMU_NAMES):
            assert np.array_equal(now[k], np.asarray(w.imu[k], float).reshape(-1)) == (bool(const[b]) or not moved), k


@pytest.mark.parametrize("name", ["wide_bw22", "border_137_lds"])
def test_two_solves_are_bit_identical(name, hip, build_path):
    _, w, _, _, _, n = WINDOWS[IDS.index(name)]
    outs = []
    for _ in range(2):
        with estimating(w, hip) as g:
            s = g.solve(n)
            outs.append((s["iterations"], g.control_points(), g.landmarks(), *g.bias(), g.gravity(), *[g.imu()[k] for k in IMU_NAMES]))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a, b)
