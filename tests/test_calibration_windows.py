"""tests/calibration_windows.py on the CPU: the restated host rules (band width, launch_factor's routes), the window generator of the sweeps, the
route-matrix windows of tests/test_gpu_calibration_routes.py, and the proof that the device bars notice a dropped camera term."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha

import calibration_solve_referee as sref
import calibration_windows as cw
from calibration_referee import camera_columns

LA3, LA4, BF2, WIDE, DENSE = "k_band_factor_la<1,3>", "k_band_factor_la<1,4>", "k_band_factor<2>", "k_band_factor_wide", "k_dense_factor"
SB, BACK = "k_band_backward_sb", "k_band_backward"


def test_band_blocks_of_the_exact_band_windows():
    from test_gpu_edge_cases import window_with_band
    for order, bw in ((4, 13), (4, 22), (6, 16), (4, 42)):
        assert cw.band_blocks(window_with_band(order, bw)) == bw


def test_routes_switch_where_launch_factor_switches():
    """48 control points, frozen prefix 4, 14 camera columns: each band width on its kernel, and one step in size on another."""
    route = lambda bw, n_cp=48, f0=4, nb=14: cw.factor_route(bw, n_cp, f0, nb)  # noqa: E731
    assert [route(bw)[0] for bw in (14, 15, 16, 17, 21)] == [LA3, LA4, LA4, BF2, BF2]
    assert route(22, n_cp=52)[0] == WIDE and route(22, n_cp=48)[0] == DENSE   # n_eff 48 > 2 bw = 44, n_eff 44 <= 44
    assert route(42)[0] == WIDE and route(30)[0] == DENSE                      # 44 block rows of 42 band blocks: 987 tiles > 896
    assert [route(bw)[1] for bw in (16, 17, 18)] == [SB, SB, BACK]            # 6 (bw - 1) <= 96
    assert route(24)[0] == DENSE and route(24, n_cp=53)[0] == WIDE             # n_eff 49 > 2 bw
    assert route(24, n_cp=44, f0=4) == ("k_dense_solve_mx", None, None)       # 6 x 40 + 14 + 1 = 255 <= 256
    assert route(24, n_cp=45, f0=4)[0] == DENSE                                # 261
    assert [route(9, nb=nb)[2] for nb in (14, 47, 48, 63, 64, 111, 112, 127, 128, 137)] == \
        ["k_border_solve_reg<%d>" % r for r in (3, 3, 4, 4, 5, 7, 8, 8)] + ["k_border_solve"] * 2
    assert [cw.border_forward_lanes(bw) for bw in (9, 22, 23, 33, 34, 42)] == [128, 128, 192, 192, 256, 256]
    assert cw.frozen_prefix(type("W", (), dict(cp_constant=np.array([1, 1, 0, 1, 0])))) == 2


def test_route_matrix_windows_take_their_routes(oracle):
    """The windows of the device route matrix, from CPU quantities: band width by the host rule, border columns from the oracle's hs_dim_pose
    plus the free camera coordinates. Every line of the matrix is there."""
    import test_gpu_calibration_routes as routes
    seen = set()
    for name, w, route, bw_want, nb_want in routes.WINDOWS:
        w0 = copy.copy(w)
        w0.cam_constant = None
        with ha.Problem(w0, lib=oracle) as c:
            nb = c.dim_pose() - 6 * w.n_cp + camera_columns(w)[1]
        bw = cw.band_blocks(w)
        assert bw_want in (None, bw) and nb_want in (None, nb), (name, bw, nb)
        assert cw.factor_route(bw, w.n_cp, cw.frozen_prefix(w), nb) == route, name
        assert w.n_cp <= 64 and len(w.landmarks) <= 150
        seen.add(route)
        seen.add((route[0], cw.frozen_prefix(w) > 0))
    for factor in (LA3, LA4, BF2, WIDE, DENSE):
        assert any(r[0] == factor for r in seen if len(r) == 3), factor
    assert (DENSE, True) in seen and (DENSE, False) in seen and (LA3, True) in seen
    assert {r[2] for r in seen if len(r) == 3} >= {"k_border_solve_reg<3>", "k_border_solve_reg<4>", "k_border_solve_reg<8>", "k_border_solve"}
    assert (BF2, SB, "k_border_solve_reg<3>") in seen and (BF2, BACK, "k_border_solve_reg<3>") in seen


def test_generator_is_deterministic_and_inside_the_limits():
    a, b = list(cw.cases(40, 12)), list(cw.cases(40, 12))
    assert [t for t, _ in a] == [t for t, _ in b] and [t for t, _ in a] != [t for t, _ in cw.cases(40, 13)]
    seen = dict(imu=0, bearing=0, priors=0, frozen=0, lmc=0, rc=0, tc=0)
    for (tag, w), (_, w2) in zip(a, b):
        assert np.array_equal(w.control_points, w2.control_points) and np.array_equal(w.cam_constant, w2.cam_constant)
        nc = camera_columns(w)[1]
        assert nc > 0 and 8 <= w.n_cp <= 64 and len(w.landmarks) <= 150 and cw.band_blocks(w) <= cw.MAX_BAND
        nbi = 6 * len(w.imu["bias_g"]) + 2 if w.imu is not None else 0
        assert nbi + nc <= cw.MAX_BORDER
        seen["imu"] += w.imu is not None
        seen["bearing"] += len(w.bearing_stamps) > 0
        seen["priors"] += len(w.prior_stamps) > 0
        seen["frozen"] += cw.frozen_prefix(w) > 0
        seen["lmc"] += w.landmark_constant is not None
        seen["rc"] += bool(w.rotation_constant)
        seen["tc"] += bool(w.translation_constant)
    assert all(v > 0 for v in seen.values()), seen
    assert len({w.order for _, w in a}) == 3 and len({len(w.imu["bias_g"]) for _, w in a if w.imu is not None}) > 3


def test_bars_catch_a_dropped_camera_term(oracle, monkeypatch, capsys):
    """A deliberate error, on the CPU: the landmark back-substitution without its camera term (y_l = L^-T (yh - Yh' y_p - Y_c y_c) with Y_c y_c
    dropped — what k_backsub_retract<false> would compute for a handle with free cameras). The bars the device tests apply to the device reject
    the wrong solve's trajectory on a window of the route matrix."""
    from test_gpu_calibration_solve import check_trajectory, rel
    import test_gpu_calibration_routes as routes
    w = routes.WINDOWS[routes.IDS.index("bf2_bw18")][1]
    good, w_good = sref.solve(w, oracle, 3)

    class Dropped(sref.System):
        def step_schur(self, s, sl, radius):
            S, g, _ = self.scaled_system(s, sl, radius)
            y = sref._solve(S, g)
            dl = np.zeros_like(self.bl)
            for l, (Vi, _) in self.landmark_blocks(sl, radius).items():
                W = self.Hxl[l] * sl[l][None, :]
                W[self.P0:] = 0.0  # the camera rows: Y_c y_c dropped
                dl[l] = np.asarray(-sl[l] * (Vi @ (sl[l] * self.bl[l] - W.T @ (s * y))), float)
            return np.asarray(-s * y, float), dl

    monkeypatch.setattr(sref, "System", Dropped)
    bad, w_bad = sref.solve(w, oracle, 3)
    assert rel(w_bad.landmarks, w_good.landmarks) > 1e-6
    with pytest.raises(AssertionError):
        check_trajectory(bad, good, "dropped Y_c dc")
    capsys.readouterr()
