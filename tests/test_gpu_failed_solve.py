"""A solve that fails, route by route, HIP against the oracle: one non-finite value in an otherwise clean window makes every step invalid
(Ceres' HandleInvalidStep: nothing committed, radius halved) and the fifth invalid step in a row ends the solve in FAILURE. The oracle
(oracle/hs_problem.hpp, run()) gives for every injection below: termination 2, 5 iterations, 0 successful steps, radii 5000, 2500, 1250,
625, 625, step_is_valid == 0 from iteration 1 on, the state untouched. Everything compared is exact — flags, counts, radii that are 1e4
times powers of 1/2, bit-identical arrays — so there is no tolerance. cost and gradient_max_norm of these iterations are non-finite or
order-dependent by construction and are not compared.
Injections (the stamps stay finite: they index the spline; no index, loop bound or wait condition of the kernels is computed from a pixel,
landmark, control-point or bias VALUE — segment_of() takes stamps, the sort keys of the fused build are segments, every wait polls an epoch
or a row count):
  pixel      one pixel NaN: the reduced system stays finite and positive definite, the gradient is NaN, the step is rejected through the
             non-finite model cost change, not through the factorisation's verdict
  cp_first / cp_last / cp_middle
             the translation of one free control point NaN: NaN block rows at the near end, the far end and around the junction of a
             two-ended factorisation — DevState::chol_failed raised by the factorisation kernel of the route
  bias       with an IMU: one gyroscope bias point NaN — the verdict comes from the border
Routes, each at the smallest window that selects it (launch_factor, host_launch.hpp; asserted on the device's own band width and border size
through the rule restated in tests/calibration_windows.py).
No residue: a handle that went through a failed solve and got its clean tables back solves bit-identically to a fresh handle — verdict,
invalid streak, scaling flag, record selector and NaN-holding candidate buffers all die with the failed solve."""
import copy

import numpy as np
import pytest

import calibration_windows as cw
import hyperslam_amd as ha
from hyperslam_amd import switches, synthetic
from test_gpu_edge_cases import window_with_band

pytestmark = pytest.mark.gpu

RADII = [1e4, 5000.0, 2500.0, 1250.0, 625.0, 625.0]  # record 0: the start point; the fifth invalid step ends the solve without halving


def small():
    return synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3, seed=33, with_priors=16)


def small_imu():
    return synthetic.small_inertial(order=4, n_cp=16, n_landmarks=30, obs_pairs=3, n_inertial=80, seed=21)


WINDOWS = {"small": small, "small_imu": small_imu, "bw14": lambda: window_with_band(4, 14, n_cp=72), "bw16": lambda: window_with_band(4, 16, n_cp=72),
           "bw24": lambda: window_with_band(4, 24), "bw24_long": lambda: window_with_band(4, 24, n_cp=53),
           "bw14_imu": lambda: window_with_band(4, 14, n_cp=72, imu=True)}
# name -> (window, band blocks, measurement switch, two-ended, factorisation kernel by the one-ended rule)
ROUTES = {
    "dense_solve_mx": ("small", None, None, False, "k_dense_solve_mx"),
    "mx_two_ended_bw14": ("bw14", 14, None, True, None),
    "mx_two_ended_bw16_wide": ("bw16", 16, None, True, None),
    "la_two_ended_bw14": ("bw14", 14, "factor_la", True, None),
    "la_two_ended_bw16": ("bw16", 16, "factor_la", True, None),
    "one_ended_bw14": ("bw14", 14, "one_ended", False, "k_band_factor_la<1,3>"),
    "one_ended_bw16": ("bw16", 16, "one_ended", False, "k_band_factor_la<1,4>"),
    "bw24": ("bw24", 24, None, False, "k_dense_factor"),  # (48 control points, 44 free block rows <= 2 x 24: every band tile in a register)
    "bw24_wide": ("bw24_long", 24, None, False, "k_band_factor_wide"),  # (49 free block rows: the trailing window in L2)
    "dense_solve_mx_imu": ("small_imu", None, None, False, "k_dense_solve_mx"),
    "mx_two_ended_bw14_imu": ("bw14_imu", 14, None, True, None),
}
INJECTIONS = ("pixel", "cp_first", "cp_last", "cp_middle", "bias")
CASES = [(r, i) for r in ROUTES for i in INJECTIONS if i != "bias" or r.endswith("_imu")]


def inject(w, what):
    """A copy of the window with one value replaced."""
    w = copy.deepcopy(w)
    free = np.arange(w.n_cp) if w.cp_constant is None else np.flatnonzero(np.asarray(w.cp_constant) == 0)
    if what == "pixel":
        w.pixels = np.array(w.pixels, float)
        w.pixels[len(w.pixels) // 2, 0] = np.nan
    elif what == "bias":
        w.imu = dict(w.imu)
        w.imu["bias_g"] = np.array(w.imu["bias_g"], float)
        w.imu["bias_g"][len(w.imu["bias_g"]) // 2, :3] = np.nan  # [value, stamp]
    else:
        # (the last control point a pixel row reaches: a window may end in control points nothing observes, whose value reaches no kernel)
        reach = int((np.floor((np.asarray(w.pixel_stamps) - w.t0) / w.dt) - (w.order - 1) // 2).max()) + w.order - 1
        i = {"cp_first": free[0], "cp_last": min(free[-1], reach), "cp_middle": w.n_cp // 2}[what]
        assert i in free
        w.control_points = np.array(w.control_points, float)
        w.control_points[i, 4:7] = np.nan  # [quaternion, translation, stamp]
    return w


def state(p, w):
    s = [p.control_points(), p.landmarks()]
    if len(w.inertial_stamps):
        s += list(p.bias()) + [p.gravity()]
    return s


def check_route(g, w, name):
    _, bw_want, flags, two_ended, kernel = ROUTES[name]
    g.cost()
    bw, nb, f0 = g.lib.band_blocks(g.h), g.dim_pose() - 6 * w.n_cp, cw.frozen_prefix(w)
    if bw_want is not None:
        assert bw == bw_want, bw
    if two_ended:  # factor_two_ended_any: k_band_factor_mx up to 16 band blocks (switch factor_la: k_band_factor_la), bordered or not
        assert w.n_cp >= 4 * bw and bw <= 16
        if nb:  # the border Schur complement goes through k_dense_solve_mx in border mode from 64 unknowns on
            assert 64 <= nb <= 254, nb
    else:
        assert w.n_cp < 4 * bw or flags == "one_ended"
        assert cw.factor_route(bw, w.n_cp, f0, nb)[0] == kernel, cw.factor_route(bw, w.n_cp, f0, nb)


_ORACLE = {}


def oracle_run(name, what, oracle):
    """The oracle's failed solve of a (window, injection): computed once. The switches select kernels of the library, not arithmetic."""
    key = (ROUTES[name][0], what)
    if key not in _ORACLE:
        w = inject(WINDOWS[key[0]](), what)
        with ha.Problem(w, lib=oracle) as c:
            before = state(c, w)
            s = c.solve(5)
            after = state(c, w)
        # what the oracle is stated to do (module docstring): the expectation the library is held to
        assert (s["termination"], s["num_iterations"], s["num_successful_steps"]) == (2, 5, 0), s
        assert [r["radius"] for r in s["iterations"]] == RADII
        assert [r["step_is_valid"] for r in s["iterations"]] == [1, 0, 0, 0, 0, 0]
        assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
        _ORACLE[key] = s
    return _ORACLE[key]


@pytest.mark.parametrize("name,what", CASES, ids=["%s-%s" % c for c in CASES])
def test_failed_solve_matches_oracle(name, what, hip, oracle, monkeypatch):
    make, flags = WINDOWS[ROUTES[name][0]], ROUTES[name][2]
    monkeypatch.setenv("HS_DEBUG_FLAGS", switches.flags(flags) if flags else "0")
    sc = oracle_run(name, what, oracle)
    w = inject(make(), what)
    with ha.Problem(make(), lib=hip) as g:  # the route, on the clean window (the injection changes no structure)
        check_route(g, w, name)
    with ha.Problem(w, lib=hip) as g:
        before = state(g, w)
        sg = g.solve(5)
        after = state(g, w)
        err = g.lib.last_error(g.h)
    print(name, what, [(r["step_is_valid"], r["step_is_successful"], r["radius"]) for r in sg["iterations"]], err)
    assert (sg["termination"], sg["num_iterations"], sg["num_successful_steps"]) == (2, 5, 0)
    assert (sc["termination"], sc["num_iterations"], sc["num_successful_steps"]) == (2, 5, 0)
    assert len(sg["iterations"]) == len(sc["iterations"]) == 6
    for rg, rc in zip(sg["iterations"], sc["iterations"]):
        assert (rg["step_is_valid"], rg["step_is_successful"], rg["radius"]) == (rc["step_is_valid"], rc["step_is_successful"], rc["radius"]), (rg, rc)
    for a, b in zip(before, after):  # control points, landmarks, biases, gravity: nothing committed
        assert np.array_equal(a, b, equal_nan=True)
    if what != "pixel":  # the verdict of the factorisation ended the solve
        assert b"not positive definite" in (err or b""), err


def summary_key(s):
    skip = ("linearize_ms", "schur_ms", "solve_ms", "update_ms", "total_ms")  # (event times of the run, not results)
    return {k: v for k, v in s.items() if k not in skip}


RESIDUE_CASES = [c for c in CASES if c[1] in ("pixel", "cp_middle")]  # (what set_residuals / set_control_points can inject into a resident window)


@pytest.mark.parametrize("name,what", RESIDUE_CASES, ids=["%s-%s" % c for c in RESIDUE_CASES])
def test_failed_solve_leaves_no_residue(name, what, hip, monkeypatch):
    make, flags = WINDOWS[ROUTES[name][0]], ROUTES[name][2]
    monkeypatch.setenv("HS_DEBUG_FLAGS", switches.flags(flags) if flags else "0")
    w, bad = make(), inject(make(), what)
    with ha.Problem(w, lib=hip) as fresh:
        want = fresh.solve(5)
        want_state = state(fresh, w)
    assert want["termination"] != 2 and want["num_successful_steps"] >= 1  # the clean window does solve
    with ha.Problem(w, lib=hip) as g:
        g.snapshot()
        if what == "pixel":
            g.set_residuals(ha.HS_PIXEL, bad.pixel_stamps, bad.pixels, bad.pixel_landmark, bad.pixel_camera)
        else:
            g.set_control_points(bad.control_points, bad.cp_constant)
        assert g.solve(5)["termination"] == 2
        if what == "pixel":
            g.set_residuals(ha.HS_PIXEL, w.pixel_stamps, w.pixels, w.pixel_landmark, w.pixel_camera)
        else:
            g.restore()
        got = g.solve(5)
        got_state = state(g, w)
    a, b = summary_key(got), summary_key(want)
    assert a.keys() == b.keys()
    for k in a:  # every field of the summary and of every iteration record, bit for bit
        assert np.array_equal(np.array(a[k] if k != "iterations" else [list(r.values()) for r in a[k]], float),
                              np.array(b[k] if k != "iterations" else [list(r.values()) for r in b[k]], float), equal_nan=True), (k, a[k], b[k])
    for x, y in zip(got_state, want_state):
        assert np.array_equal(x, y, equal_nan=True)
