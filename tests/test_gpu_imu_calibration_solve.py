"""Estimating free IMU blocks in hs_solve on the GPU (hs_set_imu_estimation) against the numpy LM referee of
tests/imu_calibration_solve_referee.py, which tests/test_imu_calibration_solve_referee.py pins to the camera referee, the build referee and a
dense solve of the full system.

The bars are those of tests/test_gpu_parity.py::test_solve_trajectory as tests/test_gpu_calibration_solve.py uses them (check_trajectory,
imported): identical iteration counts, decisions and termination; per-iteration cost within 1e-6 |cost| + 1e-8 initial cost; radius, step norm
and relative decrease within 1e-5 relative; end points within 1e-6 relative — and the five IMU blocks of hs_get_imu, each as its own array,
within 1e-6 relative of the referee's final values.

Every window is admitted by rules evaluated from the referee alone, on the CPU, and asserted here before the device is compared:
  (a) cond of the referee's scaled, damped system with the blocks free is at most twice the cond with them constant;
  (b) no iteration of the referee's solve has a relative decrease within 1e-3 of the 1e-3 threshold;
  (c) the referee's solve has at least two accepted steps that change the IMU parameters;
  (d) across the set, at least one window has a rejected step between accepted ones.
The iteration count of a window (imu_calibration_solve_referee.free_imu_windows, 3 .. 5) is the referee's: on these synthetic windows one LM
step at radius 1e4 moves the IMU blocks by far more than their error, so rejected steps are the rule, not the exception. No window of the
list had to be replaced by another seed or a smaller free set: all eight are inside the rules (worst cond ratio 1.17)."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import calibration_solve_referee as csr
import imu_calibration_referee as bref
import imu_calibration_solve_referee as sref
from imu_calibration_solve_referee import IMU_NAMES, imu_flags
from test_gpu_calibration_solve import SUMMARY, check_end_point, check_trajectory, rel

pytestmark = pytest.mark.gpu

WINDOWS = list(sref.free_imu_windows())
IDS = [n for n, *_ in WINDOWS]


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


def estimating(w, hip, mode=None):
    g = ha.Problem(w, lib=hip)
    g.set_imu_estimation(True)
    if w.cam_constant is not None:
        g.set_camera_estimation(True)
    if mode is not None:
        g.set_inertial_jacobian(mode)
    return g


_REFEREE = {}


def referee(name, oracle, n=None):
    """(rule (a), referee summary, referee end point) of a window: computed once, shared by the tests and build paths (read-only)."""
    _, w, mode, n0 = WINDOWS[IDS.index(name)]
    n = n0 if n is None else n
    if (name, n) not in _REFEREE:
        _REFEREE[(name, n)] = (sref.rule_condition(w, oracle, mode),) + sref.solve(w, oracle, n, mode=mode)
    return _REFEREE[(name, n)]


def check_imu(g, wf, name):
    now = g.imu()
    errs = {k: rel(now[k], np.asarray(wf.imu[k], float).reshape(-1)) for k in IMU_NAMES}
    print(name, errs)
    for k, e in errs.items():
        assert e < 1e-6, (name, k, e)
    return now


@pytest.mark.parametrize("name,w,mode,n", WINDOWS, ids=IDS)
def test_solve_against_referee(name, w, mode, n, hip, oracle, build_path):
    (ok, cond_free, cond_const), sr, wf = referee(name, oracle)
    print(name, "cond(S) %.3g with free blocks, %.3g with constant blocks" % (cond_free, cond_const))
    assert ok, (cond_free, cond_const)                                           # (a)
    assert n <= 10 and sref.rule_margin(sr), [it["relative_decrease"] for it in sr["iterations"]]  # (b)
    assert sref.rule_accepted(sr), [it["step_is_successful"] for it in sr["iterations"]]           # (c)
    with estimating(w, hip, mode) as g:
        if name.startswith("k4_"):
            assert 6 * w.n_cp + (g.dim_pose() - 6 * w.n_cp) + 1 <= 256  # k_dense_solve_mx
        sg = g.solve(n)
        check_trajectory(sg, sr, name)
        assert abs(sg["final_cost"] - sr["final_cost"]) <= 1e-6 * sr["final_cost"] + 1e-8 * sr["initial_cost"]
        check_end_point(g, wf, name)
        now = check_imu(g, wf, name)
        # the estimate moved, and only the free blocks did
        const = np.asarray(w.imu_constant, bool)
        for b, k in enumerate(IMU_NAMES):
            assert np.array_equal(now[k], np.asarray(w.imu[k], float).reshape(-1)) == bool(const[b]), k
        if name == "k6_frozen_prefix_constant_bias_S_g":
            bg, ba = g.bias()
            assert np.array_equal(bg, w.imu["bias_g"]) and np.array_equal(ba, w.imu["bias_a"])


def test_the_set_has_a_rejected_step_between_accepted_ones(oracle):
    assert any(sref.has_rejected_between_accepted(referee(name, oracle)[1]) for name in IDS)  # (d)


def oracle_window(w, g):
    """The window at the state the device handle g holds, every sensor block constant: what the oracle evaluates."""
    wq = copy.copy(w)
    wq.control_points, wq.landmarks, wq.gravity = g.control_points(), g.landmarks(), g.gravity()
    bg, ba = g.bias()
    wq.imu = dict(w.imu, bias_g=bg, bias_a=ba, **g.imu())
    wq.cam_T_bs, wq.cam_intrinsics, wq.cam_distortion = g.cameras()
    wq.imu_constant = wq.cam_constant = None
    return wq


def test_hand_over(hip, oracle, build_path):
    name, w, mode, n = WINDOWS[0]
    _, sr, wf = referee(name, oracle)
    with estimating(w, hip) as g:
        start = g.imu()
        for k in IMU_NAMES:
            assert np.array_equal(start[k], np.asarray(w.imu[k], float).reshape(-1))
        g.snapshot()
        s1 = g.solve(n)
        first = (g.control_points(), g.landmarks(), g.bias(), g.gravity(), g.imu())
        check_imu(g, wf, name)  # get_imu after the solve: the referee's parameters
        assert not np.array_equal(first[4]["T_bs"], start["T_bs"])
        # hs_cost / hs_reduced_system see the estimate
        assert abs(g.cost() - s1["final_cost"]) <= 1e-9 * s1["final_cost"]
        S_ref, g_ref = bref.reduced_system(wf, oracle, 1e4)
        S, gr = g.reduced_system(1e4)
        assert rel(S, S_ref) < 1e-6 and rel(gr, g_ref) < 1e-6, (rel(S, S_ref), rel(gr, g_ref))
        # a second solve starts at the first one's final cost
        s2 = g.solve(1)
        assert abs(s2["initial_cost"] - s1["final_cost"]) <= 1e-9 * s1["final_cost"]
        # snapshot / solve / restore / solve: bit-identical, IMU parameters included
        g.restore()
        back = g.imu()
        for k in IMU_NAMES:
            assert np.array_equal(back[k], start[k]), k
        s3 = g.solve(n)
        assert s3["iterations"] == s1["iterations"] and s3["final_cost"] == s1["final_cost"]
        again = (g.control_points(), g.landmarks(), g.bias(), g.gravity(), g.imu())
        assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]) and np.array_equal(again[3], first[3])
        assert np.array_equal(again[2][0], first[2][0]) and np.array_equal(again[2][1], first[2][1])
        for k in IMU_NAMES:
            assert np.array_equal(again[4][k], first[4][k]), k
        # set_imu overrides the estimate and keeps the flags
        m = w.imu
        a = [np.ascontiguousarray(np.asarray(m[k], float)) for k in IMU_NAMES]
        bg, ba = g.bias()
        d = ha.problem._d
        assert g.lib.set_imu(g.h, *[d(x) for x in a], int(m["bias_order"]), float(m["bias_t0"]), float(m["bias_dt"]), bg.shape[0], d(bg), d(ba), 0) == 0
        over = g.imu()
        for k in IMU_NAMES:
            assert np.array_equal(over[k], start[k]), k
        with ha.Problem(oracle_window(w, g), lib=oracle) as c:
            assert abs(g.cost() - c.cost()) <= 1e-9 * c.cost()
        assert g.solve(2)["num_iterations"] == 2  # (still estimating: the flags and the switch stand)
        assert not np.array_equal(g.imu()["T_bs"], start["T_bs"])


# The steps of test_hand_over that a getter between the solve and the next call would hide: the device holds the newest IMU parameters.
def test_set_imu_right_after_an_estimating_solve(hip, oracle):
    name, w, mode, n = WINDOWS[0]
    m = w.imu
    start = {k: np.ascontiguousarray(np.asarray(m[k], float)).reshape(-1) for k in IMU_NAMES}
    bg, ba = (np.ascontiguousarray(np.asarray(m[k], float)) for k in ("bias_g", "bias_a"))
    d = ha.problem._d
    with estimating(w, hip) as g:
        g.solve(n)
        assert g.lib.set_imu(g.h, *[d(start[k]) for k in IMU_NAMES], int(m["bias_order"]), float(m["bias_t0"]), float(m["bias_dt"]), bg.shape[0], d(bg), d(ba), 0) == 0
        over = g.imu()
        for k in IMU_NAMES:
            assert np.array_equal(over[k], start[k]), k
        assert not np.array_equal(g.control_points(), w.control_points)
        with ha.Problem(oracle_window(w, g), lib=oracle) as c:
            assert abs(g.cost() - c.cost()) <= 1e-9 * c.cost()


def test_restore_then_solve_without_a_getter(hip):
    name, w, mode, n = WINDOWS[0]
    with estimating(w, hip) as g:
        g.solve(n)
        first = (g.imu(), g.cameras())
    assert not np.array_equal(first[0]["T_bs"], np.asarray(w.imu["T_bs"], float).reshape(-1))
    with estimating(w, hip) as g:
        g.snapshot()
        s1 = g.solve(n)
        g.restore()
        s2 = g.solve(n)
        for f in SUMMARY:
            assert s2[f] == s1[f], f
        again = (g.imu(), g.cameras())
    for k in IMU_NAMES:
        assert np.array_equal(again[0][k], first[0][k]), k
    for a, b in zip(again[1], first[1]):
        assert np.array_equal(a, b)


def test_delta_append_keeps_the_estimated_imu(hip, oracle):
    name, w, mode, n = WINDOWS[0]
    with estimating(w, hip) as g:
        g.solve(n)
        est = g.imu()
        g.append_residuals(ha.HS_INERTIAL, w.inertial_stamps[:7], w.inertial_measurements[:7])
        g.stage()
        now = g.imu()
        for k in IMU_NAMES:
            assert np.array_equal(now[k], est[k]), k
        assert not np.array_equal(now["T_bs"], np.asarray(w.imu["T_bs"], float))
        w2 = oracle_window(w, g)
        w2.inertial_stamps = np.r_[w.inertial_stamps, w.inertial_stamps[:7]]
        w2.inertial_measurements = np.concatenate([w.inertial_measurements, w.inertial_measurements[:7]])
        with ha.Problem(w2, lib=oracle) as c:
            assert abs(g.cost() - c.cost()) <= 1e-9 * c.cost()
        g.retire_residuals_before(ha.HS_INERTIAL, float(np.sort(w.inertial_stamps)[5]))
        keep = w2.inertial_stamps >= float(np.sort(w.inertial_stamps)[5])
        w2.inertial_stamps, w2.inertial_measurements = w2.inertial_stamps[keep], w2.inertial_measurements[keep]
        with ha.Problem(w2, lib=oracle) as c:
            assert abs(g.cost() - c.cost()) <= 1e-9 * c.cost()
        s = g.solve(2)  # (and the solver goes on estimating on the changed window)
        assert s["num_iterations"] == 2


@pytest.mark.parametrize("name", ["k4_all_free_as_reference", "k5_i_g_X_a"])
def test_two_solves_are_bit_identical(name, hip, build_path):
    _, w, mode, n = WINDOWS[IDS.index(name)]
    outs = []
    for _ in range(2):
        with estimating(w, hip, mode) as g:
            s = g.solve(n)
            outs.append((s["iterations"], g.control_points(), g.landmarks(), *g.bias(), g.gravity(), *[g.imu()[k] for k in IMU_NAMES]))
    assert outs[0][0] == outs[1][0]
    for a, b in zip(outs[0][1:], outs[1][1:]):
        assert np.array_equal(a, b)


def test_free_blocks_reach_a_cost_no_higher_than_constant_blocks(hip, oracle):
    """The window is admitted only if the referee's two solves say so (a trust-region path is not monotone in the number of unknowns)."""
    name = "constant_gravity_T_bs_i_a"
    _, w, mode, n = WINDOWS[IDS.index(name)]
    _, sr_free, _ = referee(name, oracle)
    sr_const, _ = sref.solve(sref.constant_twin(w), oracle, n)
    print(name, "referee: free %.9g, constant %.9g" % (sr_free["final_cost"], sr_const["final_cost"]))
    assert sr_free["final_cost"] <= sr_const["final_cost"] * (1 + 1e-9)  # admission
    with estimating(w, hip) as a, ha.Problem(sref.constant_twin(w), lib=hip) as b:
        sa, sb = a.solve(n), b.solve(n)
    print(name, "device: free %.9g, constant %.9g" % (sa["final_cost"], sb["final_cost"]))
    assert sa["final_cost"] <= sb["final_cost"] * (1 + 1e-9)


class WithoutImuEntries:
    """The library as a handle sees it that never calls hs_set_imu_constancy or hs_set_imu_estimation."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name in ("set_imu_constancy", "set_imu_estimation"):
            raise AttributeError(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("which", ["visual", "inertial", "configs1_shaped"])
@pytest.mark.parametrize("flags", ["null", "all_set"])
def test_switch_on_with_constant_flags_is_bit_identical_to_the_default(which, flags, hip):
    w = {"visual": lambda: synthetic.small_visual(order=4, n_cp=18, n_landmarks=50, obs_pairs=3),
         "inertial": lambda: synthetic.small_inertial(order=4, n_cp=16),
         "configs1_shaped": lambda: synthetic.small_visual(order=4, n_cp=60, n_landmarks=150, obs_pairs=3, seed=13, span=0.5)}[which]()
    wc = copy.copy(w)
    wc.imu_constant = None if flags == "null" else np.ones(5, np.uint8)
    with ha.Problem(w, lib=WithoutImuEntries(hip)) as a, estimating(wc, hip) as b:
        assert a.dim_pose() == b.dim_pose()
        Sa, ga = a.reduced_system(1e4)
        Sb, gb = b.reduced_system(1e4)
        assert np.array_equal(Sa, Sb) and np.array_equal(ga, gb)
        sa, sb = a.solve(5), b.solve(5)
        for f in ("initial_cost", "final_cost", "num_iterations", "num_successful_steps", "termination"):
            assert sa[f] == sb[f], f
        assert sa["iterations"] == sb["iterations"]
        assert np.array_equal(a.control_points(), b.control_points())
        assert np.array_equal(a.landmarks(), b.landmarks())
        if w.imu is not None:
            for x, y in zip(a.bias() + (a.gravity(),), b.bias() + (b.gravity(),)):
                assert np.array_equal(x, y)


def test_switch_on_without_inertial_rows_changes_nothing(hip):
    e = synthetic.small_inertial(order=4, n_cp=16)  # an IMU with its bias splines, but no inertial row
    e.inertial_stamps, e.inertial_measurements = np.zeros(0), np.zeros((0, 6))
    ef = copy.copy(e)
    ef.imu_constant = imu_flags("tgasx")
    with ha.Problem(e, lib=WithoutImuEntries(hip)) as a, estimating(ef, hip) as b:
        assert a.dim_pose() == b.dim_pose()
        Sa, ga = a.reduced_system(1e4)
        Sb, gb = b.reduced_system(1e4)
        assert np.array_equal(Sa, Sb) and np.array_equal(ga, gb)
        sa, sb = a.solve(3), b.solve(3)
        assert sa["iterations"] == sb["iterations"] and sa["final_cost"] == sb["final_cost"]
        assert np.array_equal(a.control_points(), b.control_points()) and np.array_equal(a.landmarks(), b.landmarks())
        now = b.imu()
        for k in IMU_NAMES:
            assert np.array_equal(now[k], np.asarray(e.imu[k], float).reshape(-1))


def test_switch_off_refuses_as_before(hip):
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.imu_constant = imu_flags("t")
    with ha.Problem(w, lib=hip) as g:
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_solve.*hs_set_imu_constancy"):
            g.solve(5)
        today = g.lib.last_error(g.h)
        g.set_imu_estimation(True)
        g.solve(2)
        g.set_imu_estimation(False)
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_solve.*hs_set_imu_constancy"):
            g.solve(5)
        assert g.lib.last_error(g.h) == today
        assert today == (b"hs_solve: free IMU blocks (hs_set_imu_constancy) are not supported by the solver in this version; "
                         b"hs_reduced_system builds their system (DESIGN.md section 14)")


def test_get_imu_needs_an_imu(hip):
    with ha.Problem(synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3), lib=hip) as g:
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_get_imu"):
            g.imu()
    d = ha.problem._d
    w = synthetic.small_inertial(order=4, n_cp=16)
    with ha.Problem(w, lib=hip) as g:
        T = np.zeros(7)
        assert g.lib.get_imu(g.h, d(T), None, None, None, None) == 0  # (any pointer may be NULL)
        assert np.array_equal(T, np.asarray(w.imu["T_bs"], float))
        assert g.lib.get_imu(g.h, None, None, None, None, None) == 0


def cam_flags(w, **free):
    return csr.flags(w, **free)


def test_limits_and_refusals(hip, oracle):
    # the 170-unknown window of tests/test_gpu_imu_calibration.py::test_estimation_limits_do_not_count_the_imu_columns, both switches on
    w, rng = synthetic._visual_window(synthetic.SEED ^ 0x2f1, 4, 20, 30, 3)
    w = synthetic.add_imu(w, rng, 300, bias_dt=0.1)
    w.imu_constant = imu_flags("tgasx")
    w.cam_constant = cam_flags(w, cam0="t")
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_estimation(True)
        g.reduced_system(1e4)  # (IMU switch off: the IMU columns are not counted, the build is accepted as before)
        g.set_imu_estimation(True)
        with pytest.raises(ha.problem.HsError, match=r"\(1\).*128 bias / gravity \+ 36 free IMU coordinates \+ 6 free camera coordinates = 170, at most 137"):
            g.solve(2)
        g.set_imu_constancy(imu_flags("t"))  # 128 + 6 + 6 = 140
        with pytest.raises(ha.problem.HsError, match=r"\(1\).*128 bias / gravity \+ 6 free IMU coordinates \+ 6 free camera coordinates = 140, at most 137"):
            g.solve(2)
        g.set_camera_constancy(None)  # 128 + 6 = 134
        s = g.solve(2)
        assert s["num_iterations"] == 2 and g.dim_pose() - 6 * w.n_cp == 134
    # a window too long for the LDS-resident border forward sweep (the limit is checked before the border size)
    w = synthetic.small_inertial(order=4, n_cp=420, n_landmarks=60, obs_pairs=3, n_inertial=200, seed=2)
    w.imu_constant = imu_flags("t")
    with estimating(w, hip) as g:
        with pytest.raises(ha.problem.HsError, match=r"\(1\).*border forward sweep with free IMU coordinates: 420 control points, at most 400"):
            g.solve(2)
    # covariance, a weight matrix and sharded handles stay refused
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.imu_constant = imu_flags("t")
    with estimating(w, hip) as g:
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_compute_covariance.*hs_set_imu_constancy"):
            g.compute_covariance()
        g.set_weights(ha.HS_INERTIAL, np.eye(6))
        with pytest.raises(ha.problem.HsError, match=r"\(1\).*weight"):
            g.solve(2)
        g.set_weights(ha.HS_INERTIAL, None)
        assert g.lib.set_shard(g.h, 0, 2, 0) == 0
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_set_imu_constancy.*sharded"):
            g.solve(2)
        assert g.lib.set_shard(g.h, 0, 1, 0) == 0
        g.solve(1)
    # free cameras next to free IMU blocks with the IMU switch alone: the camera refusal, with its text
    wc = copy.copy(w)
    wc.cam_constant = cam_flags(w, cam1="i")
    with ha.Problem(wc, lib=hip) as g:
        g.set_imu_estimation(True)
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_solve: free camera blocks \(hs_set_camera_constancy\) are not supported by the solver"):
            g.solve(2)
        g.set_camera_estimation(True)
        g.solve(1)
