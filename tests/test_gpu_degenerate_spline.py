"""GPU tests: the spline at rest. Control points whose relative rotations are zero, tiny, on either side of the thresholds of rel_log /
exp_scaled / jr_inv_coef / so3_log / so3_coef (csrc/device_spline.hpp, csrc/device_math.hpp) or stored with flipped quaternion signs, on
every kernel route that evaluates the spline:

  linearize (record-path kernels), sample_trajectory (spline_full<K, false>), process_tracks (spline_pose), cost_function_evaluate
  (k_sensor_*), the fused and the record build of the reduced system, solve, compute_covariance / sample_covariance (k_cov_sample)

against the 100-digit vectors of tests/golden/make_degenerate_golden.py where a route has vectors, against the oracle elsewhere, and against
itself under a change of quaternion signs. The device's sincos, atan2, sqrt and rsqrt are not the host's; the CPU tests of the same inputs
(test_degenerate_golden.py, test_emulated_spline.py, test_degenerate_windows.py) cannot see them."""
import copy

import numpy as np
import pytest

import degenerate_windows as dw
import hyperslam_amd as ha
from gpu_fixtures import build_path  # noqa: F401
from hyperslam_amd import synthetic
from test_sensor_blocks import block_kinds
from util import TYPE_ID, check_against_golden, golden_cases_degenerate, golden_window

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max()))


@pytest.fixture(scope="module")
def cases():
    return golden_cases_degenerate()


# ---- 1. the 100-digit vectors through linearize ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ftype", ["pixel", "bearing", "prior", "inertial"])
def test_hip_matches_degenerate_golden(ftype, cases, hip):
    worst = {}
    n = 0
    for case in cases:
        if case["type"] != ftype:
            continue
        n += 1
        with ha.Problem(golden_window(case), lib=hip) as p:
            errs = check_against_golden(p, case, 1e-9)
        key = "prior_small" if case["variant"] == "prior_small" else ftype
        if max(errs.values()) > worst.get(key, (0.0,))[0]:
            worst[key] = (max(errs.values()), case["pattern"], case["inputs"]["k"], max(errs, key=errs.get))
    assert n == (69 if ftype == "prior" else 51)
    print("device linearize against the degenerate vectors, worst relative error:", worst)


# ---- 2. trajectory sampling: the only route through spline_full<K, false> ---------------------------------------------------------------------
def test_sample_trajectory_against_degenerate_golden(cases, hip):
    worst = dict(q=0.0, p=0.0, w=0.0, alpha=0.0, v=0.0, a=0.0)

    def check(name, got, want, tag):
        want = np.asarray(want, float)
        e = float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))
        assert e <= 1e-10, (tag, name, e)
        worst[name] = max(worst[name], e)

    n_rates = 0
    for case in cases:
        P, out = case["inputs"], case["outputs"]
        tag = (case["type"], case["pattern"], case["variant"], P["k"])
        with ha.Problem(golden_window(case), lib=hip) as p:
            pose, vel, acc = p.sample_trajectory([P["stamp"]], derivatives=True)
        q = np.asarray(out["pose"][:4])
        check("q", pose[0, :4] * np.sign(pose[0, :4] @ q), q, tag)
        check("p", pose[0, 4:], out["pose"][4:], tag)
        if "w_b" in out:
            n_rates += 1
            check("w", vel[0, :3], out["w_b"], tag)
            check("alpha", acc[0, :3], out["alpha_b"], tag)
        if "v_w" in out:
            check("v", vel[0, 3:], out["v_w"], tag)
            check("a", acc[0, 3:], out["a_w"], tag)
    assert n_rates == 33 + 51
    print("device sample_trajectory against the degenerate vectors, worst error relative to max(1, |ref|):", worst)


# ---- 3. two more routes against the oracle ---------------------------------------------------------------------------------------------
def test_process_tracks_on_degenerate_control_points(cases, hip, oracle):
    """spline_pose: the stereo triangulation through the pose at the case's stamp (one case per pattern, order and stamp variant)."""
    rng = np.random.default_rng(11)
    n = 40
    px0 = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], -1)
    px1 = px0 + np.stack([rng.uniform(-40, -2, n), rng.normal(0, 0.5, n)], -1)
    worst, count = 0.0, 0
    for case in cases:
        if case["type"] != "bearing":
            continue
        P = case["inputs"]
        cps = np.array(P["cps"], float)
        w = ha.Window(order=P["k"], t0=float(cps[0, 7]), dt=0.1, control_points=cps, cam_T_bs=synthetic.EUROC_CAM_T_BS.copy(),
                      cam_intrinsics=synthetic.EUROC_CAM_INTRINSICS.copy(), cam_distortion=synthetic.EUROC_CAM_DISTORTION.copy())
        with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
            a, b = g.process_tracks(P["stamp"], px0, px1), c.process_tracks(P["stamp"], px0, px1)
        for x, y in zip(a, b):
            e = float(np.abs(x - y).max()) / max(1.0, float(np.abs(y).max()))
            assert e <= 1e-11, (case["pattern"], case["variant"], P["k"], e)
            worst = max(worst, e)
        count += 1
    assert count == 51
    print("device process_tracks against the oracle on the degenerate control points, worst:", worst)


@pytest.mark.parametrize("ftype", ["pixel", "bearing", "prior"])
def test_cost_function_evaluate_on_degenerate_golden(ftype, cases, hip, oracle):
    """k_sensor_*: residual and every block's ambient Jacobian (projected on the tangent: the quaternion Jacobian is defined up to its gauge)
    against the oracle, relative to the largest Jacobian entry of the residual."""
    t = TYPE_ID[ftype]
    worst = 0.0
    for case in cases:
        if case["type"] != ftype:
            continue
        w = golden_window(case)
        kinds = block_kinds(t, w.order, 0)
        with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
            blocks = g.parameter_blocks(t, 0)
            assert all(np.array_equal(x, y) for x, y in zip(blocks, c.parameter_blocks(t, 0)))
            rg, Jg = g.cost_function_evaluate(t, 0, blocks, [True] * len(blocks))
            rc, Jc = c.cost_function_evaluate(t, 0, blocks, [True] * len(blocks))
            tag = (ftype, case["pattern"], case["variant"], w.order)
            assert rel(rg, rc) < 1e-9, (tag, rel(rg, rc))
            scale = max(np.abs(J).max() for J in Jc)
            for bi, kind in enumerate(kinds):
                Pj = c.manifold_plus_jacobian(kind, blocks[bi][None, :])[0]
                e = float(np.abs(Jg[bi] @ Pj - Jc[bi] @ Pj).max()) / scale
                assert e <= 1e-9, (tag, bi, e)
                worst = max(worst, e)
    print(f"device cost_function_evaluate ({ftype}) against the oracle, worst Jacobian error:", worst)


# ---- 4. at-rest windows, both build paths -------------------------------------------------------------------------------------------------
def rest_windows():
    for k in dw.ORDERS:
        yield f"small_k{k}_0", dw.small(k, "0")
        yield f"small_k{k}_thresholds_flip", dw.small(k, "thresholds", flip=True)
        yield f"imu_k{k}_{'0' if k != 5 else 'thresholds'}", dw.with_imu(k, "0" if k != 5 else "thresholds", flip=k == 6)
    yield "small_k5_1e-9_bearing", dw.small(5, "1e-9", bearing=True)
    yield "small_k4_thresholds_bearing_flip", dw.small(4, "thresholds", bearing=True, flip=True)
    yield "held_k6_0", dw.held(6, "0")
    yield "long_k4_thresholds", dw.long_window("thresholds")


REST = list(rest_windows())
REST_IDS = [n for n, _ in REST]


def problems(w, hip, oracle):
    g, c = ha.Problem(w, lib=hip), ha.Problem(w, lib=oracle)
    if w.imu is not None:  # (non-identity IMU parameters: the derivative of the prediction on both sides)
        g.set_inertial_jacobian(ha.HS_INERTIAL_EXACT)
        c.set_inertial_jacobian(ha.HS_INERTIAL_EXACT)
    return g, c


@pytest.mark.parametrize("name,w", REST, ids=REST_IDS)
@pytest.mark.parametrize("robustify", [False, True])
def test_linearization_at_rest(name, w, robustify, hip, oracle):
    g, c = problems(w, hip, oracle)
    with g, c:
        for t in (ha.HS_PIXEL, ha.HS_BEARING, ha.HS_PRIOR, ha.HS_INERTIAL):
            if g.num_residuals(t) == 0:
                continue
            a, b = g.linearize(t, robustify), c.linearize(t, robustify)
            assert np.array_equal(a["first_cp"], b["first_cp"])
            keys = {ha.HS_PRIOR: (), ha.HS_INERTIAL: ("J_bias_g", "J_bias_a", "J_gravity")}.get(t, ("J_landmark",))
            for k in ("r", "J_state", "cost") + keys:
                assert rel(a[k], b[k]) < 1e-9, (name, t, k, rel(a[k], b[k]))
        assert abs(g.cost() - c.cost()) <= 1e-12 * c.cost()


@pytest.mark.parametrize("name,w", REST, ids=REST_IDS)
def test_reduced_system_at_rest(name, w, hip, oracle, build_path):  # noqa: F811
    g, c = problems(w, hip, oracle)
    with g, c:
        Sg, gg = g.reduced_system(1e4)
        Sc, gc = c.reduced_system(1e4)
        assert rel(Sg, Sc) < 1e-9, rel(Sg, Sc)
        assert rel(gg, gc) < 1e-9, rel(gg, gc)
        assert np.array_equal(Sg, Sg.T)
        if name == "long_k4_thresholds":
            bw = g.lib.band_blocks(g.h)
            assert w.n_cp >= 4 * bw, (bw, "the window must take the two-ended factorisation")


@pytest.mark.parametrize("name,w", REST, ids=REST_IDS)
def test_solve_at_rest(name, w, hip, oracle, build_path):  # noqa: F811
    """The bars of test_solve_trajectory (and of test_bordered_solve_trajectory for the bias points and gravity)."""
    g, c = problems(w, hip, oracle)
    with g, c:
        sg, sc = g.solve(5), c.solve(5)
        assert sg["num_iterations"] == sc["num_iterations"] == 5
        assert sg["num_successful_steps"] == sc["num_successful_steps"]
        assert sg["termination"] == sc["termination"]
        for ig, ic in zip(sg["iterations"], sc["iterations"]):
            assert ig["step_is_successful"] == ic["step_is_successful"]
            assert abs(ig["cost"] - ic["cost"]) <= 1e-6 * abs(ic["cost"]) + 1e-8 * sc["initial_cost"], (name, ig["iteration"], ig["cost"], ic["cost"])
            for k in ("radius", "step_norm", "relative_decrease"):
                assert abs(ig[k] - ic[k]) <= 1e-5 * max(abs(ic[k]), 1e-12), (name, ig["iteration"], k, ig[k], ic[k])
        assert rel(g.control_points(), c.control_points()) < 1e-6
        assert rel(g.landmarks(), c.landmarks()) < 1e-6
        if w.imu is not None:
            bg, ba = g.bias()
            cg, ca = c.bias()
            assert rel(g.gravity(), c.gravity()) < 1e-6 and rel(bg, cg) < 1e-6 and rel(ba, ca) < 1e-6
        if w.rotation_constant:  # still at rest: every iteration of this solve ran in the series branches
            assert np.array_equal(g.control_points()[:, :4], w.control_points[:, :4]) and dw.pairs_below_t2(g.control_points()).all()


# ---- 5. covariance on an at-rest window ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", dw.ORDERS)
def test_covariance_at_rest(order, hip, oracle):
    """hs_compute_covariance and the sampled pose covariance (k_cov_sample: spline_pose_jac, and so3_coef at a zero residual) with the referee
    and the bars of test_gpu_covariance.py."""
    from test_gpu_covariance import bar, check_window, referee
    w = dw.small(order, "0", flip=order == 5)
    check_window(w, hip, oracle)
    Sigma, _, cond = referee(w, oracle)
    lo, hi = w.valid_range()
    stamps = np.r_[w.t0 + w.dt * np.arange((order - 1) // 2, (order - 1) // 2 + 4), np.linspace(lo, hi - 1e-6, 11)]
    stamps = stamps[(stamps >= lo) & (stamps < hi)]
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
    for i in range(len(stamps)):
        f = 6 * L["first_cp"][i]
        J = L["J_state"][i]
        want = J @ Sigma[f:f + 6 * order, f:f + 6 * order] @ J.T
        # (a pose that depends on constant control points only has zero covariance; at a knot the last control point of the segment enters
        # with weight u^(k-1) / (k-1)!, and u is 0 for the oracle, which reads the knots from the rows, and 3e-16 for the product, which
        # derives them from t0 + j dt: 1e-130 against 0. The floor of the scale is far below any covariance of the window, 1e-9 and up.)
        err = np.abs(got[i] - want).max() / max(np.abs(want).max(), 1e-30)
        assert err < bar(cond), (i, stamps[i], err)


# ---- 6. the sign of a stored quaternion changes nothing ---------------------------------------------------------------------------------------
def sign_pairs():
    for k in dw.ORDERS:
        yield f"small_k{k}_thresholds", dw.small(k, "thresholds"), dw.small(k, "thresholds", flip=True)
    yield "small_k4_0_bearing", dw.small(4, "0", bearing=True), dw.small(4, "0", bearing=True, flip=True)
    yield "imu_k6_0", dw.with_imu(6, "0"), dw.with_imu(6, "0", flip=True)
    yield "long_k4_thresholds", dw.long_window("thresholds"), dw.long_window("thresholds", flip=True)
    w = synthetic.small_visual(order=5, n_cp=16, n_landmarks=40, obs_pairs=3, with_priors=12)
    w.cp_constant = np.r_[np.ones(5, np.uint8), np.zeros(11, np.uint8)]
    yield "moving_k5", w, dw.negate_odd_control_points(w)


SIGN = list(sign_pairs())


@pytest.mark.parametrize("name,w,v", SIGN, ids=[n for n, _, _ in SIGN])
def test_quaternion_signs_change_nothing(name, w, v, hip):
    """A window against its twin whose odd control points are stored as -q, on the product library alone: everything agrees to 1e-13 (in the
    oracle: exactly), a solve keeps every sign (quat_plus multiplies from the left), and |control_points| agree entry by entry to 1e-12."""
    assert np.array_equal(w.control_points[1::2, :4], -v.control_points[1::2, :4]) and np.array_equal(w.control_points[0::2], v.control_points[0::2])

    def same(a, b, what, tol=1e-13):
        a, b = np.asarray(a, float), np.asarray(b, float)
        assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-300), (name, what, np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))

    lo, hi = w.valid_range()
    stamps = np.linspace(lo, hi - 1e-6, 17)
    out = []
    for x in (w, v):
        with ha.Problem(x, lib=hip) as g:
            if x.imu is not None:
                g.set_inertial_jacobian(ha.HS_INERTIAL_EXACT)
            o = dict(cost=g.cost(), lin={}, poses=g.sample_trajectory(stamps))
            for t in (ha.HS_PIXEL, ha.HS_BEARING, ha.HS_PRIOR, ha.HS_INERTIAL):
                if g.num_residuals(t):
                    o["lin"][t] = g.linearize(t, True)
            o["S"], o["g"] = g.reduced_system(1e4)
            if x.imu is None:  # (the IMU window keeps its trailing bias control points, which no residual reaches: no covariance)
                g.compute_covariance()
                o["cov"], o["pose_cov"] = g.covariance(), g.sample_covariance(stamps)
            o["solve"] = g.solve(5)
            o["cp"], o["lm"] = g.control_points().copy(), g.landmarks().copy()
            out.append(o)
    a, b = out
    same(a["cost"], b["cost"], "cost")
    assert a["lin"].keys() == b["lin"].keys()
    for t in a["lin"]:
        for k, val in a["lin"][t].items():
            if val is not None and np.asarray(val).dtype.kind == "f" and np.size(val):
                same(val, b["lin"][t][k], f"linearize {t} {k}")
    same(a["S"], b["S"], "reduced S")
    same(a["g"], b["g"], "reduced g")
    sign = np.sign(np.sum(a["poses"][:, :4] * b["poses"][:, :4], axis=1, keepdims=True))
    same(a["poses"][:, :4] * sign, b["poses"][:, :4], "sampled rotations")
    same(a["poses"][:, 4:], b["poses"][:, 4:], "sampled positions")
    if "cov" in a:
        for k in a["cov"]:
            if np.size(a["cov"][k]):
                ok = ~np.isnan(b["cov"][k])
                assert np.array_equal(np.isnan(a["cov"][k]), ~ok)
                same(a["cov"][k][ok], b["cov"][k][ok], f"covariance {k}")
        same(a["pose_cov"], b["pose_cov"], "sampled covariance")
    sa, sb = a["solve"], b["solve"]
    assert sa["num_iterations"] == sb["num_iterations"] == 5 and sa["num_successful_steps"] == sb["num_successful_steps"]
    for ia, ib in zip(sa["iterations"], sb["iterations"]):
        assert ia["step_is_successful"] == ib["step_is_successful"] and ia["step_is_valid"] == ib["step_is_valid"]
        for k in ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "radius"):
            assert abs(ia[k] - ib[k]) <= 1e-13 * max(abs(ib[k]), 1e-300), (name, ia["iteration"], k, ia[k], ib[k])
    assert np.abs(np.abs(a["cp"]) - np.abs(b["cp"])).max() <= 1e-12
    same(a["lm"], b["lm"], "landmarks after the solve", 1e-12)
    # every negated quaternion is still negated, every other one still is not
    dots = np.sum(a["cp"][:, :4] * b["cp"][:, :4], axis=1)
    assert (dots[1::2] < -0.999).all() and (dots[0::2] > 0.999).all()
