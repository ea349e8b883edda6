"""GPU parity tests: the HIP path (through the C ABI) against the oracle on the same seeded windows.

Tolerances: bit-exact for index / graph structure; 1e-6 relative (north_star) on residuals, Jacobians, normal equations
and solver trajectory — asserted much tighter (1e-9) where only round-off differs.
"""
import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


def windows():
    yield "pixel_k4", synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3)
    yield "pixel_k6", synthetic.small_visual(order=6, n_cp=20, n_landmarks=50, obs_pairs=3, seed=8)
    # order 5 (odd: the segment of a stamp starts (k - 1) / 2 = 2 control points before it, abstract.cpp:89 in integer arithmetic): instantiated since
    # round 4; visual + priors, and a window long enough for the two-ended factorisation
    yield "pixel_k5", synthetic.small_visual(order=5, n_cp=18, n_landmarks=50, obs_pairs=3, seed=21)
    yield "pixel_prior_k5", synthetic.small_visual(order=5, n_cp=18, n_landmarks=40, obs_pairs=4, seed=22, with_priors=30)
    yield "pixel_two_ended_k5", synthetic.small_visual(order=5, n_cp=66, n_landmarks=150, obs_pairs=3, seed=23, span=0.45)
    wb = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, bearing=True, seed=9)
    wb.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(12, np.uint8)]  # frozen old control points fix the gauge (optimizer.cpp:323-328)
    yield "bearing_k4", wb
    yield "pixel_prior_k4", synthetic.small_visual(order=4, n_cp=18, n_landmarks=40, obs_pairs=4, seed=10, with_priors=30)
    yield "prior_only", synthetic.config0(n_cp=32, n_prior=200)
    # feature tracks as long as the window (EuRoC-like 3 s tracks): every landmark couples ~all control points, the band is
    # wider than the register-resident factorisation handles and the wide-band kernel takes over
    yield "pixel_long_tracks_k4", synthetic.small_visual(order=4, n_cp=34, n_landmarks=80, obs_pairs=6, seed=11, span=3.2)
    # a window long enough (n_cp >= 4 bw) for the reduced system to be factored from both ends at once
    yield "pixel_two_ended_k4", synthetic.small_visual(order=4, n_cp=60, n_landmarks=150, obs_pairs=3, seed=13, span=0.5)
    yield "pixel_two_ended_k6", synthetic.small_visual(order=6, n_cp=72, n_landmarks=150, obs_pairs=3, seed=14, span=0.4)
    # medium tracks: band width 17 .. 22 (register-resident one-ended kernel with two tiles per lane)
    yield "pixel_medium_tracks_k4", synthetic.small_visual(order=4, n_cp=30, n_landmarks=80, obs_pairs=5, seed=15, span=1.6)
    yield "pixel_long_tracks_k6", synthetic.small_visual(order=6, n_cp=30, n_landmarks=80, obs_pairs=6, seed=12, span=3.0)


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
def test_structure_bit_exact(name, w, hip, oracle):
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        for t in (ha.HS_PIXEL, ha.HS_BEARING, ha.HS_PRIOR):
            n = g.num_residuals(t)
            assert n == c.num_residuals(t)
            for i in range(0, n, max(1, n // 25)):
                a, b = g.residual_layout(t, i), c.residual_layout(t, i)
                for k in a:
                    assert np.array_equal(a[k], b[k]), (name, t, i, k)


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
@pytest.mark.parametrize("robustify", [False, True])
def test_linearization(name, w, robustify, hip, oracle):
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        for t in (ha.HS_PIXEL, ha.HS_BEARING, ha.HS_PRIOR):
            if g.num_residuals(t) == 0:
                continue
            a, b = g.linearize(t, robustify), c.linearize(t, robustify)
            assert np.array_equal(a["first_cp"], b["first_cp"])
            for k in ("r", "J_state", "cost") + (("J_landmark",) if t != ha.HS_PRIOR else ()):
                assert rel(a[k], b[k]) < 1e-9, (name, t, k, rel(a[k], b[k]))
        assert abs(g.cost() - c.cost()) <= 1e-12 * c.cost()


from gpu_fixtures import build_path  # noqa: E402, F401  (both normal-equation builds: the fused build and the record path)


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
def test_reduced_system(name, w, hip, oracle, build_path):
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        Sg, gg = g.reduced_system(1e4)
        Sc, gc = c.reduced_system(1e4)
        assert rel(Sg, Sc) < 1e-9, rel(Sg, Sc)
        assert rel(gg, gc) < 1e-9, rel(gg, gc)
        assert np.array_equal(Sg, Sg.T)


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
def test_solve_trajectory(name, w, hip, oracle, build_path):
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        sg, sc = g.solve(5), c.solve(5)
        assert sg["num_iterations"] == sc["num_iterations"]
        assert sg["num_successful_steps"] == sc["num_successful_steps"]
        assert sg["termination"] == sc["termination"]
        for ig, ic in zip(sg["iterations"], sc["iterations"]):
            assert ig["step_is_successful"] == ic["step_is_successful"]
            # round-off differences between the two factorisations are amplified from one iteration to the next; the cost
            # is therefore compared relative to the scale of the problem (initial cost), the rest relatively
            assert abs(ig["cost"] - ic["cost"]) <= 1e-6 * abs(ic["cost"]) + 1e-8 * sc["initial_cost"], (name, ig["iteration"], ig["cost"], ic["cost"])
            for k in ("radius", "step_norm", "relative_decrease"):
                assert abs(ig[k] - ic[k]) <= 1e-5 * max(abs(ic[k]), 1e-12), (name, ig["iteration"], k, ig[k], ic[k])
        assert rel(g.control_points(), c.control_points()) < 1e-6
        if len(w.landmarks):
            assert rel(g.landmarks(), c.landmarks()) < 1e-6


def test_run_to_run_bit_reproducible(hip, build_path):
    w = synthetic.small_visual(order=4, n_cp=24, n_landmarks=300, obs_pairs=4, seed=11)
    outs = []
    for _ in range(3):
        with ha.Problem(w, lib=hip) as g:
            g.solve(5)
            outs.append((g.control_points().copy(), g.landmarks().copy()))
    for cp, lm in outs[1:]:
        assert np.array_equal(cp, outs[0][0]) and np.array_equal(lm, outs[0][1])


from util import check_against_golden, golden_cases, golden_window  # noqa: E402


@pytest.mark.parametrize("idx", range(len(golden_cases())))
def test_hip_matches_golden(idx, hip):
    """The HIP path against the independent 50-digit vectors (same bar as the oracle)."""
    case = golden_cases()[idx]
    if case["type"] == "inertial":
        pytest.skip("inertial factor: see test_gpu_inertial.py")
    with ha.Problem(golden_window(case), lib=hip) as p:
        check_against_golden(p, case, 1e-9)


def _quat_plus_jacobian(q):
    x, y, z, w = q
    return np.array([[w, z, -y], [-z, w, x], [y, -x, w], [-x, -y, -z]])  # columns e_i (x) q, rows (x, y, z, w)


@pytest.mark.parametrize("ftype", [ha.HS_PIXEL, ha.HS_BEARING, ha.HS_PRIOR])
def test_cost_function_evaluate_contract(ftype, hip, oracle):
    """Ceres-style single-block entry (exteroceptive.hpp:31): residuals equal the oracle's; ambient Jacobians agree after
    projection by the manifold's PlusJacobian (the ambient quaternion Jacobian is only defined up to its gauge)."""
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=20, obs_pairs=2, bearing=(ftype == ha.HS_BEARING), seed=12, with_priors=6)
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        for idx in (0, 3):
            blocks = g.parameter_blocks(ftype, idx)
            # evaluate away from the stored values to show the entry point honours `parameters`
            blocks[1] = blocks[1].copy()
            blocks[1][4:7] += 0.01
            n = len(blocks)
            want = [i < 4 or (ftype != ha.HS_PRIOR and i == n - 1) for i in range(n)]
            rg, Jg = g.cost_function_evaluate(ftype, idx, blocks, want)
            rc, Jc = c.cost_function_evaluate(ftype, idx, blocks, want)
            assert rel(rg, rc) < 1e-9
            r0, _ = g.cost_function_evaluate(ftype, idx, blocks)
            assert np.array_equal(r0, rg)
            scale = max(np.abs(J).max() for J in Jc if J is not None)  # a block's weight can vanish (B_3 = u^3/6 at u -> 0)
            for i in range(4):
                P = np.zeros((8, 6))
                P[:4, :3], P[4:7, 3:] = _quat_plus_jacobian(blocks[i][:4]), np.eye(3)
                assert np.abs(Jg[i] @ P - Jc[i] @ P).max() < 1e-9 * scale
                assert np.all(Jg[i][:, 7] == 0)
            if ftype != ha.HS_PRIOR:
                assert rel(Jg[-1], Jc[-1]) < 1e-9
            # sensor blocks: constant in the optimizer, but produced on request (tests/test_sensor_blocks.py)
            _, Jall = g.cost_function_evaluate(ftype, idx, blocks, [True] * n)
            assert all(J is not None and np.all(np.isfinite(J)) for J in Jall)


def test_sample_trajectory(hip, oracle):
    w = synthetic.small_visual(order=6, n_cp=24, n_landmarks=10, obs_pairs=2, seed=13)
    lo, hi = w.valid_range()
    st = np.linspace(lo, hi - 1e-6, 257)
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        a, b = g.sample_trajectory(st, derivatives=True), c.sample_trajectory(st, derivatives=True)
        for x, y in zip(a, b):
            assert rel(x, y) < 1e-10
        with pytest.raises(ha.HsError):
            g.sample_trajectory([hi + 1.0])


def test_sample_trajectory_after_a_solve_needs_no_getter(hip):
    """The evaluation calls send the spline the last solve left on the device, whether or not a getter fetched it in between."""
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=80, obs_pairs=4)
    lo, hi = w.valid_range()
    st = np.linspace(lo, hi - 1e-6, 9)
    with ha.Problem(w, lib=hip) as g:
        pre = g.sample_trajectory(st)
    with ha.Problem(w, lib=hip) as g:
        g.solve(2)
        a = g.sample_trajectory(st)
        g.control_points()
        b = g.sample_trajectory(st)
    assert np.array_equal(a, b) and not np.array_equal(a, pre)


@pytest.mark.parametrize("order", [4, 5, 6])
def test_process_tracks(order, hip, oracle):
    """Pixel -> bearing conversion and stereo triangulation through the spline (abstract.cpp:197-223,250-255)."""
    w = synthetic.small_visual(order=order, n_cp=14, n_landmarks=10, obs_pairs=2, seed=5)
    lo, hi = w.valid_range()
    rng = np.random.default_rng(11)
    n = 300
    px0 = np.stack([rng.uniform(0, 752, n), rng.uniform(0, 480, n)], -1)
    px1 = px0 + np.stack([rng.uniform(-40, -2, n), rng.normal(0, 0.5, n)], -1)
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        for stamp in (lo, 0.5 * (lo + hi), hi - 1e-6):
            a, b = g.process_tracks(stamp, px0, px1), c.process_tracks(stamp, px0, px1)
            for x, y in zip(a, b):
                assert np.abs(x - y).max() <= 1e-11 * max(1.0, np.abs(y).max())


def test_band_width_classes(hip):
    """The parametrised windows above really cover every factorisation path (look-ahead, two-ended, two tiles per lane, wide)."""
    got = {}
    for name, w in windows():
        with ha.Problem(w, lib=hip) as g:
            g.cost()
            got[name] = (g.lib.band_blocks(g.h), w.n_cp)
    assert got["pixel_k4"][0] <= 14
    assert 17 <= got["pixel_medium_tracks_k4"][0] <= 22, got
    assert got["pixel_long_tracks_k4"][0] >= 23
    bw, n = got["pixel_two_ended_k4"]
    assert bw <= 14 and n >= 4 * bw, got


def test_manifolds(hip, oracle):
    """hs_manifold_plus / _plus_jacobian (the retractions k_backsub_retract applies) and hs_manifold_minus / _minus_jacobian against the 100-digit vectors and,
    on a larger random batch, against the oracle."""
    from util import check_manifolds_against_golden
    w = synthetic.small_visual()
    with ha.Problem(w, lib=hip) as p, ha.Problem(w, lib=oracle) as o:
        assert check_manifolds_against_golden(p, 1e-14) <= 1e-14
        rng = np.random.default_rng(5)
        n = 1000
        q = rng.normal(size=(n, 4))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        x = np.concatenate([q, rng.normal(size=(n, 3)), rng.uniform(0, 10, size=(n, 1))], axis=1)
        d = rng.normal(size=(n, 6)) * rng.choice([0.0, 1e-8, 1e-2, 1.0], size=(n, 1))
        for kind, xs in ((ha.HS_MANIFOLD_CONTROL_POINT, x), (ha.HS_MANIFOLD_SE3, x[:, :7])):
            assert np.abs(p.manifold_plus(kind, xs, d) - o.manifold_plus(kind, xs, d)).max() <= 1e-14
            assert np.abs(p.manifold_plus_jacobian(kind, xs) - o.manifold_plus_jacobian(kind, xs)).max() <= 1e-15
            y = o.manifold_plus(kind, xs, d)
            assert np.abs(p.manifold_minus(kind, y, xs) - o.manifold_minus(kind, y, xs)).max() <= 1e-13
            assert np.abs(p.manifold_minus_jacobian(kind, xs) - o.manifold_minus_jacobian(kind, xs)).max() <= 1e-15
            small = np.abs(d[:, :3]).max(axis=1) < 1.5  # |delta| < pi: Minus inverts Plus
            assert np.abs(p.manifold_minus(kind, y, xs)[small] - d[small]).max() <= 1e-7  # (deltas of 1e-8 come back through acos-like conditioning)
        g = rng.normal(size=(n, 3)) * 9.8
        d2 = rng.normal(size=(n, 2)) * rng.choice([0.0, 1e-8, 1e-2, 1.0], size=(n, 1))
        assert np.abs(p.manifold_plus(ha.HS_MANIFOLD_SPHERE3, g, d2) - o.manifold_plus(ha.HS_MANIFOLD_SPHERE3, g, d2)).max() <= 1e-13
        assert np.abs(p.manifold_plus_jacobian(ha.HS_MANIFOLD_SPHERE3, g) - o.manifold_plus_jacobian(ha.HS_MANIFOLD_SPHERE3, g)).max() <= 1e-13
        y = o.manifold_plus(ha.HS_MANIFOLD_SPHERE3, g, d2)
        assert np.abs(p.manifold_minus(ha.HS_MANIFOLD_SPHERE3, y, g) - o.manifold_minus(ha.HS_MANIFOLD_SPHERE3, y, g)).max() <= 1e-12
        assert np.abs(p.manifold_minus_jacobian(ha.HS_MANIFOLD_SPHERE3, g) - o.manifold_minus_jacobian(ha.HS_MANIFOLD_SPHERE3, g)).max() <= 1e-13
        with pytest.raises(ha.HsError):
            p.manifold_plus(ha.HS_MANIFOLD_SPHERE3, np.zeros((1, 4)), np.zeros((1, 2)))


@pytest.mark.parametrize("name", ["config0", "config1", "config2", "config3"])
def test_baseline_configs_at_full_size(name, hip, oracle):
    """BASELINE.json configs[0..3] at their FULL sizes (1 k priors / 50 k pixel blocks / 50 k pixel + 10 k inertial blocks on an
    order-6 spline / 200 k blocks on 512 control points): cost, reduced normal equations and the whole 5-iteration LM trajectory
    of the HIP path against the oracle (which needs 0.1 - 10 s for these), plus run-to-run bit reproducibility at that size."""
    w = getattr(synthetic, name)()
    with ha.Problem(w, lib=hip) as g, ha.Problem(w, lib=oracle) as c:
        assert abs(g.cost() - c.cost()) <= 1e-11 * c.cost()
        Sg, gg = g.reduced_system(1e4)
        Sc, gc = c.reduced_system(1e4)
        assert rel(Sg, Sc) < 1e-9 and rel(gg, gc) < 1e-9, (rel(Sg, Sc), rel(gg, gc))
        assert np.array_equal(Sg, Sg.T)
        sg, sc = g.solve(5), c.solve(5)
        assert sg["num_iterations"] == sc["num_iterations"]
        assert sg["num_successful_steps"] == sc["num_successful_steps"] and sg["termination"] == sc["termination"]
        for ig, ic in zip(sg["iterations"], sc["iterations"]):
            assert ig["step_is_successful"] == ic["step_is_successful"]
            assert abs(ig["cost"] - ic["cost"]) <= 1e-6 * abs(ic["cost"]) + 1e-8 * sc["initial_cost"], (ig["iteration"], ig["cost"], ic["cost"])
        assert rel(g.control_points(), c.control_points()) < 1e-6
        if len(w.landmarks):
            assert rel(g.landmarks(), c.landmarks()) < 1e-6
        first = (g.control_points().copy(), g.landmarks().copy() if len(w.landmarks) else None)
    with ha.Problem(w, lib=hip) as g:
        g.solve(5)
        assert np.array_equal(g.control_points(), first[0])
        if first[1] is not None:
            assert np.array_equal(g.landmarks(), first[1])


@pytest.mark.parametrize("name", ["config1", "config2", "config3"])
def test_build_paths_agree_at_full_size(name, hip, monkeypatch):
    """The fused build (default) and the record path (HS_BUILD_PATH=records) of the same library on BASELINE.json configs[1..3] at full size:
    the same reduced normal equations to round-off, the same accept / reject decisions and the same 5-iteration result."""
    w = getattr(synthetic, name)()
    outs = []
    for path in ("fused", "records"):
        monkeypatch.setenv("HS_BUILD_PATH", path)
        with ha.Problem(w, lib=hip) as g:
            S, gr = g.reduced_system(1e4)
            s = g.solve(5)
            outs.append((S, gr, s, g.control_points().copy(), g.landmarks().copy()))
    (S0, g0, s0, cp0, lm0), (S1, g1, s1, cp1, lm1) = outs
    assert rel(S0, S1) < 1e-11 and rel(g0, g1) < 1e-11, (rel(S0, S1), rel(g0, g1))
    assert [it["step_is_successful"] for it in s0["iterations"]] == [it["step_is_successful"] for it in s1["iterations"]]
    assert abs(s0["final_cost"] - s1["final_cost"]) <= 1e-8 * s1["final_cost"]
    assert rel(cp0, cp1) < 1e-7 and rel(lm0, lm1) < 1e-7


def test_process_tracks_matches_golden(hip):
    """hs_process_tracks against the 100-digit vectors of tests/golden/make_tracks_golden.py (same bar as the oracle's CPU test)."""
    from util import check_tracks_against_golden
    assert check_tracks_against_golden(hip, 1e-9) <= 1e-9


def test_hip_matches_golden_order5(hip):
    """Order 5 against its own 100-digit vectors (tests/golden/factors_k5.json): every factor incl. the inertial one, every parameter block."""
    from util import golden_cases_k5
    for case in golden_cases_k5():
        with ha.Problem(golden_window(case), lib=hip) as p:
            check_against_golden(p, case, 1e-9)
