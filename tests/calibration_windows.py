"""Windows with free camera blocks for the device parity tests and sweeps, and the host-side rules that say which kernels solve
them. Everything here runs without a GPU: the generator and the acceptance rule of the solve sweep consult the oracle and the numpy referees only.

cases(n, seed)        random windows in the spirit of tools/fuzz_parity.py::cases, every one with at least one free camera block
solve_acceptance(...) the rule by which the solve sweep takes or leaves a candidate (CPU quantities alone)
band_blocks(w)        the band width hs_band_blocks reports, restated from csrc/host_structure.hpp
factor_route(...)     launch_factor's choice among the one-ended kernels (csrc/host_launch.hpp), restated
tests/test_gpu_calibration_routes.py asserts the routes on the device's own hs_band_blocks / hs_dim_pose; tests/test_calibration_windows.py pins
band_blocks and the generator on the CPU."""
import copy

import numpy as np

from hyperslam_amd import synthetic

import calibration_solve_referee as sref
from calibration_referee import camera_columns

MAX_BORDER = 137  # border unknowns the LDS border solve takes (bias + gravity + camera columns; prepare() refuses more)
MAX_BAND = 42     # control points a track may touch (6 bw <= 256)


def band_blocks(w):
    """hs_band_blocks of window w: the most control points one landmark's observations touch, at least the spline order (host_structure.hpp:
    first control point of a stamp = floor((t - t0) / dt) - (k - 1) // 2, a segment touches k of them)."""
    k = w.order
    stamp = np.r_[np.asarray(w.pixel_stamps, float), np.asarray(w.bearing_stamps, float)]
    lm = np.r_[np.asarray(w.pixel_landmark, int), np.asarray(w.bearing_landmark, int)]
    if len(stamp) == 0:
        return k
    first = (np.floor((stamp - w.t0) / w.dt) - (k - 1) // 2).astype(int)
    lo, hi = np.full(len(w.landmarks), 1 << 30), np.full(len(w.landmarks), -1)
    np.minimum.at(lo, lm, first)
    np.maximum.at(hi, lm, first + k - 1)
    return int(max(k, (hi - lo + 1).max()))


def frozen_prefix(w):
    """Leading constant control points (hs_problem::frozen_prefix): their block rows are decoupled from the factorisation."""
    if w.cp_constant is None:
        return 0
    c = np.asarray(w.cp_constant, bool)
    return int(len(c) if c.all() else np.argmin(c))


def la_compute_waves(bw):
    """kernels_factor.hpp: compute waves of k_band_factor_la (3 up to 14 band blocks, 4 for 15 and 16, 0: the kernel does not take the band)."""
    return 3 if ((bw + 2) // 3) * (bw - 2) <= 64 else 4 if ((bw + 3) // 4) * (bw - 2) <= 64 else 0


def dense_factor_fits(n, bw):
    """kernels_factor.hpp: k_dense_factor holds n <= 128 block rows and at most 2 x 448 band / right-hand-side tiles."""
    return n <= 128 and sum(min(n - i, bw) for i in range(n)) <= 896


def factor_route(bw, n_cp, f0, nb):
    """launch_factor for a handle with free camera coordinates (T.nc > 0: never two-ended). bw = hs_band_blocks, f0 = frozen prefix,
    nb = every border column (hs_dim_pose - 6 n_cp). Returns (factorisation, backward sweep, border solve); the one-launch dense solve has
    neither of the latter two."""
    f0 = min(f0, n_cp - 1)
    n_eff = n_cp - f0
    if 6 * n_eff + nb + 1 <= 256:  # use_dense_mx / dense_mx_fits
        return "k_dense_solve_mx", None, None
    if bw > 14 and n_eff <= 2 * bw and dense_factor_fits(n_eff, min(bw, n_eff)):
        factor = "k_dense_factor"
    elif la_compute_waves(bw) == 3:
        factor = "k_band_factor_la<1,3>"
    elif la_compute_waves(bw) == 4:
        factor = "k_band_factor_la<1,4>"
    elif bw * bw <= 256:
        factor = "k_band_factor<1>"
    elif bw <= 21:
        factor = "k_band_factor<2>"
    else:
        factor = "k_band_factor_wide"
    backward = "k_band_backward_sb" if 6 * (bw - 1) <= 96 else "k_band_backward"
    if nb + 1 <= 128:  # launch_border_solve: the register Cholesky on 16 R columns, R = 3 .. 8; beyond it the LDS version
        border = "k_border_solve_reg<%d>" % min(8, max(3, (nb + 1 + 15) // 16))
    else:
        border = "k_border_solve"
    return factor, backward, border


def border_forward_lanes(bw):
    """Lanes of k_border_forward: one per pending row, whole waves, at least two."""
    return max(128, 64 * ((6 * (bw - 1) + 63) // 64))


def cases(n_cases, seed):
    """(description line, window) of a sweep, deterministic in the seed: spline order 4 / 5 / 6, 8 .. 64 control points, tracks of 0.3 s to
    window-wide (capped at the band limit), pixel or bearing rows, with or without an IMU whose bias knot spacing is drawn so that the border
    size varies (never beyond the border solve's limit), pose priors, frozen prefixes, constant landmarks, rotation- / translation-only
    splines, and a random non-empty subset of the six camera blocks [T_bs, intrinsics, distortion] x 2 free."""
    rng = np.random.default_rng(seed)
    for case in range(n_cases):
        order = int(rng.choice([4, 4, 5, 6]))
        n_cp = int(rng.integers(max(8, order + 2), 65))
        imu = bool(rng.random() < 0.4)
        span = float(rng.choice([0.3, 0.6, 1.0, 1.6, 2.4, 0.1 * n_cp]))
        span = min(span, 0.1 * (MAX_BAND - order - 1))  # (a track of `span` seconds touches at most span / dt + 1 + k control points)
        n_lm = int(rng.integers(30, 151))
        pairs = int(rng.integers(2, 6))
        bearing = bool(rng.random() < 0.3)
        wseed = int(rng.integers(1, 1 << 20))
        priors = int(rng.integers(4, 40)) if rng.random() < 0.4 else 0
        free = np.zeros(6, bool)
        while not free.any():
            free = rng.random(6) < 0.35
        w = synthetic.small_visual(order=order, n_cp=n_cp, n_landmarks=n_lm, obs_pairs=pairs, bearing=bearing, seed=wseed, span=span, with_priors=priors)
        w.cam_constant = (~free).reshape(2, 3).astype(np.uint8)
        nc = camera_columns(w)[1]
        n_bias = 0
        if imu:
            lo, hi = w.valid_range()
            most = min(18, (MAX_BORDER - nc - 2) // 6 - 4)  # n_bias = ceil((hi - lo) / bias_dt) + bias order
            m = int(rng.integers(1, most + 1))
            synthetic.add_imu(w, synthetic.SplitMix64(wseed), int(rng.integers(60, 500)), bias_dt=(hi - lo) / m * 1.001)
            n_bias = len(w.imu["bias_g"])
            assert 6 * n_bias + 2 + nc <= MAX_BORDER
        frozen = int(rng.integers(1, max(2, n_cp // 2))) if rng.random() < 0.7 else 0
        if frozen:
            w.cp_constant = np.r_[np.ones(frozen, np.uint8), np.zeros(n_cp - frozen, np.uint8)]
        u = rng.random()
        if u < 0.1:
            w.rotation_constant = True
        elif u < 0.2:
            w.translation_constant = True
        if rng.random() < 0.3:
            w.landmark_constant = (rng.random(n_lm) < 0.15).astype(np.uint8)
        bw = band_blocks(w)
        assert bw <= MAX_BAND, bw
        blocks = "".join(("tid"[i % 3] if free[i] else "-") for i in range(6))
        yield (f"case {case:3d}: k {order} n_cp {n_cp:2d} bw {bw:2d} imu {int(imu)} n_bias {n_bias:2d} span {span:3.1f} lm {n_lm:3d} pairs {pairs} bearing {int(bearing)} "
               f"priors {priors:2d} frozen {frozen:2d} rc {int(w.rotation_constant)} tc {int(w.translation_constant)} lmc {int(w.landmark_constant is not None)} "
               f"free {blocks[:3]}|{blocks[3:]} wseed {wseed}"), w


def conditioning(w, oracle):
    """(cond of the reduced system with the free camera blocks, cond with constant cameras, whether the pair meets the rule of
    tests/test_gpu_calibration_solve.py::test_solve_against_referee: freeing the cameras at most doubles it, and below 1e7 without an IMU)."""
    w_const = copy.copy(w)
    w_const.cam_constant = None
    cond_free, cond_const = sref.condition(w, oracle), sref.condition(w_const, oracle)
    ok = bool(np.isfinite(cond_free) and cond_free <= 2.0 * cond_const and (w.imu is not None or cond_free < 1e7))
    return cond_free, cond_const, ok


def solve_acceptance(w, oracle, iterations):
    """The solve sweep's acceptance rule, from CPU quantities alone: the conditioning rule above, and no iteration of the referee's solve with a
    relative decrease within 1e-3 of the threshold of the step decision (min_relative_decrease = 1e-3) — an ill-conditioned window, or a
    decision on the edge, amplifies the rounding of BOTH sides. Returns (accepted, reason, referee summary, referee end point)."""
    cond_free, cond_const, ok = conditioning(w, oracle)
    if not ok:
        return False, "cond %.3g free / %.3g constant" % (cond_free, cond_const), None, None
    sr, wf = sref.solve(w, oracle, iterations)
    for it in sr["iterations"][1:]:
        if it["step_is_valid"] and abs(it["relative_decrease"] - 1e-3) <= 1e-3:
            return False, "iteration %d: relative decrease %.3g next to the threshold" % (it["iteration"], it["relative_decrease"]), None, None
    return True, "cond %.3g free / %.3g constant" % (cond_free, cond_const), sr, wf


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def check_build(w, hip, reference):
    """hs_reduced_system against reference = calibration_referee.reduced_system(w, oracle, 1e4) at the bars of
    tests/test_gpu_calibration.py::test_reduced_system_against_referee: 1e-9 relative, symmetric, two calls bit-identical."""
    import hyperslam_amd as ha
    S_ref, g_ref = reference
    nc = camera_columns(w)[1]
    with ha.Problem(w, lib=hip) as g:
        assert g.dim_pose() == S_ref.shape[0]
        S, gr = g.reduced_system(1e4)
        S2, gr2 = g.reduced_system(1e4)
    assert rel(S, S_ref) < 1e-9, rel(S, S_ref)
    assert rel(gr, g_ref) < 1e-9, rel(gr, g_ref)
    if nc:
        cam = slice(S.shape[0] - nc, S.shape[0])
        assert rel(S[:, cam], S_ref[:, cam]) < 1e-9, rel(S[:, cam], S_ref[:, cam])
        assert rel(gr[cam], g_ref[cam]) < 1e-9, rel(gr[cam], g_ref[cam])
    assert np.array_equal(S, S.T)
    assert np.array_equal(S, S2) and np.array_equal(gr, gr2)


def check_solve(w, hip, sr, wf, iterations, name):
    """hs_solve estimating the free blocks against the referee's summary sr and end point wf, at the bars of tests/test_gpu_calibration_solve.py."""
    import hyperslam_amd as ha
    from test_gpu_calibration_solve import check_end_point, check_trajectory
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_estimation(True)
        sg = g.solve(iterations)
        check_trajectory(sg, sr, name)
        assert abs(sg["final_cost"] - sr["final_cost"]) <= 1e-6 * sr["final_cost"] + 1e-8 * sr["initial_cost"]
        check_end_point(g, wf, name)
