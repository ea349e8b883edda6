"""Per-camera distortion models on the GPU (hs_set_camera_models: radial-tangential and equidistant) against the numpy referee of
tests/camera_model_referee.py — the oracle's pinhole chain with the model composed on top — which tests/test_camera_model_referee.py pins to
the oracle (radial-tangential) and to mpmath (equidistant). Inside `cmr.driving()` the existing referees (reduced system, LM solve, camera
covariance) run on that referee, so every level of the library is compared at the bar its radial-tangential test has.

Windows: tests/camera_model_windows.py — f ~ 190 on 512 x 512, plane radii from the optical axis (exactly, in axis_window) to beyond 1.5
(tests/test_camera_model_referee.py::test_windows_span_the_plane). Solve windows are admitted by rules evaluated from the referee alone and
asserted first: at least two accepted steps, no relative decrease within 1e-3 of the acceptance threshold 1e-3. Seeds chosen on the CPU so
that none had to be dropped: small_visual seed 7 (constant cameras, both model pairs; estimation with camera 1's distortion free) and
seed 10 (covariance). The sweep draws its 20 windows from numpy seed 20240611."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import calibration_referee
import calibration_solve_referee as sref
import calibration_windows
import camera_covariance_referee as ccr
import camera_model_referee as cmr
import camera_model_windows as cw
from camera_model_windows import EQUI, RADTAN
from test_gpu_calibration_solve import check_end_point, check_trajectory
from test_gpu_camera_covariance import compare as compare_covariance

pytestmark = pytest.mark.gpu

BLOCKS = ("r", "J_state", "J_landmark", "J_extrinsics", "J_intrinsics", "J_distortion", "cost")
PAIRS = {"equi_equi": (EQUI, EQUI), "radtan_equi": (RADTAN, EQUI)}


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


def check_linearization(w, hip, oracle, name):
    with ha.Problem(w, lib=hip) as g, cmr.RefereeProblem(w, oracle) as c:
        assert np.array_equal(g.camera_models(), cmr.models_of(w))
        for robustify in (False, True):
            a, b = g.linearize(ha.HS_PIXEL, robustify, sensor_blocks=True), c.linearize(ha.HS_PIXEL, robustify, sensor_blocks=True)
            errs = {key: rel(a[key], b[key]) for key in BLOCKS}
            print(name, robustify, " ".join("%s %.3g" % kv for kv in errs.items()))
            assert all(np.isfinite(a[key]).all() for key in BLOCKS)
            assert np.array_equal(a["first_cp"], b["first_cp"])
            for key, e in errs.items():
                assert e <= 1e-10, (name, robustify, key, e)
        assert abs(g.cost() - c.cost()) <= 1e-11 * c.cost()


@pytest.mark.parametrize("order", [4, 5, 6])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_linearization_against_referee(order, pair, hip, oracle):
    w = cw.window(PAIRS[pair], order=order, n_cp=16, n_landmarks=40, obs_pairs=3, seed=7 + order)
    check_linearization(w, hip, oracle, f"k{order} {pair}")


def test_fifth_camera_is_read_from_the_table(hip, oracle, build_path):
    """Five cameras, the fifth equidistant: the fused build stages four cameras in LDS and reads a later one from the table in HBM."""
    w = cw.five_cameras(cw.window((EQUI, RADTAN), order=4, n_cp=16, n_landmarks=40, obs_pairs=3))
    assert list(w.cam_models) == [RADTAN] * 4 + [EQUI] and (w.pixel_camera == 4).sum() == 120
    check_linearization(w, hip, oracle, "five cameras")
    with cmr.driving():
        S_ref, g_ref = calibration_referee.reduced_system(w, oracle, 1e4)
    with ha.Problem(w, lib=hip) as g:
        S, gr = g.reduced_system(1e4)
        s = g.solve(2)  # (the update and cost kernels read the fifth camera too)
    assert rel(S, S_ref) < 1e-9 and rel(gr, g_ref) < 1e-9
    with cmr.driving():
        sr, _ = sref.solve(w, oracle, 2)
    assert abs(s["final_cost"] - sr["final_cost"]) <= 1e-6 * sr["final_cost"]


@pytest.mark.parametrize("order", [4, 6])
def test_landmark_on_the_optical_axis(order, hip, oracle, build_path):
    w = cw.axis_window(order)
    with cmr.RefereeProblem(w, oracle) as c:
        n = c._plane.linearize(ha.HS_PIXEL, robustify=False)["r"]
    assert (np.hypot(n[:, 0], n[:, 1]) == 0.0).sum() >= 4
    check_linearization(w, hip, oracle, f"axis k{order}")
    wf = copy.copy(w)
    wf.cam_constant = np.array([[1, 0, 0], [1, 0, 0]], np.uint8)
    with cmr.driving():
        S_ref, g_ref = calibration_referee.reduced_system(wf, oracle, 1e4)
    with ha.Problem(wf, lib=hip) as g:
        S, gr = g.reduced_system(1e4)
    assert np.isfinite(S).all() and rel(S, S_ref) < 1e-9 and rel(gr, g_ref) < 1e-9


@pytest.mark.parametrize("pair", list(PAIRS))
def test_cost_function_evaluate(pair, hip, oracle):
    w = cw.five_cameras(cw.window(PAIRS[pair][::-1], order=4, n_cp=16, n_landmarks=20, obs_pairs=2))
    with ha.Problem(w, lib=hip) as g, cmr.RefereeProblem(w, oracle) as c:
        L = c.linearize(ha.HS_PIXEL, False, sensor_blocks=True)
        rows = [0, 1, 2, 3] + [int(np.flatnonzero(w.pixel_camera == 4)[5])]
        for idx in rows:
            lay = g.residual_layout(ha.HS_PIXEL, idx)
            res, jac = g.cost_function_evaluate(ha.HS_PIXEL, idx, g.parameter_blocks(ha.HS_PIXEL, idx), want=[True] * lay["num_blocks"])
            k = w.order
            assert rel(res, L["r"][idx]) <= 1e-10
            # Euclidean blocks: ambient = local (intrinsics, distortion, landmark at static_sensor_idx + 1, + 2, + 3)
            assert rel(jac[k + 1], L["J_intrinsics"][idx]) <= 1e-10 and rel(jac[k + 2], L["J_distortion"][idx]) <= 1e-10
            assert rel(jac[k + 3], L["J_landmark"][idx]) <= 1e-10


@pytest.mark.parametrize("free", ["constant", "free"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_reduced_system_against_referee(pair, free, hip, oracle, build_path):
    w = cw.window(PAIRS[pair], order=4, n_cp=16, n_landmarks=40, obs_pairs=3, with_priors=8)
    if free == "free":
        w.cam_constant = ccr.flags(w, cam0="id", cam1="id")
    with cmr.driving():
        reference = calibration_referee.reduced_system(w, oracle, 1e4)
    calibration_windows.check_build(w, hip, reference)


def admitted(w, oracle, iterations):
    """The referee's solve of w, and the admission rules asserted on it."""
    with cmr.driving():
        sr, wf = sref.solve(w, oracle, iterations)
    steps = sr["iterations"][1:]
    assert sum(it["step_is_successful"] for it in steps) >= 2
    assert not [it for it in steps if it["step_is_valid"] and abs(it["relative_decrease"] - 1e-3) <= 1e-3]
    return sr, wf


@pytest.mark.parametrize("pair", list(PAIRS))
def test_solve_against_referee(pair, hip, oracle, build_path):
    w = cw.window(PAIRS[pair], order=4, n_cp=16, n_landmarks=40, obs_pairs=3, seed=7, with_priors=16)
    sr, wf = admitted(w, oracle, 5)
    with ha.Problem(w, lib=hip) as g:
        sg = g.solve(5)
        check_trajectory(sg, sr, pair)
        assert rel(g.control_points(), wf.control_points) < 1e-6 and rel(g.landmarks(), wf.landmarks) < 1e-6
        assert sg["final_cost"] < 0.2 * sg["initial_cost"]


def test_estimation_with_free_distortion(hip, oracle, build_path):
    w = cw.window((RADTAN, EQUI), order=4, n_cp=16, n_landmarks=40, obs_pairs=3, seed=7, with_priors=16)
    w.cam_constant = ccr.flags(w, cam1="d")
    sr, wf = admitted(w, oracle, 5)
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_estimation(True)
        sg = g.solve(5)
        check_trajectory(sg, sr, "estimation")
        check_end_point(g, wf, "estimation")  # (hs_get_cameras: T_bs, intrinsics and distortion at 1e-6 relative)
        T, I, D = g.cameras()
        assert not np.array_equal(D[1], w.cam_distortion[1]) and np.array_equal(D[0], w.cam_distortion[0])
        # the tags survived the accepted steps: the device's cost at its own end point is the referee's under the same models
        assert np.array_equal(g.camera_models(), [RADTAN, EQUI])
        end = copy.copy(w)
        end.control_points, end.landmarks, end.cam_T_bs, end.cam_intrinsics, end.cam_distortion = g.control_points(), g.landmarks(), T, I, D
        with cmr.RefereeProblem(end, oracle) as c:
            assert abs(g.cost() - c.cost()) <= 1e-9 * c.cost()


def test_camera_covariance_against_referee(hip, oracle):
    w = cw.window((EQUI, EQUI), order=4, n_cp=16, n_landmarks=60, obs_pairs=3, seed=10, with_priors=16)
    w.cam_constant = ccr.flags(w, cam1="tid")
    with cmr.driving():
        R = ccr.referee(w, oracle)
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_covariance(True)
        assert g.dim_pose() == R["Sigma"].shape[0]
        g.compute_covariance()
        cov, bw = g.covariance(), g.lib.band_blocks(g.h)
    compare_covariance(w, R, cov, bw)


def test_process_tracks(hip, oracle):
    """64 stereo tracks: bearings against the numpy inverse of each camera's model, positions against the midpoint of the two rays. The
    points lie 1 .. 3 m in front of the pair and up to 2 m off its axis (plane radii up to 2.8): with the 0.11 m baseline the two rays meet at
    no less than 0.02 rad; the ray parameters divide by sin^2 of that angle, so the midpoint amplifies the rounding of the bearings (2e-16) by
    up to 2.5e3 — 5e-13, inside the 1e-12 asked (rays meeting at a smaller angle would not be: that is the triangulation, not the model)."""
    for pair in PAIRS.values():
        w = cw.window(pair, order=4, n_cp=12, n_landmarks=8, obs_pairs=2)
        rng = np.random.default_rng(64)
        stamp = 0.5 * sum(w.valid_range())
        p0 = np.c_[rng.uniform(-2, 2, (64, 2)), rng.uniform(1, 3, 64)]  # in the frame of camera 0
        p0[0, :2] = 0.0                                                   # one on the axis of camera 0
        R = [synthetic.quat_to_matrix(w.cam_T_bs[c, :4]) for c in (0, 1)]
        t = [w.cam_T_bs[c, 4:] for c in (0, 1)]
        pb = p0 @ R[0].T + t[0]
        p1 = (pb - t[1]) @ R[1]
        assert (p1[:, 2] > 0.5).all()
        px = [synthetic.project(p, np.tile(w.cam_intrinsics[c], (64, 1)), np.tile(w.cam_distortion[c], (64, 1)), pair[c]) for c, p in ((0, p0), (1, p1))]
        px[0][0] = w.cam_intrinsics[0, :2]  # exactly the principal point
        want = []
        for c in (0, 1):
            nd = (px[c] - w.cam_intrinsics[c, :2]) / w.cam_intrinsics[c, 2:]
            k = np.tile(w.cam_distortion[c], (64, 1))
            want.append(cmr.equidistant_bearing(nd, k) if pair[c] == EQUI else cmr.radtan_bearing(nd, k))
        with cmr.RefereeProblem(w, oracle) as c:
            pose = c.sample_trajectory(np.array([stamp]))[0]
        R_wb, p_wb = synthetic.quat_to_matrix(pose[:4]), pose[4:]
        o = (t[1] - t[0]) @ R[0]
        d1 = want[1] @ (R[0].T @ R[1]).T
        b0 = want[0]
        a, b, cc, e, f = (b0 * b0).sum(1), (b0 * d1).sum(1), (d1 * d1).sum(1), b0 @ o, d1 @ o
        den = a * cc - b * b
        s0, s1 = (cc * e - b * f) / den, (b * e - a * f) / den
        mid = 0.5 * (s0[:, None] * b0 + o + s1[:, None] * d1)
        pw = (mid @ R[0].T + t[0]) @ R_wb.T + p_wb
        with ha.Problem(w, lib=hip) as g:
            g0, g1, gw = g.process_tracks(stamp, px[0], px[1])
        print(pair, rel(g0, want[0]), rel(g1, want[1]), rel(gw, pw))
        assert (den > 1e-12).all()
        assert rel(g0, want[0]) <= 1e-12 and rel(g1, want[1]) <= 1e-12 and rel(gw, pw) <= 1e-12
        if pair[0] == EQUI:
            assert np.array_equal(g0[0], [0.0, 0.0, 1.0])


def sweep_cases():
    rng = np.random.default_rng(20240611)
    for case in range(20):
        order = int(rng.choice([4, 5, 6]))
        kw = dict(order=order, n_cp=int(rng.integers(order + 2, 25)), n_landmarks=int(rng.integers(10, 41)), obs_pairs=int(rng.integers(2, 5)),
                  seed=int(rng.integers(1, 1 << 20)), span=float(rng.choice([0.3, 0.6, 1.0])), with_priors=int(rng.choice([0, 8])))
        models = tuple(int(m) for m in rng.integers(0, 2, 2))
        free = rng.random(6) < 0.3
        yield case, models, kw, free


@pytest.mark.parametrize("case,models,kw,free", list(sweep_cases()), ids=["%d" % c[0] for c in sweep_cases()])
def test_sweep(case, models, kw, free, hip, oracle):
    w = cw.window(models, **kw)
    check_linearization(w, hip, oracle, f"sweep {case} {models} {kw}")
    if free.any():
        w.cam_constant = (~free).reshape(2, 3).astype(np.uint8)
    with cmr.driving():
        S_ref, g_ref = calibration_referee.reduced_system(w, oracle, 1e4)
    with ha.Problem(w, lib=hip) as g:
        S, gr = g.reduced_system(1e4)
    assert rel(S, S_ref) < 1e-9 and rel(gr, g_ref) < 1e-9, (rel(S, S_ref), rel(gr, g_ref))


# -- unchanged behaviour ------------------------------------------------------------------------------------------------------------------
def _run(g):
    S, gr = g.reduced_system(1e4)
    s = g.solve(5)
    return S, gr, s["iterations"], s["final_cost"], g.control_points(), g.landmarks()


def _same(a, b):
    assert a[2] == b[2] and a[3] == b[3]
    for x, y in ((a[0], b[0]), (a[1], b[1]), (a[4], b[4]), (a[5], b[5])):
        assert np.array_equal(x, y)


def test_default_tags_are_bit_identical_to_no_call(hip, monkeypatch, build_path):
    w = synthetic.small_visual(order=4, n_cp=18, n_landmarks=50, obs_pairs=3, with_priors=8)
    called = []
    real = ha.Problem.set_camera_models
    monkeypatch.setattr(ha.Problem, "set_camera_models", lambda self, m: called.append(m))
    with ha.Problem(w, lib=hip) as g:  # a handle that never calls the entry point
        assert called == [None]
        never = _run(g)
    monkeypatch.setattr(ha.Problem, "set_camera_models", real)
    with ha.Problem(w, lib=hip) as g:  # NULL
        _same(_run(g), never)
    wz = copy.copy(w)
    wz.cam_models = np.zeros(2, np.int32)
    with ha.Problem(wz, lib=hip) as g:  # all zeros
        _same(_run(g), never)
    with ha.Problem(w, lib=hip) as g:  # set, then back to the default
        g.set_camera_models([EQUI, EQUI])
        g.set_camera_models(None)
        _same(_run(g), never)


def test_tag_on_a_camera_seen_through_bearings_changes_nothing(hip):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, bearing=True, seed=9)
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(12, np.uint8)]
    wt = copy.copy(w)
    wt.cam_models = np.array([EQUI, EQUI], np.int32)
    with ha.Problem(w, lib=hip) as a, ha.Problem(wt, lib=hip) as b:
        assert list(b.camera_models()) == [EQUI, EQUI]
        _same(_run(a), _run(b))


def test_tags_survive(hip, oracle):
    w = cw.window((RADTAN, EQUI), order=4, n_cp=16, n_landmarks=40, obs_pairs=3, with_priors=8)
    with ha.Problem(w, lib=hip) as g, cmr.RefereeProblem(w, oracle) as c:
        c0 = c.cost()
        assert abs(g.cost() - c0) <= 1e-11 * c0
        # hs_set_cameras with the same count
        w2 = copy.copy(w)
        w2.cam_intrinsics = w.cam_intrinsics + [[0.5, -0.5, 1.0, -1.0], [0.0, 0.0, 0.0, 0.0]]
        T, I, D = (np.ascontiguousarray(x, dtype=float) for x in (w2.cam_T_bs, w2.cam_intrinsics, w2.cam_distortion))
        assert g.lib.set_cameras(g.h, 2, ha.problem._d(T), ha.problem._d(I), ha.problem._d(D)) == 0
        assert list(g.camera_models()) == [RADTAN, EQUI]
        with cmr.RefereeProblem(w2, oracle) as c2:
            assert abs(g.cost() - c2.cost()) <= 1e-11 * c2.cost() and abs(c2.cost() - c0) > 1e-3 * c0
        assert g.lib.set_cameras(g.h, 2, ha.problem._d(T), ha.problem._d(np.ascontiguousarray(w.cam_intrinsics)), ha.problem._d(D)) == 0
        # snapshot / solve / restore
        g.snapshot()
        first = g.solve(3)
        g.restore()
        assert list(g.camera_models()) == [RADTAN, EQUI] and abs(g.cost() - c0) <= 1e-11 * c0
        again = g.solve(3)
        assert again["iterations"] == first["iterations"]
    with ha.Problem(w, lib=hip) as g:
        # the delta interface: a landmark and two rows appended, a landmark retired, staged
        new = g.append_landmarks(w.landmarks[:1] + 0.01)
        g.append_residuals(ha.HS_PIXEL, w.pixel_stamps[:2], w.pixels[:2], landmark=np.full(2, new, np.int32), camera=w.pixel_camera[:2])
        g.stage()
        assert list(g.camera_models()) == [RADTAN, EQUI]
        w3 = copy.copy(w)
        w3.landmarks = np.concatenate([w.landmarks, w.landmarks[:1] + 0.01])
        w3.pixel_stamps, w3.pixels = np.r_[w.pixel_stamps, w.pixel_stamps[:2]], np.concatenate([w.pixels, w.pixels[:2]])
        w3.pixel_landmark = np.r_[w.pixel_landmark, np.full(2, new)].astype(np.int32)
        w3.pixel_camera = np.r_[w.pixel_camera, w.pixel_camera[:2]].astype(np.int32)
        with cmr.RefereeProblem(w3, oracle) as c3:
            assert abs(g.cost() - c3.cost()) <= 1e-11 * c3.cost()
        g.retire_landmarks([3])
        g.stage()
        keep = w3.pixel_landmark != 3
        w4 = copy.copy(w3)
        w4.pixel_stamps, w4.pixels, w4.pixel_camera = w3.pixel_stamps[keep], w3.pixels[keep], w3.pixel_camera[keep]
        w4.pixel_landmark = w3.pixel_landmark[keep]
        with cmr.RefereeProblem(w4, oracle) as c4:
            assert abs(g.cost() - c4.cost()) <= 1e-11 * c4.cost()
        assert list(g.camera_models()) == [RADTAN, EQUI]
        # a camera table of another size starts from the default
        T3 = np.ascontiguousarray(np.concatenate([w.cam_T_bs, w.cam_T_bs[:1]]))
        I3, D3 = np.ascontiguousarray(np.concatenate([w.cam_intrinsics, w.cam_intrinsics[:1]])), np.ascontiguousarray(np.concatenate([w.cam_distortion, w.cam_distortion[:1]]))
        assert g.lib.set_cameras(g.h, 3, ha.problem._d(T3), ha.problem._d(I3), ha.problem._d(D3)) == 0
        m = np.ones(3, np.int32)
        assert g.lib.get_camera_models(g.h, ha.problem._i(m)) == 0 and list(m) == [RADTAN] * 3


def test_restore_brings_back_values_not_models(hip, oracle):
    """A model set after the snapshot stands after hs_restore, next to the snapshot's camera values (the estimate of the solve in between is gone)."""
    w = cw.window((RADTAN, EQUI), order=4, n_cp=16, n_landmarks=40, obs_pairs=3, seed=7, with_priors=16)
    w.cam_constant = ccr.flags(w, cam1="d")
    wn = copy.copy(w)
    wn.cam_models, wn.cam_constant = np.array([EQUI, EQUI], np.int32), None
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_estimation(True)
        g.snapshot()
        g.solve(3)
        g.set_camera_models([EQUI, EQUI])
        g.cost()
        g.restore()
        assert list(g.camera_models()) == [EQUI, EQUI]
        T, I, D = g.cameras()
        assert np.array_equal(T, w.cam_T_bs) and np.array_equal(I, w.cam_intrinsics) and np.array_equal(D, w.cam_distortion)
        with cmr.RefereeProblem(wn, oracle) as c, cmr.RefereeProblem(w, oracle) as c_old:
            assert abs(c.cost() - c_old.cost()) > 1e-3 * c_old.cost()  # (the snapshot's tags would be seen)
            assert abs(g.cost() - c.cost()) <= 1e-11 * c.cost()


def test_refusals(hip):
    w = cw.window((EQUI, EQUI), order=4, n_cp=12, n_landmarks=10, obs_pairs=2)
    with ha.Problem(w, lib=hip) as g:
        with pytest.raises(ha.HsError, match=r"\(1\).*hs_set_camera_models: n must equal the camera count"):
            g.set_camera_models([EQUI, EQUI, EQUI])
        with pytest.raises(ha.HsError, match=r"\(1\).*hs_set_camera_models: unknown distortion model 2 \(camera 1\)"):
            g.set_camera_models([EQUI, 2])
        with pytest.raises(ha.HsError, match=r"unknown distortion model -1"):
            g.set_camera_models([-1, RADTAN])
        assert list(g.camera_models()) == [EQUI, EQUI]  # a refused call changes nothing
