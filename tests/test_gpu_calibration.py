"""Free camera blocks in the reduced system on the GPU (hs_set_camera_constancy / hs_reduced_system / hs_get_cameras) against the
numpy referee of tests/calibration_referee.py, which tests/test_calibration_referee.py pins to the oracle.

Only the BUILD of the system is checked: hs_reduced_system runs no factorisation, and hs_solve refuses free camera blocks in this version.
The window shapes named after a factorisation (two-ended, dense small system, long band) are the shapes whose build those paths would read."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import calibration_referee as ref

pytestmark = pytest.mark.gpu

HS_ERR_INVALID, HS_ERR_STATE = 1, 3


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def flags(w, **free):
    """Constancy flags: every block constant but those named, e.g. cam1="tid" (T_bs, intrinsics, distortion of camera 1 free)."""
    c = np.ones((len(w.cam_T_bs), 3), np.uint8)
    for name, blocks in free.items():
        for b in blocks:
            c[int(name[3:]), "tid".index(b)] = 0
    return c


def windows():
    for order, seed in ((4, 7), (5, 21), (6, 8)):
        w = synthetic.small_visual(order=order, n_cp=18, n_landmarks=50, obs_pairs=3, seed=seed)
        w.cam_constant = flags(w, cam1="tid")
        yield f"pixel_cam1_free_k{order}", w
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, seed=10, with_priors=20)
    w.cam_constant = flags(w, cam0="id", cam1="id")
    yield "pixel_intrinsics_distortion_free", w
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, bearing=True, seed=9)
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(12, np.uint8)]
    w.cam_constant = flags(w, cam1="tid")  # (bearing rows: zero intrinsics / distortion columns, kept in the system)
    yield "bearing_cam1_free", w
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.cam_constant = flags(w, cam0="t")
    yield "stereo_inertial_cam0_T_bs", w
    w = synthetic.small_inertial(order=6, n_cp=18, seed=5)
    w.cam_constant = flags(w, cam0="t", cam1="tid")
    yield "stereo_inertial_k6_two_cameras", w
    w = synthetic.small_visual(order=5, n_cp=20, n_landmarks=60, obs_pairs=3, seed=31, with_priors=20)
    w.cp_constant = np.r_[np.ones(5, np.uint8), np.zeros(15, np.uint8)]
    w.landmark_constant = (np.arange(60) % 4 == 0).astype(np.uint8)
    w.cam_constant = flags(w, cam0="id", cam1="tid")
    yield "constant_landmarks_frozen_prefix", w
    w = synthetic.small_visual(order=4, n_cp=60, n_landmarks=150, obs_pairs=3, seed=13, span=0.5)
    w.cam_constant = flags(w, cam0="id", cam1="tid")
    yield "two_ended_window_build", w
    w = synthetic.small_visual(order=4, n_cp=24, n_landmarks=72, obs_pairs=3, with_priors=24)
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(20, np.uint8)]
    w.cam_constant = flags(w, cam1="tid")
    yield "dense_small_system_window_build", w
    w = synthetic.small_visual(order=4, n_cp=34, n_landmarks=80, obs_pairs=6, seed=11, span=3.2)
    w.cam_constant = flags(w, cam1="tid")
    yield "long_band_window_build", w


def imu_window(n_cp, n_landmarks, n_inertial, order, seed):
    """An IMU border next to two fully free cameras (28 camera columns): replay-shaped (40 control points, ~44 bias / gravity unknowns) or
    configs[2]-shaped (128 control points, ~110), fewer landmarks than configs[2] so that the dense referee stays small."""
    w = synthetic.small_inertial(order=order, n_cp=n_cp, n_landmarks=n_landmarks, obs_pairs=3, n_inertial=n_inertial, seed=seed)
    w.cp_constant = np.r_[np.ones(order, np.uint8), np.zeros(n_cp - order, np.uint8)]
    w.cam_constant = flags(w, cam0="tid", cam1="tid")
    return w


@pytest.mark.parametrize("shape", ["replay", "configs2"])
def test_two_free_cameras_next_to_an_imu_border(shape, hip, oracle):
    w = imu_window(40, 150, 400, 4, 3) if shape == "replay" else imu_window(128, 300, 2000, 6, 4)
    S_ref, g_ref = ref.reduced_system(w, oracle, 1e4)
    assert ref.camera_columns(w)[1] == 28
    with ha.Problem(w, lib=hip) as g:
        nbi = g.dim_pose() - 6 * w.n_cp - 28
        assert nbi >= (100 if shape == "configs2" else 40), nbi
        S, gr = g.reduced_system(1e4)
    assert rel(S, S_ref) < 1e-9, rel(S, S_ref)
    assert rel(gr, g_ref) < 1e-9, rel(gr, g_ref)
    cam = slice(S.shape[0] - 28, S.shape[0])
    assert rel(S[:, cam], S_ref[:, cam]) < 1e-9, rel(S[:, cam], S_ref[:, cam])


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


@pytest.mark.parametrize("name,w", list(windows()), ids=[n for n, _ in windows()])
def test_reduced_system_against_referee(name, w, hip, oracle, build_path):
    S_ref, g_ref = ref.reduced_system(w, oracle, 1e4)
    nc = ref.camera_columns(w)[1]
    assert nc > 0
    with ha.Problem(w, lib=hip) as g:
        assert g.dim_pose() == S_ref.shape[0]
        S, gr = g.reduced_system(1e4)
        S2, gr2 = g.reduced_system(1e4)
    assert rel(S, S_ref) < 1e-9, rel(S, S_ref)
    assert rel(gr, g_ref) < 1e-9, rel(gr, g_ref)
    P = S.shape[0]
    cam = slice(P - nc, P)
    assert rel(S[:, cam], S_ref[:, cam]) < 1e-9, rel(S[:, cam], S_ref[:, cam])
    assert rel(gr[cam], g_ref[cam]) < 1e-9, rel(gr[cam], g_ref[cam])
    assert np.array_equal(S, S.T)
    assert np.array_equal(S, S2) and np.array_equal(gr, gr2)  # (owner-computes, fixed order: bit-identical)


def regression_windows():
    yield "visual", synthetic.small_visual(order=4, n_cp=18, n_landmarks=50, obs_pairs=3)
    yield "inertial", synthetic.small_inertial(order=4, n_cp=16)
    yield "configs1_shaped", synthetic.small_visual(order=4, n_cp=60, n_landmarks=150, obs_pairs=3, seed=13, span=0.5)


@pytest.mark.parametrize("name,w", list(regression_windows()), ids=[n for n, _ in regression_windows()])
def test_all_constant_flags_are_bit_identical_to_the_default(name, w, hip):
    wc = copy.copy(w)
    wc.cam_constant = np.ones((len(w.cam_T_bs), 3), np.uint8)
    with ha.Problem(w, lib=hip) as a, ha.Problem(wc, lib=hip) as b:
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


def test_flags_round_trip_and_state(hip):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    with ha.Problem(w, lib=hip) as g:
        P0 = g.dim_pose()
        g.set_camera_constancy(flags(w, cam1="tid"))
        assert g.dim_pose() == P0 + 14
        g.set_camera_constancy(flags(w, cam0="d"))
        assert g.dim_pose() == P0 + 4
        g.set_camera_constancy(None)
        assert g.dim_pose() == P0
        T, I, D = g.cameras()
        assert np.array_equal(T, w.cam_T_bs) and np.array_equal(I, w.cam_intrinsics) and np.array_equal(D, w.cam_distortion)
        # a camera no visual row references is left out of the system
        w2 = copy.copy(w)
        w2.pixel_camera = np.zeros_like(w.pixel_camera)
        w2.cam_constant = flags(w, cam1="tid")
        g.upload(w2)
        assert g.dim_pose() == P0
        w4 = copy.copy(w)
        w4.cam_constant = flags(w, cam1="tid")
        g.upload(w4)
        assert g.dim_pose() == P0 + 14
        # re-uploading a window without flags restores the default (None: every block constant)
        g.upload(w)
        assert g.dim_pose() == P0
        # a camera table of another size resets the flags
        g.set_camera_constancy(flags(w, cam1="tid"))
        assert g.dim_pose() == P0 + 14
        T3, I3, D3 = (np.ascontiguousarray(np.concatenate([x, x[:1]])) for x in (w.cam_T_bs, w.cam_intrinsics, w.cam_distortion))
        assert g.lib.set_cameras(g.h, 3, ha.problem._d(T3), ha.problem._d(I3), ha.problem._d(D3)) == 0
        assert g.dim_pose() == P0


def test_refusals(hip):
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    w.cam_constant = flags(w, cam1="t")
    with ha.Problem(w, lib=hip) as g:
        L = g.lib
        bad = np.ones(9, np.uint8)
        assert L.set_camera_constancy(g.h, 3, ha.problem._u8(bad)) == HS_ERR_INVALID
        assert b"camera count" in L.last_error(g.h)
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*free camera blocks"):
            g.solve(5)
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*free camera blocks"):
            g.compute_covariance()
        g.set_camera_constancy(None)
        g.solve(2)  # (the default again: the solver runs)
    # more free coordinates than the border machinery takes (64): five cameras, each fully free
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    w.cam_T_bs, w.cam_intrinsics, w.cam_distortion = (np.tile(x[:1], (5, 1)) for x in (w.cam_T_bs, w.cam_intrinsics, w.cam_distortion))
    w.pixel_camera = (np.arange(len(w.pixel_camera)) % 5).astype(np.int32)
    w.cam_constant = np.zeros((5, 3), np.uint8)
    with ha.Problem(w, lib=hip) as g:
        with pytest.raises(ha.problem.HsError, match=r"\(1\).*at most 64"):
            g.reduced_system(1e4)
