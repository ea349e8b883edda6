"""The stereo KLT front-end on the MI355X (hs_tracker_*, kernels_klt.hpp) against its numpy restatement (tests/klt_numpy.py): pyramids,
derivatives and the corner response bit for bit, the corner lists identical (ties and the slice of many candidates included), Lucas-Kanade
positions and statuses identical, and whole frames of the stereo sequence identical message for message; then the messages through
hs_process_tracks onto the textured plane."""
import numpy as np
import pytest

import hyperslam_amd as ha
import klt_numpy as K
import klt_scenes as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("w,h", [(752, 480), (751, 479)])
def test_pyramid_and_response_bit_identical(w, h):
    img = S.image(S.Texture(4), w, h, t=(3.3, 1.7))
    with ha.Tracker(w, h) as t:
        lv, dv = t.build_pyramid(img)
        ref_l, ref_d = K.build_pyramid(img, 3, 21)
        assert len(lv) == len(ref_l) == 4
        for a, b, c, d in zip(lv, ref_l, dv, ref_d):
            assert np.array_equal(a, b) and np.array_equal(c, d)
        assert np.array_equal(t.min_eigen(img).view(np.uint32), K.min_eigen(img).view(np.uint32))


def _corner_cases():
    w, h = 752, 480
    img = S.image(S.Texture(5), w, h)
    dense = S.image(S.Texture(6, min_wavelength=4.0, max_wavelength=9.0), w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    mask = ((xx - 300) ** 2 + (yy - 200) ** 2 > 90 ** 2) & (xx > 40)
    return w, h, img, dense, mask


@pytest.mark.parametrize("max_corners", [0, 1, 150, 5000])
@pytest.mark.parametrize("min_distance", [1, 10, 30])
def test_good_features_identical(max_corners, min_distance):
    w, h, img, _, mask = _corner_cases()
    with ha.Tracker(w, h) as t:
        for m in (None, mask):
            got = t.good_features(img, max_corners, 0.01, min_distance, m)
            ref = K.good_features(img, max_corners, 0.01, min_distance, m)
            assert np.array_equal(got, ref), (m is None, len(got), len(ref))


def test_good_features_ties_and_many_candidates():
    w, h, _, dense, _ = _corner_cases()
    with ha.Tracker(w, h) as t:
        tie = S.tie_image(w, h, period=6)
        for mc, md in ((0, 1), (200, 10), (5000, 3)):
            assert np.array_equal(t.good_features(tie, mc, 0.01, md), K.good_features(tie, mc, 0.01, md))
        got, ref = t.good_features(dense, 0, 0.001, 2), K.good_features(dense, 0, 0.001, 2)
        assert len(ref) > 4096 and np.array_equal(got, ref)


@pytest.mark.parametrize("patch,levels", [(21, 3), (7, 0), (15, 1), (31, 2), (21, 2), (7, 3)])
def test_optical_flow_identical(patch, levels):
    w, h = 400, 300
    tex = S.Texture(7)
    img0, img1 = S.image(tex, w, h), S.image(tex, w, h, A=np.array([[0.995, 0.01], [-0.008, 1.004]]), t=(-6.3, 4.1))
    rng = np.random.default_rng(patch + levels)
    inner = np.stack([rng.uniform(0, w, 300), rng.uniform(0, h, 300)], -1)
    border = np.array([[0, 0], [w - 1, h - 1], [-5, 100], [w + 3, 50], [100, -patch - 3], [200, h + 40], [0.5, h - 0.5], [w - 0.25, 0.75]])
    pts = np.vstack([inner, border]).astype(np.float32)
    pa, pb = K.build_pyramid(img0, levels, patch), K.build_pyramid(img1, levels, patch)
    kw = dict(patch=patch)
    init = (pts + np.array([6.0, -4.0], np.float32)).astype(np.float32)
    with ha.Tracker(w, h, patch_size=patch, num_pyramid_levels=levels) as t:
        for initial in (None, init):
            got, gs = t.optical_flow(img0, img1, pts, initial)
            ref, rs = K.optical_flow(pa, pb, pts, initial, **kw)
            assert np.array_equal(gs, rs)
            assert np.abs(got - ref).max() <= 1e-4
            assert 0 < rs.sum() < len(rs)


def _run_sequence(n_frames):
    scene = S.StereoPlane(0)
    ref, msgs, ref_msgs = K.Frontend(), [], []
    with ha.Tracker(S.WIDTH, S.HEIGHT) as t:
        for k in range(n_frames):
            L, R = scene.frame(k)
            a, b = t.process(float(k), L, R), ref.process(float(k), L, R)
            assert (a is None) == (b is None)
            if a is not None:
                msgs.append(a), ref_msgs.append(b)
    return msgs, ref_msgs


def test_process_sequence_identical():
    from test_klt_numpy import ground_truth_errors
    msgs, ref_msgs = _run_sequence(16)
    assert len(msgs) == 15
    for a, b in zip(msgs, ref_msgs):
        assert a["stamp"] == b["stamp"]
        for key in ("ids", "lengths", "pixels0", "pixels1"):
            assert np.array_equal(a[key], b[key]), key
    err = ground_truth_errors(msgs)
    assert (err < 0.1).mean() >= 0.95


def test_messages_triangulate_onto_plane():
    """pixels0 / pixels1 -> Problem.process_tracks with the true (constant-orientation) spline: points on z = PLANE_Z. At 3 m with a
    0.11 m baseline and f = 458 px, 0.1 px of disparity error is 3^2 / (458 * 0.11) * 0.1 = 0.018 m of depth: tolerance 0.05 m."""
    msgs, _ = _run_sequence(4)
    m = msgs[-1]
    k = int(m["stamp"])
    c = S.camera_position(k)
    n_cp = 8
    cps = np.zeros((n_cp, 8))
    cps[:, 3] = 1.0
    cps[:, 4:7] = c
    cps[:, 7] = k - 0.3 + 0.1 * np.arange(n_cp)
    w = ha.Window(order=4, t0=cps[0, 7], dt=0.1, control_points=cps,
                  cam_T_bs=np.array([[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, S.BASELINE, 0, 0]], float),
                  cam_intrinsics=np.array([[S.CX, S.CY, S.FX, S.FY]] * 2), cam_distortion=np.zeros((2, 4)))
    with ha.Problem(w) as p:
        _, _, xyz = p.process_tracks(float(k), m["pixels0"].astype(np.float64), m["pixels1"].astype(np.float64))
    assert len(xyz) > 100
    assert np.percentile(np.abs(xyz[:, 2] - S.PLANE_Z), 95) < 0.05


def test_invalid_arguments_and_interleaving_with_problem():
    from hyperslam_amd import _lib, synthetic
    lib = _lib.load()
    import ctypes as C
    h = C.c_void_p()
    o = _lib.TrackerOptions()
    lib.tracker_default_options(C.byref(o))
    o.patch_size = 2
    assert lib.tracker_create(0, None, 752, 480, C.byref(o), C.byref(h)) == 1
    o.patch_size = 21
    assert lib.tracker_create(0, None, 20, 480, C.byref(o), C.byref(h)) == 1
    with pytest.raises(ha.HsError):
        ha.Tracker(752, 480, num_pyramid_levels=9)
    w, h_ = 320, 240
    tex = S.Texture(8)
    img0, img1 = S.image(tex, w, h_), S.image(tex, w, h_, t=(-2.0, 1.0))
    pts = np.array([[100.0, 100.0], [200.0, 150.0]], np.float32)
    win = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, with_priors=16)
    with ha.Tracker(w, h_) as t, ha.Problem(win) as p:
        assert lib.tracker_optical_flow(t.h, None, None, 0, None, None, None, 0) == 1
        assert lib.tracker_process(t.h, 0.0, None, None, None, None, None, None, None, None, None) == 1
        a0 = t.optical_flow(img0, img1, pts)
        s0 = p.solve(3)
        a1 = t.optical_flow(img0, img1, pts)
        assert np.array_equal(a0[0], a1[0]) and np.array_equal(a0[1], a1[1])
    with ha.Problem(win) as q:
        assert q.solve(3)["final_cost"] == s0["final_cost"]
