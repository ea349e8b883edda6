"""The numpy restatement of the KLT front-end (tests/klt_numpy.py) against analytic ground truth: pure sub-pixel translations, a small
affine warp and a stereo pair moving over a textured plane (tests/klt_scenes.py). These are the accuracy bars the device code inherits
through its bit-identity with the restatement (tests/test_gpu_klt.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import klt_numpy as K
import klt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("t", [(0.3, 0.7), (5.25, -3.5), (14.6, 11.2), (-19.3, 6.1), (19.5, -4.25), (-2.5, -19.75)])
def test_translation_accuracy(t):
    tex = S.Texture(1)
    w, h = 320, 240
    img0, img1 = S.image(tex, w, h), S.image(tex, w, h, t=(-t[0], -t[1]))
    rng = np.random.default_rng(0)
    pts = np.stack([rng.uniform(32, w - 32, 300), rng.uniform(32, h - 32, 300)], -1).astype(np.float32)
    nxt, st = K.optical_flow(K.build_pyramid(img0, 3, 21), K.build_pyramid(img1, 3, 21), pts)
    truth = pts + np.array(t, np.float32)
    inside = (truth[:, 0] > 12) & (truth[:, 0] < w - 12) & (truth[:, 1] > 12) & (truth[:, 1] < h - 12)
    assert st[inside].mean() >= 0.95
    err = np.linalg.norm(nxt - truth, axis=1)[(st == 1) & inside]
    assert np.percentile(err, 95) <= 0.05


def test_affine_warp():
    tex = S.Texture(2)
    w, h = 320, 240
    A = np.array([[1.01, 0.015], [-0.01, 0.995]])
    img0, img1 = S.image(tex, w, h), S.image(tex, w, h, A=np.linalg.inv(A), t=(0.0, 0.0))
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(40, w - 40, 200), rng.uniform(40, h - 40, 200)], -1).astype(np.float32)
    nxt, st = K.optical_flow(K.build_pyramid(img0, 3, 21), K.build_pyramid(img1, 3, 21), pts)
    truth = pts.astype(np.float64) @ A.T
    assert st.mean() >= 0.95
    assert np.percentile(np.linalg.norm(nxt - truth, axis=1)[st == 1], 95) <= 0.2


def test_point_pushed_outside_fails():
    tex = S.Texture(3)
    w, h = 200, 160
    img0, img1 = S.image(tex, w, h), S.image(tex, w, h, t=(-15.0, 0.0))
    pts = np.array([[196.0, 80.0], [198.0, 60.0], [100.0, 80.0]], np.float32)
    pa, pb = K.build_pyramid(img0, 3, 21), K.build_pyramid(img1, 3, 21)
    _, keep = K.track_points(pa, pb, pts, K.DEFAULTS, (h, w))
    assert not keep[0] and not keep[1] and keep[2]
    # the patch entirely beyond the last column: LK itself reports failure at level 0
    _, st = K.optical_flow(pa, pb, np.array([[100.0, 80.0]], np.float32), initial=np.array([[225.0, 80.0]], np.float32))
    assert st[0] == 0


def test_corner_tie_order():
    img = S.tie_image(96, 64)
    c = K.good_features(img, 0, 0.01, 1)
    lam = K.min_eigen(img)[c[:, 1].astype(int), c[:, 0].astype(int)]
    assert (np.diff(lam) <= 0).all()
    idx = c[:, 1].astype(int) * 96 + c[:, 0].astype(int)
    same = lam[1:] == lam[:-1]
    assert same.any() and (idx[1:][same] < idx[:-1][same]).all()


def ground_truth_errors(messages):
    first, errs = {}, []
    for m in messages:
        f = int(round(m["stamp"]))
        for i, l, p in zip(m["ids"], m["lengths"], m["pixels0"]):
            if l == 0:
                first[int(i)] = (f, p.astype(np.float64))
        for i, l, p0, p1 in zip(m["ids"], m["lengths"], m["pixels0"], m["pixels1"]):
            f0, q = first[int(i)]
            P = S.StereoPlane.backproject(q[None], f0)
            errs.append(max(np.linalg.norm(S.StereoPlane.project(P, f)[0] - p0), np.linalg.norm(S.StereoPlane.project(P, f, True)[0] - p1)))
    return np.array(errs)


def test_frame_driver_on_stereo_plane():
    scene, fe, msgs = S.StereoPlane(0), K.Frontend(), []
    for k in range(7):
        m = fe.process(float(k), *scene.frame(k))
        if m is not None:
            msgs.append(m)
    assert [m["stamp"] for m in msgs] == [float(k) for k in range(6)]
    for a, b in zip(msgs, msgs[1:]):
        assert len(b["ids"]) <= 150
        prev = dict(zip(a["ids"].tolist(), a["lengths"].tolist()))
        for i, l in zip(b["ids"].tolist(), b["lengths"].tolist()):
            assert l == (prev[i] + 1 if i in prev else 0)
    assert sum(int((m["lengths"] > 0).sum()) for m in msgs[1:]) > 100 * (len(msgs) - 1)
    err = ground_truth_errors(msgs)
    assert (err < 0.1).mean() >= 0.95


def test_tracker_create_fails_without_gpu():
    """hs_tracker_create on a machine without a usable GPU is an HsError, not a crash (in a subprocess: the HIP runtime stays out of this one)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    code = ("import hyperslam_amd as ha\n"
            "try:\n    ha.Tracker(752, 480)\nexcept ha.HsError as e:\n    print('HsError', e)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "HsError" in r.stdout
