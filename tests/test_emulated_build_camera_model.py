"""CPU tests (no GPU): the fused build of the visual factors (k_build_visual -> k_assemble -> k_finalize_reduced, compiled from the product's
kernel sources for the host by tests/emul/build_harness.cpp, unchanged) on windows with equidistant cameras, against the reduced system of
the camera-model referee (tests/camera_model_referee.py driving tests/calibration_referee.py) at 1e-9, the bar of tests/test_emulated_build.py.
The harness reads 16 doubles per camera; the distortion model travels in slot 15, as in the library (hs_set_camera_models).
Shape: 16 control points, 40 landmarks, 3 observation pairs — 240 rows in two chunks (more under the forced small geometry)."""
from unittest import mock

import numpy as np
import pytest

import calibration_referee
import camera_model_referee as cmr
import camera_model_windows as cw
import test_emulated_build as teb
from test_emulated_build import harness  # noqa: F401  (the session fixture that compiles the harness)


def _pack_cameras_with_models(w):
    cam = np.zeros((len(w.cam_T_bs), 16))
    cam[:, :7], cam[:, 7:11], cam[:, 11:15], cam[:, 15] = w.cam_T_bs, w.cam_intrinsics, w.cam_distortion, cmr.models_of(w)
    return cam


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("order,models,R,L", [(4, (cw.EQUI, cw.EQUI), 0, 0), (6, (cw.EQUI, cw.EQUI), 0, 0), (4, (cw.RADTAN, cw.EQUI), 0, 0),
                                               (6, (cw.RADTAN, cw.EQUI), 0, 0), (4, (cw.EQUI, cw.EQUI), 64, 3)])
def test_emulated_fused_build_matches_the_referee(harness, oracle, order, models, R, L):  # noqa: F811
    w = cw.window(models, order=order, n_cp=16, n_landmarks=40, obs_pairs=3)
    assert len(w.pixel_stamps) == 240
    with mock.patch.object(teb, "_pack_cameras", _pack_cameras_with_models):
        out = teb.run_emulated_build(harness, w, 1e4, R=R, L=L)
    assert out["n_chunk"] >= 2 and (R == 0 or out["R"] == 64)
    with cmr.driving():
        S, g = calibration_referee.reduced_system(w, oracle, 1e4)
        with cmr.RefereeProblem(w, oracle) as p:
            cost = p.cost()
    n = out["S"].shape[0]
    assert S.shape[0] == n
    print(order, models, R, "S %.3g g %.3g cost %.3g" % (rel(out["S"], S), np.abs(out["g"] - g).max() / max(1.0, np.abs(g).max()), abs(out["cost"] - cost) / cost))
    assert np.abs(out["S"] - S).max() <= 1e-9 * np.abs(S).max()
    assert np.abs(out["g"] - g).max() <= 1e-9 * max(1.0, np.abs(g).max())
    assert abs(out["cost"] - cost) <= 1e-11 * cost
    # k_update_visual against k_backsub_retract + k_cost_visual on the same (fabricated) step: both read the model too
    u = out["upd"]
    assert u[0] <= 1e-13 and u[1] == 0.0, u[:2]
    for a, b in zip(u[2::2], u[3::2]):
        assert abs(a - b) <= 1e-12 * max(abs(a), 1e-300), (a, b)


def test_the_model_is_not_ignored(harness, oracle):  # noqa: F811
    """The same window packed without the tag (slot 15 zero: a radial-tangential solve of equidistant coefficients) is far from the referee."""
    w = cw.window((cw.EQUI, cw.EQUI), order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    out = teb.run_emulated_build(harness, w, 1e4)
    with cmr.RefereeProblem(w, oracle) as p:
        cost = p.cost()
    assert abs(out["cost"] - cost) > 0.5 * cost
