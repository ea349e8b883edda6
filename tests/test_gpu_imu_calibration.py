"""Free IMU blocks in the reduced system on the GPU (hs_set_imu_constancy / hs_reduced_system) against the numpy referee of
tests/imu_calibration_referee.py, which tests/test_imu_calibration_referee.py pins to the oracle and to finite differences of its cost.

Only the BUILD of the system is checked: hs_reduced_system runs no factorisation, and hs_solve / hs_compute_covariance refuse a free IMU
block in this version. Bar: 1e-9 relative, the project's bar for the reduced system — for the whole matrix, for the IMU columns against
their own max-norm, and for g likewise."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

import imu_calibration_referee as ref

pytestmark = pytest.mark.gpu

BLOCKS = "tgasx"  # [T_bs, i_g, i_a, S_g, X_a]
ALL = "tgasx"


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def imu_flags(free):
    """Constancy flags with the named blocks free, e.g. "gx" = i_g and X_a."""
    c = np.ones(5, np.uint8)
    for b in free:
        c[BLOCKS.index(b)] = 0
    return c


def cam_flags(w, **free):
    c = np.ones((len(w.cam_T_bs), 3), np.uint8)
    for name, blocks in free.items():
        for b in blocks:
            c[int(name[3:]), "tid".index(b)] = 0
    return c


def imu_window(n_cp, n_landmarks, n_inertial, order, seed):
    """The IMU-border shapes of tests/test_gpu_calibration.py, rebuilt here: replay-shaped (40 control points, ~44 bias / gravity unknowns) or
    configs[2]-shaped (128 control points, order 6, ~110), fewer landmarks than configs[2] so that the dense referee stays small."""
    w = synthetic.small_inertial(order=order, n_cp=n_cp, n_landmarks=n_landmarks, obs_pairs=3, n_inertial=n_inertial, seed=seed)
    w.cp_constant = np.r_[np.ones(order, np.uint8), np.zeros(n_cp - order, np.uint8)]
    return w


def middle_third(w):
    lo, hi = w.valid_range()
    keep = (w.inertial_stamps >= lo + (hi - lo) / 3) & (w.inertial_stamps < lo + 2 * (hi - lo) / 3)
    w.inertial_stamps, w.inertial_measurements = w.inertial_stamps[keep], w.inertial_measurements[keep]
    return w


def cases():
    """name -> (window, Jacobian mode or None)."""
    for mode, tag in ((ha.HS_INERTIAL_AS_REFERENCE, "as_reference"), (ha.HS_INERTIAL_EXACT, "exact")):
        w = synthetic.small_inertial(order=4, n_cp=16)
        w.imu_constant = imu_flags(ALL)
        yield f"k4_all_free_{tag}", w, mode
    for free, tag in (("t", "T_bs"), ("gx", "i_g_X_a"), ("s", "S_g")):
        w = synthetic.small_inertial(order=5, n_cp=18, seed=11)
        w.imu_constant = imu_flags(free)
        yield f"k5_{tag}", w, None
        w = synthetic.small_inertial(order=6, n_cp=18, seed=5)
        w.imu_constant = imu_flags(free)
        yield f"k6_{tag}", w, None
    for tag in ("constant_bias", "constant_gravity"):
        w = synthetic.small_inertial(order=4, n_cp=16, seed=9)
        w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(12, np.uint8)]
        if tag == "constant_bias":
            w.imu = dict(w.imu, bias_constant=True)
        else:
            w.gravity_constant = True
        w.imu_constant = imu_flags(ALL)
        yield f"frozen_prefix_{tag}", w, None
    w = middle_third(synthetic.small_inertial(order=4, n_cp=24, n_inertial=240, seed=6))
    w.imu_constant = imu_flags(ALL)
    yield "middle_third", w, None
    w = synthetic.small_inertial(order=4, n_cp=16, seed=4)
    w.imu_constant = imu_flags(ALL)
    w.cam_constant = cam_flags(w, cam0="t", cam1="tid")
    yield "free_cameras_as_well", w, None
    w = synthetic.small_inertial(order=4, n_cp=16, n_inertial=257, seed=2)
    w.imu_constant = imu_flags(ALL)
    yield "257_inertial_rows", w, None
    w = imu_window(40, 150, 400, 4, 3)
    w.imu_constant = imu_flags(ALL)
    yield "replay_shaped", w, None
    w = imu_window(128, 300, 2000, 6, 4)
    w.imu_constant = imu_flags(ALL)
    yield "configs2_shaped", w, None


CASES = {name: (w, mode) for name, w, mode in cases()}
_referee = {}


def referee(name, oracle):
    """(S, g, P0, ni, nc) of a case, computed once and shared (read-only)."""
    if name not in _referee:
        w, mode = CASES[name]
        S, g = ref.reduced_system(w, oracle, 1e4, mode)
        S.setflags(write=False), g.setflags(write=False)
        _referee[name] = (S, g) + ref.layout(w, oracle)
    return _referee[name]


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


@pytest.mark.parametrize("name", list(CASES))
def test_reduced_system_against_referee(name, hip, oracle, build_path):
    w, mode = CASES[name]
    S_ref, g_ref, P0, ni, nc = referee(name, oracle)
    assert ni > 0
    with ha.Problem(w, lib=hip) as g:
        if mode is not None:
            g.set_inertial_jacobian(mode)
        assert g.dim_pose() == S_ref.shape[0] == P0 + ni + nc
        S, gr = g.reduced_system(1e4)
        S2, gr2 = g.reduced_system(1e4)
    imu = slice(P0, P0 + ni)
    print(name, build_path, "S", rel(S, S_ref), "g", rel(gr, g_ref), "S[:, imu]", rel(S[:, imu], S_ref[:, imu]), "g[imu]", rel(gr[imu], g_ref[imu]))
    assert rel(S, S_ref) < 1e-9, rel(S, S_ref)
    assert rel(gr, g_ref) < 1e-9, rel(gr, g_ref)
    assert rel(S[:, imu], S_ref[:, imu]) < 1e-9, rel(S[:, imu], S_ref[:, imu])
    assert rel(gr[imu], g_ref[imu]) < 1e-9, rel(gr[imu], g_ref[imu])
    assert np.array_equal(S, S.T)
    assert np.array_equal(S, S2) and np.array_equal(gr, gr2)  # (owner-computes, fixed order: bit-identical)
    n_cp = w.n_cp
    if name == "frozen_prefix_constant_bias":
        assert np.all(S[6 * n_cp:P0 - 2, imu] == 0.0) and np.all(S[imu, 6 * n_cp:P0 - 2] == 0.0)
        assert np.abs(S[P0 - 2:P0, imu]).max() > 0.0
    if name == "frozen_prefix_constant_gravity":
        assert np.all(S[P0 - 2:P0, imu] == 0.0) and np.all(S[imu, P0 - 2:P0] == 0.0)
        assert np.abs(S[6 * n_cp:P0 - 2, imu]).max() > 0.0
    if name.startswith("frozen_prefix"):
        assert np.all(S[:6 * 4, imu] == 0.0)  # constant control points: no entry
    if name == "middle_third":
        w0 = copy.copy(w)
        w0.imu_constant = None
        with ha.Problem(w0, lib=oracle) as c:
            first = c.linearize(ha.HS_INERTIAL, True)["first_cp"]
        reached = np.zeros(n_cp, bool)
        for f in first:
            reached[f:f + w.order] = True
        assert 0 < reached.sum() < n_cp
        for i in np.nonzero(~reached)[0]:
            assert np.all(S[6 * i:6 * i + 6, imu] == 0.0), i
        assert all(np.abs(S[6 * i:6 * i + 6, imu]).max() > 0.0 for i in np.nonzero(reached)[0])
    if name == "free_cameras_as_well":
        cam = slice(P0 + ni, P0 + ni + nc)
        assert nc == 20
        assert np.all(S[imu, cam] == 0.0) and np.all(S[cam, imu] == 0.0)
        assert rel(S[:, cam], S_ref[:, cam]) < 1e-9, rel(S[:, cam], S_ref[:, cam])
        assert rel(gr[cam], g_ref[cam]) < 1e-9, rel(gr[cam], g_ref[cam])
    if name == "257_inertial_rows":
        assert len(w.inertial_stamps) == 257
    if name == "configs2_shaped":
        # prepare() splits the accumulation of H_pb over min(16, 2048 / n_cp) workgroups per control point: more than one here
        assert len(w.inertial_stamps) == 2000 and min(16, 2048 // n_cp) > 1
        assert P0 - 6 * n_cp >= 100


class WithoutImuEntry:
    """The library as a handle sees it that never calls hs_set_imu_constancy (Problem.upload skips an entry point the library lacks)."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name == "set_imu_constancy":
            raise AttributeError(name)
        return getattr(self._lib, name)


def regression_windows():
    yield "visual", synthetic.small_visual(order=4, n_cp=18, n_landmarks=50, obs_pairs=3)
    yield "inertial", synthetic.small_inertial(order=4, n_cp=16)
    yield "configs1_shaped", synthetic.small_visual(order=4, n_cp=60, n_landmarks=150, obs_pairs=3, seed=13, span=0.5)


@pytest.mark.parametrize("name,w", list(regression_windows()), ids=[n for n, _ in regression_windows()])
@pytest.mark.parametrize("flags", ["null", "all_set"])
def test_constant_flags_are_bit_identical_to_a_handle_without_the_call(name, w, flags, hip):
    wc = copy.copy(w)
    wc.imu_constant = None if flags == "null" else np.ones(5, np.uint8)
    with ha.Problem(w, lib=WithoutImuEntry(hip)) as a, ha.Problem(wc, lib=hip) as b:
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


def test_a_free_flag_without_inertial_rows_changes_nothing(hip):
    v = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    e = synthetic.small_inertial(order=4, n_cp=16)  # an IMU with its bias splines, but no inertial row
    e.inertial_stamps, e.inertial_measurements = np.zeros(0), np.zeros((0, 6))
    for w in (v, e):
        wf = copy.copy(w)
        wf.imu_constant = imu_flags(ALL)
        with ha.Problem(w, lib=hip) as a, ha.Problem(wf, lib=hip) as b:
            assert a.dim_pose() == b.dim_pose()
            Sa, ga = a.reduced_system(1e4)
            Sb, gb = b.reduced_system(1e4)
            assert np.array_equal(Sa, Sb) and np.array_equal(ga, gb)
            sa, sb = a.solve(3), b.solve(3)  # (nothing is free: the solver runs)
            assert sa["final_cost"] == sb["final_cost"]


def test_flags_belong_to_the_handle(hip):
    w = synthetic.small_inertial(order=4, n_cp=16)
    with ha.Problem(w, lib=hip) as g:
        P0 = g.dim_pose()
        g.set_imu_constancy(imu_flags("t"))
        assert g.dim_pose() == P0 + 6
        g.set_imu_constancy(imu_flags("gsx"))
        assert g.dim_pose() == P0 + 24
        # a later hs_set_imu keeps them
        m = w.imu
        a = [np.ascontiguousarray(np.asarray(m[k], float)) for k in ("T_bs", "i_g", "i_a", "S_g", "X_a")]
        bg, ba = (np.ascontiguousarray(np.asarray(m[k], float).reshape(-1, 4)) for k in ("bias_g", "bias_a"))
        d = ha.problem._d
        assert g.lib.set_imu(g.h, *[d(x) for x in a], int(m["bias_order"]), float(m["bias_t0"]), float(m["bias_dt"]), bg.shape[0], d(bg), d(ba), 0) == 0
        assert g.dim_pose() == P0 + 24
        g.set_imu_constancy(np.ones(5, np.uint8))
        assert g.dim_pose() == P0
        g.set_imu_constancy(imu_flags(ALL))
        assert g.dim_pose() == P0 + 36
        g.set_imu_constancy(None)
        assert g.dim_pose() == P0


def test_delta_interface_equals_the_whole_table_handle(hip):
    """The number of IMU columns is decided when the tables are prepared: rows appended to an empty inertial table bring the columns in, and
    appending / retiring gives the system of the handle that was handed the same table in one piece (same row order: bit-identical)."""
    w = synthetic.small_inertial(order=4, n_cp=16, n_inertial=120, seed=8)
    w.imu_constant = imu_flags(ALL)
    st, me = w.inertial_stamps, w.inertial_measurements
    start = copy.copy(w)
    start.inertial_stamps, start.inertial_measurements = np.zeros(0), np.zeros((0, 6))
    cut = float(np.sort(st)[20])
    keep = st >= cut
    whole = copy.copy(w)
    whole.inertial_stamps, whole.inertial_measurements = st[keep], me[keep]
    with ha.Problem(start, lib=hip) as d, ha.Problem(whole, lib=hip) as t, ha.Problem(w, lib=hip) as full:
        P0 = d.dim_pose()
        S0, _ = d.reduced_system(1e4)
        assert S0.shape[0] == P0
        d.append_residuals(ha.HS_INERTIAL, st[:70], me[:70])
        d.stage()
        assert d.dim_pose() == P0 + 36
        d.append_residuals(ha.HS_INERTIAL, st[70:], me[70:])
        Sf, gf = d.reduced_system(1e4)
        Sw, gw = full.reduced_system(1e4)
        assert np.array_equal(Sf, Sw) and np.array_equal(gf, gw)
        d.retire_residuals_before(ha.HS_INERTIAL, cut)
        assert d.num_residuals(ha.HS_INERTIAL) == 100
        Sd, gd = d.reduced_system(1e4)
        St, gt = t.reduced_system(1e4)
        assert np.array_equal(Sd, St) and np.array_equal(gd, gt)
        d.retire_residuals_before(ha.HS_INERTIAL, float(st.max()) + 1.0)  # the last inertial row leaves: so do the IMU columns
        assert d.dim_pose() == P0
        S1, g1 = d.reduced_system(1e4)
        assert np.array_equal(S1, S0)


def test_refusals(hip):
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.imu_constant = imu_flags("t")
    for cameras in (False, True):
        wc = copy.copy(w)
        if cameras:
            wc.cam_constant = cam_flags(w, cam1="t")
        with ha.Problem(wc, lib=hip) as g:
            if cameras:  # the camera switches do not open the door
                g.set_camera_estimation(True), g.set_camera_covariance(True)
            with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_solve.*hs_set_imu_constancy"):
                g.solve(5)
            with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_compute_covariance.*hs_set_imu_constancy"):
                g.compute_covariance()
            S, _ = g.reduced_system(1e4)  # (the build is what this version offers)
            assert S.shape[0] == g.dim_pose()
            # a weight matrix is refused as before
            g.set_weights(ha.HS_INERTIAL, np.eye(6))
            with pytest.raises(ha.problem.HsError, match=r"\(1\).*weight"):
                g.reduced_system(1e4)
            g.set_weights(ha.HS_INERTIAL, None)
            # sharded handles
            assert g.lib.set_shard(g.h, 0, 2, 0) == 0
            with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_set_imu_constancy.*sharded"):
                g.solve(5)
            if not cameras:
                with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_set_imu_constancy.*sharded"):
                    g.reduced_system(1e4)
            assert g.lib.set_shard(g.h, 0, 1, 0) == 0
            g.set_imu_constancy(None)
            if not cameras:
                g.solve(2)  # (the default again: the solver runs)


def test_estimation_limits_do_not_count_the_imu_columns(hip, oracle):
    """The 137-unknown limit of the bordered solve (checked when hs_set_camera_estimation is on) counts what the solver estimates: bias /
    gravity and camera columns. IMU columns are built only: a window with 128 + 6 <= 137 of the former and 36 IMU columns on top still builds."""
    w, rng = synthetic._visual_window(synthetic.SEED ^ 0x2f1, 4, 20, 30, 3)
    w = synthetic.add_imu(w, rng, 300, bias_dt=0.1)
    w.imu_constant = imu_flags(ALL)
    w.cam_constant = cam_flags(w, cam0="t")
    S_ref, g_ref = ref.reduced_system(w, oracle, 1e4)
    P0, ni, nc = ref.layout(w, oracle)
    nbi = P0 - 6 * w.n_cp
    assert (ni, nc) == (36, 6) and nbi + nc <= 137 < nbi + ni + nc, (nbi, ni, nc)
    with ha.Problem(w, lib=hip) as g:
        g.set_camera_estimation(True)
        assert g.dim_pose() == P0 + ni + nc
        S, gr = g.reduced_system(1e4)
        assert rel(S, S_ref) < 1e-9, rel(S, S_ref)
        assert rel(gr, g_ref) < 1e-9, rel(gr, g_ref)
        with pytest.raises(ha.problem.HsError, match=r"\(3\).*hs_solve.*hs_set_imu_constancy"):
            g.solve(2)
        # without the IMU columns the same border is inside the limit and the solver takes it; one more camera block is over it, as before
        g.set_imu_constancy(None)
        g.solve(2)
        g.set_camera_constancy(cam_flags(w, cam0="tid"))
        with pytest.raises(ha.problem.HsError, match=r"\(1\).*128 bias / gravity \+ 14 free camera coordinates = 142, at most 137"):
            g.reduced_system(1e4)
