"""TEST INFRASTRUCTURE: windows of a platform AT REST. Every generator of hyperslam_amd/synthetic.py samples one moving trajectory with 1e-2 of
tangent noise, so no relative rotation of two control points is ever small there; here the ground truth is ONE constant pose, and every pair
of control points sits in the series branches of rel_log / exp_scaled / jr_inv_coef (csrc/device_spline.hpp), as in the first seconds of a
real sequence. (A solve moves the free control points out of them again, see tests/test_degenerate_windows.py; the `held` windows do not.)

  ground truth   one pose (REST_ROTVEC, REST_POSITION); stereo pixels or bearings through the EuRoC pair with 0.5 px of noise
  control points that pose with 1e-3 m of position noise and a rotation offset Exp(amp_j axis_j) about a random axis:
                 amp = "0" | "1e-9" | "thresholds" (the cycle 0, 1e-9, 2e-8, 3e-5, 0.99e-4, 1.01e-4, 1e-3: both sides of every threshold)
  flip           the odd control points are stored with the other sign of their quaternion (the same rotations)
  priors         pose priors at the rest pose (sensor frame of synthetic.small_visual), 1e-4 of noise
  imu            the conventions of synthetic.add_imu with the measurements of a body at rest: gyroscope = bias, accelerometer = gravity in
                 the sensor frame + bias, + noise
The first K control points are constant (the gauge, optimizer.cpp:323-328).
"""
import numpy as np

from hyperslam_amd import Window, synthetic
from hyperslam_amd.synthetic import SplitMix64, compose, quat_exp, quat_mul, quat_to_matrix

REST_ROTVEC = np.array([0.3, -0.2, 0.5])
REST_POSITION = np.array([0.4, -0.3, 0.2])
THRESHOLDS = (0.0, 1e-9, 2e-8, 3e-5, 0.99e-4, 1.01e-4, 1e-3)
AMPLITUDES = {"0": (0.0,), "1e-9": (1e-9,), "thresholds": THRESHOLDS}
BIAS_G, BIAS_A = np.array([1e-3, -2e-3, 5e-4]), np.array([2e-2, 1e-2, -3e-2])


def rest_pose():
    return quat_exp(REST_ROTVEC), REST_POSITION.copy()


def at_rest(order=4, n_cp=16, n_landmarks=40, obs_pairs=3, amp="0", flip=False, bearing=False, with_priors=0, n_inertial=0, identity_imu=False,
            seed=1, span=1.0, dt=0.1, pixel_noise=0.5, lm_noise=0.05):
    rng = SplitMix64(synthetic.SEED ^ (0xA7000 + seed))
    q0, p0 = rest_pose()
    t0 = -((order - 1) // 2) * dt
    t = t0 + dt * np.arange(n_cp)
    axis = rng.normal(n_cp, 3)
    axis /= np.linalg.norm(axis, axis=1, keepdims=True)
    cycle = AMPLITUDES[amp]
    a = np.array([cycle[j % len(cycle)] for j in range(n_cp)])
    q = quat_mul(quat_exp(a[:, None] * axis), np.broadcast_to(q0, (n_cp, 4)))
    q[a == 0.0] = q0  # (exactly the rest rotation, not Exp(0) times it rounded)
    if flip:
        q[1::2] *= -1.0
    cp = np.concatenate([q, p0 + rng.normal(n_cp, 3, sigma=1e-3), t[:, None]], -1)
    T, intr, dist = synthetic.EUROC_CAM_T_BS, synthetic.EUROC_CAM_INTRINSICS, synthetic.EUROC_CAM_DISTORTION
    w = Window(order=order, t0=t0, dt=dt, control_points=cp, cam_T_bs=T.copy(), cam_intrinsics=intr.copy(), cam_distortion=dist.copy())
    w.cp_constant = np.r_[np.ones(order, np.uint8), np.zeros(n_cp - order, np.uint8)]
    lo, hi = w.valid_range()
    eps = 1e-9
    # landmarks: a pixel of camera 0 and a depth, back-projected through the rest pose
    px = np.stack([rng.uniform(n_landmarks, lo=0.0, hi=752.0), rng.uniform(n_landmarks, lo=0.0, hi=480.0)], -1)
    depth = rng.uniform(n_landmarks, lo=2.0, hi=10.0)
    cx, cy, fx, fy = intr[0]
    ps = np.stack([(px[:, 0] - cx) / fx * depth, (px[:, 1] - cy) / fy * depth, depth], -1)
    q_ws, p_ws = compose(q0, p0, T[0, :4], T[0, 4:])
    lm_gt = ps @ quat_to_matrix(q_ws).T + p_ws
    ta = rng.uniform(n_landmarks, lo=lo, hi=hi - eps)
    st = np.clip(ta[:, None] + rng.uniform(n_landmarks, obs_pairs, lo=-0.5 * span, hi=0.5 * span), lo, hi - eps)
    stf = np.repeat(st[:, :, None], 2, axis=2).reshape(-1)
    camf = np.broadcast_to(np.array([0, 1], np.int32), (n_landmarks, obs_pairs, 2)).reshape(-1).copy()
    lmf = np.broadcast_to(np.arange(n_landmarks, dtype=np.int32)[:, None, None], (n_landmarks, obs_pairs, 2)).reshape(-1).copy()
    qs, psw = compose(q0, p0, T[camf, :4], T[camf, 4:])
    p_s = np.einsum("nji,nj->ni", quat_to_matrix(qs), lm_gt[lmf] - psw)
    assert (p_s[:, 2] > 0.5).all()
    n_obs = len(stf)
    if bearing:
        b = p_s / np.linalg.norm(p_s, axis=-1, keepdims=True) + rng.normal(n_obs, 3, sigma=pixel_noise / 458.0)
        b /= np.linalg.norm(b, axis=-1, keepdims=True)
        w.bearing_stamps, w.bearings, w.bearing_landmark, w.bearing_camera = stf, b, lmf, camf
    else:
        meas = synthetic.project_radtan(p_s, intr[camf], dist[camf]) + rng.normal(n_obs, 2, sigma=pixel_noise)
        w.pixel_stamps, w.pixels, w.pixel_landmark, w.pixel_camera = stf, meas, lmf, camf
    w.landmarks = lm_gt + rng.normal(n_landmarks, 3, sigma=lm_noise)
    if with_priors:
        q_bs, p_bs = quat_exp(rng.uniform(1, 3, lo=-0.5, hi=0.5)), rng.uniform(1, 3, lo=-0.2, hi=0.2)
        w.sensor_T_bs = np.concatenate([q_bs, p_bs], -1)
        qm, pm = compose(q0, p0, q_bs[0], p_bs[0])
        qm = quat_mul(quat_exp(rng.normal(with_priors, 3, sigma=1e-4)), np.broadcast_to(qm, (with_priors, 4)))
        pm = pm + rng.normal(with_priors, 3, sigma=1e-4)
        w.prior_stamps = rng.uniform(with_priors, lo=lo, hi=hi - eps)
        w.prior_poses, w.prior_sensor = np.concatenate([qm, pm], -1), np.zeros(with_priors, np.int32)
    if n_inertial:
        add_imu_at_rest(w, rng, n_inertial, identity=identity_imu)
    return w


def add_imu_at_rest(w, rng, n_inertial, bias_dt=1.0, bias_order=4, identity=False):
    """synthetic.add_imu for a body at rest: w_b = alpha_b = 0 and a_w = 0, so every lever-arm term of the model vanishes and the prediction
    is [S_g a_b + b_g, A(i_a) R_bs^T a_b + b_a] with a_b = R_wb^T (0 - g) (inertial.cpp:200-203)."""
    lo, hi = w.valid_range()
    kb = bias_order
    n_bias = int(np.ceil((hi - lo) / bias_dt)) + kb
    bias_t0 = lo - ((kb - 1) // 2) * bias_dt - 1e-3
    stamps_b = bias_t0 + bias_dt * np.arange(n_bias)
    bg = np.concatenate([BIAS_G + rng.normal(n_bias, 3, sigma=1e-3), stamps_b[:, None]], -1)
    ba = np.concatenate([BIAS_A + rng.normal(n_bias, 3, sigma=1e-2), stamps_b[:, None]], -1)
    if identity:
        T_bs = np.array([0, 0, 0, 1, 0, 0, 0.0])
        i_g = np.array([1, 1, 1, 0, 0, 0.0])
        i_a = i_g.copy()
        S_g, X_a = np.zeros(9), np.zeros(9)
    else:
        T_bs = np.concatenate([quat_exp(rng.uniform(3, lo=-0.3, hi=0.3)), rng.uniform(3, lo=-0.1, hi=0.1)])
        i_g = np.array([1, 1, 1, 0, 0, 0.0]) + rng.uniform(6, lo=-0.05, hi=0.05)
        i_a = np.array([1, 1, 1, 0, 0, 0.0]) + rng.uniform(6, lo=-0.05, hi=0.05)
        S_g, X_a = rng.uniform(9, lo=-1e-3, hi=1e-3), rng.uniform(9, lo=-0.02, hi=0.02)
    w.imu = dict(T_bs=T_bs, i_g=i_g, i_a=i_a, S_g=S_g, X_a=X_a, bias_order=kb, bias_t0=bias_t0, bias_dt=bias_dt, bias_g=bg, bias_a=ba,
                 bias_constant=False)
    g_true = np.array([0.0, 0.0, -synthetic.GRAVITY_NORM])
    w.gravity, w.gravity_constant = quat_to_matrix(quat_exp(rng.normal(3, sigma=0.02))) @ g_true, False
    st = rng.uniform(n_inertial, lo=lo, hi=min(hi, stamps_b[-1] - (kb // 2) * bias_dt) - 1e-9)
    q0, _ = rest_pose()
    a_b = quat_to_matrix(q0).T @ (-g_true)
    align = lambda c: np.array([[c[0], 0, 0], [c[3], c[1], 0], [c[4], c[5], c[2]]])
    gyro = S_g.reshape(3, 3).T @ a_b + BIAS_G  # (column-major 3 x 3 maps)
    acc = align(i_a) @ (quat_to_matrix(T_bs[:4]).T @ a_b) + BIAS_A
    meas = np.tile(np.concatenate([gyro, acc]), (n_inertial, 1))
    meas[:, :3] += rng.normal(n_inertial, 3, sigma=synthetic.GYRO_NOISE_DENSITY * np.sqrt(synthetic.IMU_RATE))
    meas[:, 3:] += rng.normal(n_inertial, 3, sigma=synthetic.ACCEL_NOISE_DENSITY * np.sqrt(synthetic.IMU_RATE))
    w.inertial_stamps, w.inertial_measurements = st, meas
    return w


def negate_odd_control_points(w):
    """A copy of the window whose odd control points carry the other sign of their quaternion: the same rotations, the same problem."""
    import copy
    v = copy.copy(w)
    v.control_points = w.control_points.copy()
    v.control_points[1::2, :4] *= -1.0
    return v


def pairs_below_t2(control_points):
    """Per pair of consecutive control points: is the relative rotation in the t2 < 1e-8 branch (below 1e-4 rad)?"""
    q = np.asarray(control_points)[:, :4]
    r = quat_mul(q[:-1] * [-1, -1, -1, 1], q[1:])
    r = r * np.sign(r[:, 3:4])
    n = np.linalg.norm(r[:, :3], axis=1)
    return (2 * np.arctan2(n, r[:, 3])) ** 2 < 1e-8


# ---- the committed windows ------------------------------------------------------------------------------------------------------------
# (priors, seed) per order, chosen on the CPU with the oracle alone so that five LM iterations are all successful (tests/
# test_degenerate_windows.py); an order-6 window of 16 control points with 12 priors or none does not manage that: its last control points
# are barely observed and steps get rejected.
SMALL = {4: (12, 1), 5: (12, 1), 6: (40, 1)}
WITH_IMU = {4: (40, 7), 5: (12, 15), 6: (40, 15)}
LONG = {4: (12, 1)}
ORDERS = (4, 5, 6)
AMPS = ("0", "1e-9", "thresholds")


def small(order, amp="0", flip=False, bearing=False):
    """16 control points, 40 landmarks, 3 stereo pairs, pose priors."""
    priors, seed = SMALL[order]
    return at_rest(order=order, amp=amp, flip=flip, bearing=bearing, with_priors=priors, seed=seed)


def visual_only(order, amp="thresholds", flip=False, bearing=False):
    """No priors: what the emulated fused build takes (pixels or bearings only)."""
    return at_rest(order=order, amp=amp, flip=flip, bearing=bearing, seed=SMALL[order][1])


def with_imu(order, amp="0", flip=False):
    """The small window with 80 inertial residuals of a body at rest (bordered reduced system: bias splines and gravity)."""
    priors, seed = WITH_IMU[order]
    return at_rest(order=order, amp=amp, flip=flip, with_priors=priors, n_inertial=80, seed=seed)


def long_window(amp="thresholds", flip=False):
    """Order 4, 60 control points, the observations of a landmark within 0.5 s: long enough for the two-ended factorisation."""
    priors, seed = LONG[4]
    return at_rest(order=4, n_cp=60, n_landmarks=150, amp=amp, flip=flip, span=0.5, with_priors=priors, seed=seed)


def held(order, amp="0", flip=False):
    """The small window with the rotations held (Window.rotation_constant): the only at-rest window whose control points are still at rest
    after a solve, see tests/test_degenerate_windows.py."""
    w = small(order, amp, flip)
    w.rotation_constant = True
    return w
