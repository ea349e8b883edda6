"""Numpy referee of the reduced system with free IMU blocks and free camera blocks.

The construction of tests/calibration_referee.py — the oracle's robustified rows assembled into a dense J'J, the landmarks eliminated by a
dense Schur complement, Jacobi scaling and Levenberg-Marquardt damping as the solver applies them — over the column order of
hs_reduced_system:
    [control points | bias_g points | bias_a points | gravity | free IMU coordinates | free camera coordinates].
IMU columns follow hs_set_imu_constancy: the free blocks of [T_bs 6 | i_g 6 | i_a 6 | S_g 9 | X_a 9], Ceres-local (T_bs on
Product(EigenQuaternion, R3), the rest Euclidean in the parameter layout of hs_set_imu); a window without inertial rows has none. Their rows
are the oracle's sensor-block Jacobians of the inertial factor (hs_linearize with the optional outputs), in the Jacobian mode asked for."""
import copy

import numpy as np

import hyperslam_amd as ha

import calibration_referee as cref

IMU_BLOCKS = ((0, 6), (6, 6), (12, 6), (18, 9), (27, 9))  # [T_bs | i_g | i_a | S_g | X_a] inside the IMU's 36 local coordinates
IMU_KEYS = ("J_extrinsics", "J_gyro_intrinsics", "J_acc_intrinsics", "J_gyro_sensitivity", "J_acc_offsets")


def imu_columns(w):
    """Column inside the IMU group of each of the 36 local IMU coordinates that is free; -1 otherwise. Returns (cols, ni)."""
    cols = -np.ones(36, int)
    if w.imu is None or w.imu_constant is None or len(np.asarray(w.inertial_stamps)) == 0:
        return cols, 0
    const = np.asarray(w.imu_constant, bool).reshape(5)
    n = 0
    for b, (first, size) in enumerate(IMU_BLOCKS):
        if not const[b]:
            cols[first:first + size] = np.arange(n, n + size)
            n += size
    return cols, n


def layout(w, oracle):
    """(P0, ni, nc): size of the system with every sensor block constant, free IMU coordinates, free camera coordinates."""
    w0 = copy.copy(w)
    w0.cam_constant = w0.imu_constant = None
    with ha.Problem(w0, lib=oracle) as c:
        P0 = c.dim_pose()
    return P0, imu_columns(w)[1], cref.camera_columns(w)[1]


def reduced_system(w, oracle, radius=1e4, mode=None):
    """(S, g) in the column order of hs_reduced_system, from the oracle's rows. mode: hs_set_inertial_jacobian (None: the default)."""
    w0 = copy.copy(w)
    w0.cam_constant = w0.imu_constant = None  # (the oracle keeps every sensor block constant; its rows carry their Jacobians all the same)
    cam_cols, nc = cref.camera_columns(w)
    imu_cols, ni = imu_columns(w)
    k, n_cp, n_lm = w.order, w.n_cp, len(w.landmarks)
    with ha.Problem(w0, lib=oracle) as c:
        if mode is not None:
            c.set_inertial_jacobian(mode)
        P0 = c.dim_pose()
        nbi = P0 - 6 * n_cp
        n_bias = (nbi - 2) // 6 if nbi else 0
        PI = P0 + ni  # first camera column
        P = PI + nc
        free = np.ones(P, bool)
        cpc = np.zeros(n_cp, bool) if w.cp_constant is None else np.asarray(w.cp_constant, bool)
        for i in range(n_cp):
            free[6 * i:6 * i + 3] &= not (cpc[i] or w.rotation_constant)
            free[6 * i + 3:6 * i + 6] &= not (cpc[i] or w.translation_constant)
        if nbi:
            free[6 * n_cp:6 * n_cp + 6 * n_bias] = not w.imu.get("bias_constant", False)
            free[6 * n_cp + 6 * n_bias:P0] = not w.gravity_constant
        lmc = np.zeros(n_lm, bool) if w.landmark_constant is None else np.asarray(w.landmark_constant, bool)
        H, gx = np.zeros((P, P)), np.zeros(P)
        Hll, bl, Hxl = np.zeros((n_lm, 3, 3)), np.zeros((n_lm, 3)), np.zeros((n_lm, P, 3))

        def rows(idx, J, r):
            J = J * free[idx][:, None, :]
            np.add.at(H, (idx[:, :, None], idx[:, None, :]), np.einsum("nri,nrj->nij", J, J))
            np.add.at(gx, idx, np.einsum("nri,nr->ni", J, r))
            return J

        for ftype, lm_of, cam_of in ((ha.HS_PIXEL, w.pixel_landmark, w.pixel_camera), (ha.HS_BEARING, w.bearing_landmark, w.bearing_camera)):
            n = c.num_residuals(ftype)
            if n == 0:
                continue
            L = c.linearize(ftype, True, sensor_blocks=True)
            lm, cam = np.asarray(lm_of, int), np.asarray(cam_of, int)
            nres = L["r"].shape[1]
            Jc = np.zeros((n, nres, 14))
            Jc[:, :, 0:6] = L["J_extrinsics"]
            if ftype == ha.HS_PIXEL:
                Jc[:, :, 6:10], Jc[:, :, 10:14] = L["J_intrinsics"], L["J_distortion"]
            ccol = cam_cols[cam]  # (n, 14)
            on = ccol >= 0
            # pose columns, then the camera columns; a local camera coordinate that is not in the system points at a dropped column
            idx = np.concatenate([6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :], np.where(on, PI + ccol, 0)], 1)
            J = np.concatenate([L["J_state"], Jc * on[:, None, :]], 2)
            J = rows(idx, J, L["r"])
            Jl = L["J_landmark"] * (~lmc[lm])[:, None, None]
            np.add.at(Hll, lm, np.einsum("nri,nrj->nij", Jl, Jl))
            np.add.at(bl, lm, np.einsum("nri,nr->ni", Jl, L["r"]))
            np.add.at(Hxl, (lm[:, None], idx), np.einsum("nri,nrj->nij", J, Jl))
        if c.num_residuals(ha.HS_PRIOR):
            L = c.linearize(ha.HS_PRIOR, True)
            rows(6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :], L["J_state"], L["r"])
        if c.num_residuals(ha.HS_INERTIAL):
            L = c.linearize(ha.HS_INERTIAL, True, sensor_blocks=True)
            kb = int(w.imu["bias_order"])
            f, fb = L["first_cp"][:, None], L["first_bias"][:, None]
            on = imu_cols >= 0
            Ji = np.concatenate([L[key] for key in IMU_KEYS], 2)[:, :, on]  # (n, 6, ni): the free columns, in block order
            idx = np.concatenate([6 * f + np.arange(6 * k), 6 * n_cp + 3 * fb + np.arange(3 * kb), 6 * n_cp + 3 * n_bias + 3 * fb + np.arange(3 * kb),
                                  np.broadcast_to(6 * n_cp + 6 * n_bias + np.arange(2), (len(f), 2)), np.broadcast_to(P0 + np.arange(ni), (len(f), ni))], 1)
            rows(idx, np.concatenate([L["J_state"], L["J_bias_g"], L["J_bias_a"], L["J_gravity"], Ji], 2), L["r"])
    Hx_diag = np.diag(H).copy()
    observed = np.zeros(n_lm, bool)
    observed[np.asarray(w.pixel_landmark, int)] = True
    observed[np.asarray(w.bearing_landmark, int)] = True
    act = observed & ~lmc
    Sred, gred = H.copy(), gx.copy()
    for l in np.nonzero(act)[0]:
        h = np.diag(Hll[l])
        sl = 1.0 / (1.0 + np.sqrt(h))
        V = sl[:, None] * Hll[l] * sl[None, :]
        V += np.diag(np.clip(np.diag(V), 1e-6, 1e32) / radius)
        W = Hxl[l] * sl[None, :]  # H_xl S_l
        Vi = np.linalg.inv(V)
        Sred -= W @ Vi @ W.T
        gred -= W @ Vi @ (sl * bl[l])
    s = 1.0 / (1.0 + np.sqrt(Hx_diag))
    S = s[:, None] * Sred * s[None, :]
    g = s * gred
    d = np.clip(s * s * Hx_diag, 1e-6, 1e32) / radius
    zero = Hx_diag <= 0.0
    S[np.diag_indices(P)] += np.where(zero, 0.0, d)
    S[zero, zero] = 1.0
    return S, g
