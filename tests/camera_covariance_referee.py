"""Numpy referee of the covariance with free camera blocks (hs_set_camera_covariance), and the windows its tests share.

Independent of every device build path and of the block formulas the device uses: the oracle's robustified rows (hs_linearize with the
sensor-block Jacobians) are assembled into a dense J'J over [control points | bias_g points | bias_a points | gravity | free camera
coordinates] AND the landmarks — constant columns and constant / unobserved landmarks dropped, no damping — and that full matrix is
inverted densely (on its Jacobi-scaled form, unscaled afterwards). Landmark blocks are read off the full inverse.

Column order of the camera coordinates: tests/calibration_referee.py::camera_columns (the order of hs_reduced_system). The condition number
that sets a window's tolerance, bar(cond) = max(1e-8, cond * 1e-14), is that of the Jacobi-scaled reduced matrix (landmarks eliminated,
scale 1 / (1 + sqrt(diag J'J)) as in the solver) including the camera columns."""
import copy

import numpy as np

import hyperslam_amd as ha
from hyperslam_amd import synthetic

from calibration_referee import camera_columns


def bar(cond):
    return max(1e-8, cond * 1e-14)


def rel(a, b):
    if np.size(a) == 0 or np.size(b) == 0:
        raise ValueError(f"rel() of an empty selection (shapes {np.shape(a)} and {np.shape(b)}): nothing would be compared")
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def flags(w, **free):
    """Constancy flags: every block constant but those named, e.g. cam1="tid" (T_bs, intrinsics, distortion of camera 1 free)."""
    c = np.ones((len(w.cam_T_bs), 3), np.uint8)
    for name, blocks in free.items():
        for b in blocks:
            c[int(name[3:]), "tid".index(b)] = 0
    return c


def assemble(w, oracle):
    """Dense J'J blocks from the oracle's rows: H (P x P) over the reduced unknowns, camera columns last; Hll (n_lm x 3 x 3); Hxl
    (n_lm x P x 3); the masks of free columns and of landmarks in the problem (observed and not constant); nc."""
    w0 = copy.copy(w)
    w0.cam_constant = None  # (the oracle keeps every camera block constant; its rows carry the camera Jacobians all the same)
    cam_cols, nc = camera_columns(w)
    k, n_cp, n_lm = w.order, w.n_cp, len(w.landmarks)
    with ha.Problem(w0, lib=oracle) as c:
        P0 = c.dim_pose()
        nbi = P0 - 6 * n_cp
        n_bias = (nbi - 2) // 6 if nbi else 0
        P = P0 + nc
        H, Hll, Hxl = np.zeros((P, P)), np.zeros((n_lm, 3, 3)), np.zeros((n_lm, P, 3))

        def rows(idx, J):
            np.add.at(H, (idx[:, :, None], idx[:, None, :]), np.einsum("nri,nrj->nij", J, J))

        for ftype, lm_of, cam_of in ((ha.HS_PIXEL, w.pixel_landmark, w.pixel_camera), (ha.HS_BEARING, w.bearing_landmark, w.bearing_camera)):
            n = c.num_residuals(ftype)
            if n == 0:
                continue
            L = c.linearize(ftype, True, sensor_blocks=True)
            lm, cam = np.asarray(lm_of, int), np.asarray(cam_of, int)
            Jc = np.zeros((n, L["r"].shape[1], 14))
            Jc[:, :, 0:6] = L["J_extrinsics"]
            if ftype == ha.HS_PIXEL:
                Jc[:, :, 6:10], Jc[:, :, 10:14] = L["J_intrinsics"], L["J_distortion"]
            ccol = cam_cols[cam]
            on = ccol >= 0
            idx = np.concatenate([6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :], np.where(on, P0 + ccol, 0)], 1)
            J = np.concatenate([L["J_state"], Jc * on[:, None, :]], 2)
            rows(idx, J)
            Jl = L["J_landmark"]
            np.add.at(Hll, lm, np.einsum("nri,nrj->nij", Jl, Jl))
            np.add.at(Hxl, (lm[:, None], idx), np.einsum("nri,nrj->nij", J, Jl))
        if c.num_residuals(ha.HS_PRIOR):
            L = c.linearize(ha.HS_PRIOR, True)
            rows(6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :], L["J_state"])
        if c.num_residuals(ha.HS_INERTIAL):
            L = c.linearize(ha.HS_INERTIAL, True)
            kb = int(w.imu["bias_order"])
            f, fb = L["first_cp"][:, None], L["first_bias"][:, None]
            idx = np.concatenate([6 * f + np.arange(6 * k), 6 * n_cp + 3 * fb + np.arange(3 * kb), 6 * n_cp + 3 * n_bias + 3 * fb + np.arange(3 * kb),
                                  np.broadcast_to(6 * n_cp + 6 * n_bias + np.arange(2), (len(f), 2))], 1)
            rows(idx, np.concatenate([L["J_state"], L["J_bias_g"], L["J_bias_a"], L["J_gravity"]], 2))
    free = np.ones(P, bool)
    cpc = np.zeros(n_cp, bool) if w.cp_constant is None else np.asarray(w.cp_constant, bool)
    for i in range(n_cp):
        free[6 * i:6 * i + 3] &= not (cpc[i] or w.rotation_constant)
        free[6 * i + 3:6 * i + 6] &= not (cpc[i] or w.translation_constant)
    if nbi:
        free[6 * n_cp:6 * n_cp + 6 * n_bias] = not w.imu.get("bias_constant", False)
        free[6 * n_cp + 6 * n_bias:P0] = not w.gravity_constant
    lmc = np.zeros(n_lm, bool) if w.landmark_constant is None else np.asarray(w.landmark_constant, bool)
    observed = np.zeros(n_lm, bool)
    observed[np.asarray(w.pixel_landmark, int)] = True
    observed[np.asarray(w.bearing_landmark, int)] = True
    return dict(H=H, Hll=Hll, Hxl=Hxl, free=free, act=observed & ~lmc, observed=observed, nc=nc, P=P)


def scaled_reduced(A):
    """The Jacobi-scaled reduced matrix over the free columns (landmarks eliminated by a dense Schur complement) and its scale."""
    H, act, free = A["H"], A["act"], A["free"]
    Hxl = A["Hxl"][act][:, free, :]
    W = Hxl @ np.linalg.inv(A["Hll"][act])
    Sf = H[np.ix_(free, free)] - np.tensordot(W, Hxl, axes=([0, 2], [0, 2]))
    d = 1.0 / (1.0 + np.sqrt(np.diag(H)[free]))  # the solver's Jacobi scaling
    return Sf * d[:, None] * d[None, :], d


def referee(w, oracle):
    """Sigma (P x P, zero rows / columns for constant coordinates), landmark blocks (n_lm x 3 x 3: NaN unobserved, zero constant), cond of the
    Jacobi-scaled reduced matrix, and the assembly (for the block formula and the admissibility checks)."""
    A = assemble(w, oracle)
    fi, la = np.flatnonzero(A["free"]), np.flatnonzero(A["act"])
    nf, n = len(fi), len(fi) + 3 * len(la)
    F = np.zeros((n, n))
    F[:nf, :nf] = A["H"][np.ix_(fi, fi)]
    for j, l in enumerate(la):
        s = slice(nf + 3 * j, nf + 3 * j + 3)
        F[s, s] = A["Hll"][l]
        F[:nf, s] = A["Hxl"][l][fi]
        F[s, :nf] = A["Hxl"][l][fi].T
    s = 1.0 / np.sqrt(np.diag(F))
    Fi = np.linalg.inv(F * s[:, None] * s[None, :]) * s[:, None] * s[None, :]
    P = A["P"]
    Sigma = np.zeros((P, P))
    Sigma[np.ix_(fi, fi)] = Fi[:nf, :nf]
    lm_cov = np.zeros((len(w.landmarks), 3, 3))
    lm_cov[~A["observed"]] = np.nan
    for j, l in enumerate(la):
        lm_cov[l] = Fi[nf + 3 * j:nf + 3 * j + 3, nf + 3 * j:nf + 3 * j + 3]
    M, d = scaled_reduced(A)
    return dict(Sigma=Sigma, lm_cov=lm_cov, cond=np.linalg.cond(M), M=M, d=d, A=A, nc=A["nc"])


def block_formula(A, Sigma):
    """The landmark blocks by the formula of DESIGN §12 / §13, from the same rows: with s_l = 1 / (1 + sqrt(diag H_ll)), V = S_l H_ll S_l = L L',
    Yh = H_pl S_l L^-T, Y_c = L^-1 S_l H_lc and G = [Yh ; Y_c'] over the pose rows the landmark touches and the camera columns,
    Sigma_ll = S_l L^-T (I + G' Sigma_[p_l,c] G) L^-1 S_l."""
    P, nc = A["P"], A["nc"]
    out = np.zeros((len(A["act"]), 3, 3))
    out[~A["observed"]] = np.nan
    for l in np.flatnonzero(A["act"]):
        sl = 1.0 / (1.0 + np.sqrt(np.diag(A["Hll"][l])))
        L = np.linalg.cholesky(sl[:, None] * A["Hll"][l] * sl[None, :])
        Li = np.linalg.inv(L)
        G = (A["Hxl"][l] * sl[None, :]) @ Li.T  # rows of every reduced unknown; only the landmark's pose rows and the camera rows are non-zero
        touched = np.flatnonzero(np.abs(A["Hxl"][l][:P - nc]).sum(1) > 0.0) // 6  # (none: seen from constant control points only — zero rows)
        pose = np.arange(6 * touched.min(), 6 * touched.max() + 6) if len(touched) else np.arange(0)
        idx = np.r_[pose, np.arange(P - nc, P)]
        mid = np.eye(3) + G[idx].T @ Sigma[np.ix_(idx, idx)] @ G[idx]
        out[l] = sl[:, None] * (Li.T @ mid @ Li) * sl[None, :]
    return out


def perturbation_response(R, n_cp, draws=5, eps=1e-13, seed=20240607):
    """How far Sigma_cc and the camera columns of Sigma_pc move, each relative to its own max-norm, when the scaled reduced matrix is perturbed
    entry by entry by a symmetric relative eps (uniform in [-eps, eps]); the largest over the draws. (pc, cc)."""
    M, d, free, nc = R["M"], R["d"], R["A"]["free"], R["nc"]
    rng = np.random.default_rng(seed)
    pos = np.cumsum(free) - 1  # index of a free column inside M
    cam = pos[np.arange(len(free) - nc, len(free))]
    pose = pos[np.flatnonzero(free[:6 * n_cp])]

    def blocks(Mx):
        S = np.linalg.inv(Mx) * d[:, None] * d[None, :]
        return S[np.ix_(pose, cam)], S[np.ix_(cam, cam)]

    pc0, cc0 = blocks(M)
    worst = [0.0, 0.0]
    for _ in range(draws):
        E = rng.uniform(-eps, eps, M.shape)
        E = np.triu(E) + np.triu(E, 1).T
        pc, cc = blocks(M * (1.0 + E))
        worst = [max(worst[0], rel(pc, pc0)), max(worst[1], rel(cc, cc0))]
    return tuple(worst)


# ---- the windows of tests/test_gpu_camera_covariance.py; tests/test_camera_covariance_referee.py asserts their admissibility on the CPU ------------

def gauge(w):
    w.cp_constant = np.r_[np.ones(w.order, np.uint8), np.zeros(w.n_cp - w.order, np.uint8)]
    return w


def trim_bias(w, oracle):
    """Drops the trailing bias control points no inertial row reaches (free coordinates without information)."""
    with ha.Problem(w, lib=oracle) as c:
        used = int(c.linearize(ha.HS_INERTIAL, True)["first_bias"].max()) + int(w.imu["bias_order"])
    w.imu["bias_g"], w.imu["bias_a"] = w.imu["bias_g"][:used], w.imu["bias_a"][:used]
    return w


def bearing_window():
    return gauge(synthetic.small_visual(order=4, n_cp=18, n_landmarks=60, obs_pairs=3, bearing=True, seed=9, with_priors=18))


# Windows A and B are not the ones first proposed for them — small_visual(4, 16, 40, obs_pairs=3, with_priors=16) with cam1="tid", and this B
# with cam0="id", cam1="id". Both were turned down by test_window_is_admissible's perturbation check, on CPU quantities alone: a relative 1e-13
# moved their camera blocks by 7.5e-9 (A: Sigma_pc) and 9.3e-9 / 6.4e-9 (B: Sigma_pc / Sigma_cc) against bar / 10 = 1e-9 and 1.8e-9. With the
# intrinsics of BOTH cameras free and no T_bs, no variant of B passed (more landmarks, priors, longer tracks, a frozen prefix: 1.6e-9 .. 1.9e-8):
# the two focal lengths share a weakly determined direction. The replacements keep what the windows are for — A: no IMU, the border is the 14
# columns of one camera; B: intrinsics / distortion blocks of both cameras and no T_bs — and respond with 2.7e-10 / 3.2e-10 (A) and
# 2.7e-10 / 3.2e-11 (B).
WINDOWS = ("A", "B", "D", "bearing", "rotation_constant", "translation_constant", "F", "I4", "I5", "I6", "I4_both", "W")
BOTH_BUILD_PATHS = ("A", "B")  # (the windows run on the fused and on the records build path, HS_BUILD_PATH)
_cache = {}


def window(name, oracle):
    """(window with its camera flags, has an IMU). Built once per name."""
    if name in _cache:
        return _cache[name]
    imu = False
    if name == "A":
        w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, seed=10, with_priors=16)
        w.cam_constant = flags(w, cam1="tid")
    elif name == "B":
        w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, seed=10, with_priors=20)
        w.cam_constant = flags(w, cam0="id", cam1="d")
    elif name == "D":
        w = synthetic.small_visual(order=5, n_cp=20, n_landmarks=60, obs_pairs=3, seed=31, with_priors=20)
        w.cp_constant = np.r_[np.ones(5, np.uint8), np.zeros(15, np.uint8)]
        w.landmark_constant = (np.arange(60) % 4 == 0).astype(np.uint8)
        w.cam_constant = flags(w, cam0="id", cam1="tid")
    elif name == "bearing":
        w = bearing_window()
        w.cam_constant = flags(w, cam1="t")
    elif name in ("rotation_constant", "translation_constant"):
        w = gauge(synthetic.small_visual(order=4, n_cp=18, n_landmarks=50, obs_pairs=3, seed=35, with_priors=18))
        setattr(w, name, True)
        w.cam_constant = flags(w, cam1="tid")
    elif name == "F":
        w = synthetic.small_visual(order=4, n_cp=34, n_landmarks=80, obs_pairs=6, seed=11, span=3.2)
        w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(30, np.uint8)]
        w.cam_constant = flags(w, cam1="tid")
    elif name in ("I4", "I5", "I6", "I4_both"):
        order = int(name[1])
        w = trim_bias(gauge(synthetic.small_inertial(order=order, n_cp=18)), oracle)
        w.cam_constant = flags(w, cam0="tid", cam1="tid") if name == "I4_both" else (flags(w, cam0="t", cam1="tid") if order == 6 else flags(w, cam1="tid"))
        imu = True
    elif name == "W":
        w = synthetic.small_visual(order=4, n_cp=30, n_landmarks=60, obs_pairs=6, seed=40, span=2.8)
        synthetic.add_imu(w, synthetic.SplitMix64(77), 150, identity=True, gravity_constant=False)
        w = trim_bias(gauge(w), oracle)
        w.cam_constant = flags(w, cam1="tid")
        imu = True
    else:
        raise KeyError(name)
    _cache[name] = (w, imu)
    return _cache[name]


_referees = {}


def window_referee(name, oracle):
    """The referee of a named window, computed once and shared (its arrays are not to be changed)."""
    if name not in _referees:
        _referees[name] = referee(window(name, oracle)[0], oracle)
    return _referees[name]


def constant_cameras(w):
    wc = copy.copy(w)
    wc.cam_constant = None
    return wc
