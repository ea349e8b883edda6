"""Numpy referee of the solve with free camera blocks: a Levenberg-Marquardt loop over the oracle's robustified rows.

The oracle keeps every camera block constant, so it cannot referee the estimation itself. What it can deliver — the rows of every factor
with the sensor-block Jacobians, the cost of any point, the retractions — is assembled here into the UNSCALED normal equations over
[control points | bias_g | bias_a | gravity | free camera coordinates] and the landmark blocks, and iterated with the rules of Ceres'
TrustRegionMinimizer + LevenbergMarquardtStrategy as oracle/hs_problem.hpp restates them (LM::run):
  Jacobi scaling s = 1 / (1 + sqrt(diag J'J)), fixed at the first iteration of a solve;
  LM diagonal clamp(s^2 diag J'J, 1e-6, 1e32) / radius; a column without a Jacobian entry is not in the program (unit row, zero step);
  dense solve of the Schur complement, landmark step by back-substitution  y_l = V^-1 (s_l b_l - S_l H_lx y_x);
  model cost change -(J step).(r + J step / 2), step valid iff > 0, five invalid steps in a row end the solve;
  parameter, function and gradient tolerances 1e-8 / 1e-6 / 1e-10, min_relative_decrease 1e-3;
  radius / max(1/3, 1 - (2 rho - 1)^3) after a successful step, radius / decrease_factor (2, 4, ...) after an unsuccessful one;
  candidate = Plus(x, delta) per block — cameras' T_bs through the oracle's manifold_plus(HS_MANIFOLD_SE3), intrinsics / distortion additive —
  and its cost from a fresh oracle Problem at the candidate values.
Camera columns follow calibration_referee.camera_columns."""
import copy

import numpy as np

import hyperslam_amd as ha

from calibration_referee import camera_columns

NO_CONVERGENCE, CONVERGENCE, FAILURE = 0, 1, 2  # hs_summary.termination


def _plain(w):
    w0 = copy.copy(w)
    w0.cam_constant = None  # (the oracle's upload refuses anything else; its rows carry the camera Jacobians all the same)
    return w0


LD = np.longdouble


def _solve(A, b):
    """A x = b for an extended-precision A, b: fp64 LU with rounds of iterative refinement on the extended-precision residual. Both ways of
    computing a step (Schur complement, full system) are formed in extended precision too, so that they agree far below the 1e-10 at which
    tests/test_calibration_solve_referee.py compares them (formed in fp64 they differ by 2e-10 on the windows with intrinsics columns)."""
    Af = np.asarray(A, float)
    x = np.linalg.solve(Af, np.asarray(b, float)).astype(LD)
    for _ in range(3):
        x = x + np.linalg.solve(Af, np.asarray(b - A @ x, float))
    return x


def _inv3(V):
    """Inverse of a symmetric 3 x 3 matrix by cofactors (any precision)."""
    a, b, c, d, e, f = V[0, 0], V[0, 1], V[0, 2], V[1, 1], V[1, 2], V[2, 2]
    C = np.array([[d * f - e * e, c * e - b * f, b * e - c * d], [c * e - b * f, a * f - c * c, b * c - a * e], [b * e - c * d, b * c - a * e, a * d - b * b]], V.dtype)
    return C / (a * C[0, 0] + b * C[0, 1] + c * C[0, 2])


class System:
    """Unscaled normal equations of window w at its current values."""

    def __init__(self, w, oracle):
        cam_cols, nc = camera_columns(w)
        k, n_cp, n_lm = w.order, w.n_cp, len(w.landmarks)
        with ha.Problem(_plain(w), lib=oracle) as c:
            P0 = c.dim_pose()
            nbi = P0 - 6 * n_cp
            n_bias = (nbi - 2) // 6 if nbi else 0
            P = P0 + nc
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
                Jc = np.zeros((n, L["r"].shape[1], 14))
                Jc[:, :, 0:6] = L["J_extrinsics"]
                if ftype == ha.HS_PIXEL:
                    Jc[:, :, 6:10], Jc[:, :, 10:14] = L["J_intrinsics"], L["J_distortion"]
                ccol = cam_cols[cam]
                on = ccol >= 0
                idx = np.concatenate([6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :], np.where(on, P0 + ccol, 0)], 1)
                J = rows(idx, np.concatenate([L["J_state"], Jc * on[:, None, :]], 2), L["r"])
                Jl = L["J_landmark"] * (~lmc[lm])[:, None, None]
                np.add.at(Hll, lm, np.einsum("nri,nrj->nij", Jl, Jl))
                np.add.at(bl, lm, np.einsum("nri,nr->ni", Jl, L["r"]))
                np.add.at(Hxl, (lm[:, None], idx), np.einsum("nri,nrj->nij", J, Jl))
            if c.num_residuals(ha.HS_PRIOR):
                L = c.linearize(ha.HS_PRIOR, True)
                rows(6 * L["first_cp"][:, None] + np.arange(6 * k)[None, :], L["J_state"], L["r"])
            if c.num_residuals(ha.HS_INERTIAL):
                L = c.linearize(ha.HS_INERTIAL, True)
                kb = int(w.imu["bias_order"])
                f, fb = L["first_cp"][:, None], L["first_bias"][:, None]
                idx = np.concatenate([6 * f + np.arange(6 * k), 6 * n_cp + 3 * fb + np.arange(3 * kb), 6 * n_cp + 3 * n_bias + 3 * fb + np.arange(3 * kb),
                                      np.broadcast_to(6 * n_cp + 6 * n_bias + np.arange(2), (len(f), 2))], 1)
                rows(idx, np.concatenate([L["J_state"], L["J_bias_g"], L["J_bias_a"], L["J_gravity"]], 2), L["r"])
            self.cost = c.cost()
        observed = np.zeros(n_lm, bool)
        observed[np.asarray(w.pixel_landmark, int)] = True
        observed[np.asarray(w.bearing_landmark, int)] = True
        self.H, self.gx, self.Hll, self.bl, self.Hxl = H, gx, Hll, bl, Hxl
        self.act = observed & ~lmc        # eliminated landmarks
        self.P, self.P0, self.nc, self.n_bias, self.cam_cols = P, P0, nc, n_bias, cam_cols
        self.active = np.diag(H) > 0.0    # columns in the program

    def scaling(self):
        return 1.0 / (1.0 + np.sqrt(np.diag(self.H))), 1.0 / (1.0 + np.sqrt(np.einsum("lii->li", self.Hll)))

    def gradient_max_norm(self):
        m = np.abs(self.gx).max() if self.P else 0.0
        return max(m, np.abs(self.bl).max() if len(self.bl) else 0.0)

    def landmark_blocks(self, sl, radius):
        """Per eliminated landmark: V^-1 of the scaled, damped block and its LM diagonal."""
        out = {}
        for l in np.nonzero(self.act)[0]:
            V = sl[l][:, None].astype(LD) * self.Hll[l] * sl[l][None, :]
            d = np.clip(np.diag(V), 1e-6, 1e32) / radius
            out[l] = (_inv3(V + np.diag(d)), d)
        return out

    def scaled_system(self, s, sl, radius):
        """(S, g, D): the scaled, damped Schur complement, its right-hand side and the LM diagonal of the pose side (hs_reduced_system's layout)."""
        Sred, gred = self.H.astype(LD), self.gx.astype(LD)
        for l, (Vi, _) in self.landmark_blocks(sl, radius).items():
            W = self.Hxl[l] * sl[l][None, :]
            Sred -= W @ Vi @ W.T
            gred -= W @ Vi @ (sl[l] * self.bl[l])
        S = s[:, None] * Sred * s[None, :]
        g = s * gred
        D = np.where(self.active, np.clip(s * s * np.diag(self.H), 1e-6, 1e32) / radius, 0.0)
        S[np.diag_indices(self.P)] += D
        off = ~self.active
        S[off, :] = 0.0
        S[:, off] = 0.0
        S[off, off] = 1.0
        g[off] = 0.0
        return S, g, D

    def step_schur(self, s, sl, radius):
        """Unscaled step (delta_x, delta_l) by Schur complement + back-substitution."""
        S, g, _ = self.scaled_system(s, sl, radius)
        y = _solve(S, g)
        dx = -s * y
        dl = np.zeros_like(self.bl)
        for l, (Vi, _) in self.landmark_blocks(sl, radius).items():
            W = self.Hxl[l] * sl[l][None, :]
            yl = Vi @ (sl[l] * self.bl[l] - W.T @ (s * y))
            dl[l] = np.asarray(-sl[l] * yl, float)
        return np.asarray(dx, float), dl

    def step_full(self, s, sl, radius):
        """The same step from the full damped normal equations, landmarks included, in one dense solve."""
        la = np.nonzero(self.act)[0]
        P, n = self.P, self.P + 3 * len(la)
        A, b, sc = np.zeros((n, n), LD), np.zeros(n, LD), np.ones(n, LD)
        A[:P, :P], b[:P], sc[:P] = self.H, self.gx, s
        for i, l in enumerate(la):
            o = P + 3 * i
            A[o:o + 3, o:o + 3], A[:P, o:o + 3], A[o:o + 3, :P] = self.Hll[l], self.Hxl[l], self.Hxl[l].T
            b[o:o + 3], sc[o:o + 3] = self.bl[l], sl[l]
        A = sc[:, None] * A * sc[None, :]
        b = sc * b
        on = np.r_[self.active, np.ones(3 * len(la), bool)]
        A[np.diag_indices(n)] += np.where(on, np.clip(np.diag(A), 1e-6, 1e32) / radius, 0.0)
        A[~on, :] = 0.0
        A[:, ~on] = 0.0
        A[~on, ~on] = 1.0
        b[~on] = 0.0
        y = _solve(A, b)
        dl = np.zeros_like(self.bl)
        for i, l in enumerate(la):
            dl[l] = np.asarray(-(sc * y)[P + 3 * i:P + 3 * i + 3], float)
        return np.asarray(-(sc * y)[:P], float), dl

    def model_cost_change(self, dx, dl):
        """-(J step).(r + J step / 2) = -g.step - step'J'J step / 2 over every block."""
        lin = self.gx @ dx + np.einsum("li,li->", self.bl, dl)
        quad = dx @ self.H @ dx + 2.0 * np.einsum("i,lij,lj->", dx, self.Hxl, dl) + np.einsum("li,lij,lj->", dl, self.Hll, dl)
        return -lin - 0.5 * quad


def retract(w, sysm, dx, dl, oracle):
    """Candidate window Plus(x, delta), and (|x|^2 over the blocks in the program, |x+ - x|^2)."""
    c = copy.deepcopy(w)
    n_cp, nb, P0 = w.n_cp, sysm.n_bias, sysm.P0
    act = sysm.active
    xs = 0.0
    with ha.Problem(_plain(w), lib=oracle) as o:
        c.control_points = o.manifold_plus(ha.HS_MANIFOLD_CONTROL_POINT, w.control_points, dx[:6 * n_cp].reshape(n_cp, 6))
        cp_on = act[:6 * n_cp].reshape(n_cp, 6).any(1)
        xs += (np.asarray(w.control_points)[cp_on] ** 2).sum()
        c.landmarks = np.asarray(w.landmarks, float) + dl
        xs += (np.asarray(w.landmarks, float)[sysm.act] ** 2).sum()
        if P0 > 6 * n_cp:
            c.imu = dict(w.imu)
            for key, off in (("bias_g", 6 * n_cp), ("bias_a", 6 * n_cp + 3 * nb)):
                b = np.array(w.imu[key], float)
                on = act[off:off + 3 * nb].reshape(nb, 3)[:, 0]
                xs += (b[on] ** 2).sum()
                b[:, :3] += dx[off:off + 3 * nb].reshape(nb, 3)
                c.imu[key] = b
            if act[6 * n_cp + 6 * nb]:
                xs += (np.asarray(w.gravity) ** 2).sum()
                c.gravity = o.manifold_plus(ha.HS_MANIFOLD_SPHERE3, np.asarray(w.gravity, float)[None, :], dx[6 * n_cp + 6 * nb:P0][None, :])[0]
        c.cam_T_bs, c.cam_intrinsics, c.cam_distortion = (np.array(a, float) for a in (w.cam_T_bs, w.cam_intrinsics, w.cam_distortion))
        for cam in range(len(c.cam_T_bs)):
            cols = sysm.cam_cols[cam]
            if cols[0] >= 0:
                xs += (c.cam_T_bs[cam] ** 2).sum()
                c.cam_T_bs[cam] = o.manifold_plus(ha.HS_MANIFOLD_SE3, c.cam_T_bs[cam][None, :], dx[P0 + cols[0:6]][None, :])[0]
            if cols[6] >= 0:
                xs += (c.cam_intrinsics[cam] ** 2).sum()
                c.cam_intrinsics[cam] = c.cam_intrinsics[cam] + dx[P0 + cols[6:10]]
            if cols[10] >= 0:
                xs += (c.cam_distortion[cam] ** 2).sum()
                c.cam_distortion[cam] = c.cam_distortion[cam] + dx[P0 + cols[10:14]]
    ss = ((np.asarray(c.control_points) - np.asarray(w.control_points)) ** 2).sum() + ((c.landmarks - np.asarray(w.landmarks, float)) ** 2).sum()
    if P0 > 6 * n_cp:
        ss += sum(((np.asarray(c.imu[k]) - np.asarray(w.imu[k], float)) ** 2).sum() for k in ("bias_g", "bias_a"))
        ss += ((np.asarray(c.gravity) - np.asarray(w.gravity)) ** 2).sum()
    ss += sum(((np.asarray(a) - np.asarray(b, float)) ** 2).sum() for a, b in
              ((c.cam_T_bs, w.cam_T_bs), (c.cam_intrinsics, w.cam_intrinsics), (c.cam_distortion, w.cam_distortion)))
    return c, xs, ss


def cost_of(w, oracle):
    with ha.Problem(_plain(w), lib=oracle) as c:
        return c.cost()


def solve(w, oracle, max_iterations=5, radius=1e4):
    """LM::run on window w (free camera blocks per w.cam_constant). Returns (summary in the layout of Problem.solve, final window)."""
    w = copy.deepcopy(w)
    sysm = System(w, oracle)
    s, sl = sysm.scaling()
    cost, gmax = sysm.cost, sysm.gradient_max_norm()
    its = [dict(iteration=0, cost=cost, cost_change=0.0, gradient_max_norm=gmax, step_norm=0.0, relative_decrease=0.0, radius=radius,
                step_is_valid=1, step_is_successful=1)]
    out = dict(initial_cost=cost, num_iterations=0, num_successful_steps=0, termination=NO_CONVERGENCE)
    decrease_factor, invalid_streak, it = 2.0, 0, 0
    while True:
        it += 1
        if it - 1 >= max_iterations:
            out["termination"] = NO_CONVERGENCE
            break
        if gmax <= 1e-10 or radius <= 1e-32:
            out["termination"] = CONVERGENCE
            break
        rec = dict(iteration=it, cost=cost, cost_change=0.0, gradient_max_norm=gmax, step_norm=0.0, relative_decrease=0.0, radius=radius,
                   step_is_valid=0, step_is_successful=0)
        out["num_iterations"] = it
        try:
            dx, dl = sysm.step_schur(s, sl, radius)
            mcc = sysm.model_cost_change(dx, dl)
            valid = bool(np.isfinite(dx).all() and np.isfinite(dl).all() and mcc > 0.0)
        except np.linalg.LinAlgError:
            valid = False
        if not valid:
            invalid_streak += 1
            if invalid_streak >= 5:
                out["termination"] = FAILURE
                its.append(rec)
                break
            radius *= 0.5
            rec["radius"] = radius
            its.append(rec)
            continue
        invalid_streak = 0
        rec["step_is_valid"] = 1
        cand, xs, ss = retract(w, sysm, dx, dl, oracle)
        cand_cost = cost_of(cand, oracle)
        rec["step_norm"] = np.sqrt(ss)
        if rec["step_norm"] <= 1e-8 * (np.sqrt(xs) + 1e-8):
            out["termination"] = CONVERGENCE
            its.append(rec)
            break
        rec["cost_change"] = cost - cand_cost
        if abs(rec["cost_change"]) <= 1e-6 * cost:
            out["termination"] = CONVERGENCE
            its.append(rec)
            break
        rho = rec["relative_decrease"] = (cost - cand_cost) / mcc
        if rho > 1e-3:
            rec["step_is_successful"] = 1
            out["num_successful_steps"] += 1
            w = cand
            sysm = System(w, oracle)
            cost, gmax = sysm.cost, sysm.gradient_max_norm()
            rec["cost"], rec["gradient_max_norm"] = cost, gmax
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3))
            decrease_factor = 2.0
        else:
            rec["cost"] = cand_cost
            radius = radius / decrease_factor
            decrease_factor *= 2.0
        rec["radius"] = radius
        its.append(rec)
    out["final_cost"] = cost
    out["iterations"] = its
    return out, w


def condition(w, oracle, radius=1e4):
    """cond of the scaled, damped reduced system at the window's values."""
    sysm = System(w, oracle)
    s, sl = sysm.scaling()
    return np.linalg.cond(np.asarray(sysm.scaled_system(s, sl, radius)[0], float))


def flags(w, **free):
    """Constancy flags: every block constant but those named, e.g. cam1="tid" (T_bs, intrinsics, distortion of camera 1 free)."""
    c = np.ones((len(w.cam_T_bs), 3), np.uint8)
    for name, blocks in free.items():
        for b in blocks:
            c[int(name[3:]), "tid".index(b)] = 0
    return c


def free_camera_windows():
    """(name, window with free camera blocks, dense: small enough for the one-launch dense solve) — the windows of the device parity tests."""
    from hyperslam_amd import synthetic
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=40, obs_pairs=3)
    w.cam_constant = flags(w, cam1="tid")
    yield "pixel_k4_cam1_free", w
    w = synthetic.small_visual(order=5, n_cp=18, n_landmarks=80, obs_pairs=4, seed=22, with_priors=30)
    w.cam_constant = flags(w, cam0="id", cam1="id")
    yield "pixel_prior_k5_intrinsics_distortion", w
    w = synthetic.small_visual(order=4, n_cp=16, n_landmarks=60, obs_pairs=3, bearing=True, seed=9)
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(12, np.uint8)]
    w.cam_constant = flags(w, cam1="t")
    yield "bearing_k4_cam1_T_bs", w
    w = synthetic.small_visual(order=6, n_cp=20, n_landmarks=50, obs_pairs=3, seed=8)
    w.cp_constant = np.r_[np.ones(6, np.uint8), np.zeros(14, np.uint8)]
    w.landmark_constant = (np.arange(50) % 5 == 0).astype(np.uint8)
    w.cam_constant = flags(w, cam1="tid")
    yield "frozen_const_landmarks_k6_cam1_free", w
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.cam_constant = flags(w, cam1="t")
    yield "inertial_k4_cam1_T_bs", w
    w = synthetic.small_visual(order=4, n_cp=48, n_landmarks=120, obs_pairs=3, seed=13, span=0.5)
    w.cam_constant = flags(w, cam1="tid")
    yield "pixel_k4_48cp_cam1_free", w
