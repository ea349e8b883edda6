"""Numpy referee of the solve with free IMU blocks ("Estimation in hs_solve"): the Levenberg-Marquardt loop of
tests/calibration_solve_referee.py over the column order
    [control points | bias_g points | bias_a points | gravity | free IMU coordinates | free camera coordinates].

The oracle keeps every sensor block constant but evaluates at whatever hs_set_imu gave it, so it delivers what a referee needs: the rows of the
inertial factor with the sensor-block Jacobians (linearize(HS_INERTIAL, True, sensor_blocks=True), as tests/imu_calibration_referee.py takes
them), the cost of any point and the retractions. `System` here is calibration_solve_referee.System with the IMU columns inserted in front of
the camera columns: no landmark touches them, so H_xl has zero rows there and the Schur complement, the back-substitution and the model cost
change of the base class apply unchanged. The candidate's T_bs goes through the oracle's manifold_plus(HS_MANIFOLD_SE3), i_g / i_a / S_g / X_a
are additive in the parameter layout of hs_set_imu, and the candidate's cost comes from a fresh oracle Problem at the candidate IMU values.
The loop restates calibration_solve_referee.solve statement for statement: with every IMU block constant the two agree to rounding
(tests/test_imu_calibration_solve_referee.py)."""
import copy

import numpy as np

import hyperslam_amd as ha

import calibration_solve_referee as csr
from calibration_solve_referee import NO_CONVERGENCE, CONVERGENCE, FAILURE  # noqa: F401
from imu_calibration_referee import IMU_BLOCKS, IMU_KEYS, imu_columns

IMU_NAMES = ("T_bs", "i_g", "i_a", "S_g", "X_a")
BLOCKS = "tgasx"  # [T_bs, i_g, i_a, S_g, X_a]


def imu_flags(free):
    """Constancy flags with the named blocks free, e.g. "gx" = i_g and X_a."""
    c = np.ones(5, np.uint8)
    for b in free:
        c[BLOCKS.index(b)] = 0
    return c


def _plain(w):
    w0 = csr._plain(w)
    w0.imu_constant = None  # (the oracle's upload refuses anything else; its rows carry the IMU Jacobians all the same)
    return w0


class System(csr.System):
    """Unscaled normal equations of window w at its current values, IMU columns (w.imu_constant) included. mode: hs_set_inertial_jacobian
    (None: the default)."""

    def __init__(self, w, oracle, mode=None):
        super().__init__(_plain_keep_cameras(w), oracle)
        imu_cols, ni = imu_columns(w)
        self.ni, self.imu_cols, self.mode = ni, imu_cols, mode
        if w.imu is None or len(np.asarray(w.inertial_stamps)) == 0 or (ni == 0 and mode is None):
            return
        k, n_cp, n_bias, P0, Pold = w.order, w.n_cp, self.n_bias, self.P0, self.P
        P = Pold + ni
        new = np.r_[np.arange(P0), P0 + ni + np.arange(Pold - P0)]  # where the base class's columns go
        H, gx, Hxl = np.zeros((P, P)), np.zeros(P), np.zeros((len(self.Hxl), P, 3))
        H[np.ix_(new, new)], gx[new], Hxl[:, new, :] = self.H, self.gx, self.Hxl
        free = np.ones(P0, bool)
        cpc = np.zeros(n_cp, bool) if w.cp_constant is None else np.asarray(w.cp_constant, bool)
        for i in range(n_cp):
            free[6 * i:6 * i + 3] &= not (cpc[i] or w.rotation_constant)
            free[6 * i + 3:6 * i + 6] &= not (cpc[i] or w.translation_constant)
        free[6 * n_cp:6 * n_cp + 6 * n_bias] = not w.imu.get("bias_constant", False)
        free[6 * n_cp + 6 * n_bias:P0] = not w.gravity_constant
        with ha.Problem(_plain(w), lib=oracle) as c:
            kb = int(w.imu["bias_order"])

            def inertial_rows(sensor_blocks):
                L = c.linearize(ha.HS_INERTIAL, True, sensor_blocks=sensor_blocks)
                f, fb = L["first_cp"][:, None], L["first_bias"][:, None]
                idx = np.concatenate([6 * f + np.arange(6 * k), 6 * n_cp + 3 * fb + np.arange(3 * kb), 6 * n_cp + 3 * n_bias + 3 * fb + np.arange(3 * kb),
                                      np.broadcast_to(6 * n_cp + 6 * n_bias + np.arange(2), (len(f), 2))], 1)
                J = np.concatenate([L["J_state"], L["J_bias_g"], L["J_bias_a"], L["J_gravity"]], 2) * free[idx][:, None, :]
                return L, idx, J

            if mode is not None:  # the base class took the state / gravity columns in the default mode: out with them, in with this mode's
                L, idx, J = inertial_rows(False)
                np.subtract.at(H, (idx[:, :, None], idx[:, None, :]), np.einsum("nri,nrj->nij", J, J))
                np.subtract.at(gx, idx, np.einsum("nri,nr->ni", J, L["r"]))
                c.set_inertial_jacobian(mode)
                L, idx, J = inertial_rows(True)
                np.add.at(H, (idx[:, :, None], idx[:, None, :]), np.einsum("nri,nrj->nij", J, J))
                np.add.at(gx, idx, np.einsum("nri,nr->ni", J, L["r"]))
            else:
                L, idx, J = inertial_rows(True)
            if ni:
                Ji = np.concatenate([L[key] for key in IMU_KEYS], 2)[:, :, imu_cols >= 0]  # (n, 6, ni): the free columns, in block order
                imu = P0 + np.arange(ni)
                cross = np.einsum("nri,nrj->nij", J, Ji)
                np.add.at(H, (idx[:, :, None], imu[None, None, :]), cross)
                np.add.at(H, (imu[None, :, None], idx[:, None, :]), cross.transpose(0, 2, 1))
                H[np.ix_(imu, imu)] += np.einsum("nri,nrj->ij", Ji, Ji)
                gx[imu] += np.einsum("nri,nr->i", Ji, L["r"])
        self.H, self.gx, self.Hxl, self.P = H, gx, Hxl, P
        self.active = np.diag(H) > 0.0

    def without_imu(self, v):
        """A vector over this system's columns without its IMU entries: the base class's column order."""
        return np.r_[v[:self.P0], v[self.P0 + self.ni:]]


def _plain_keep_cameras(w):
    w0 = copy.copy(w)
    w0.imu_constant = None
    return w0


def retract(w, sysm, dx, dl, oracle):
    """Candidate window Plus(x, delta), and (|x|^2 over the blocks in the program, |x+ - x|^2)."""
    base = copy.copy(sysm)  # the base class's view: its columns, without the IMU group
    base.P, base.active = sysm.P - sysm.ni, sysm.without_imu(sysm.active)
    c, xs, ss = csr.retract(_plain_keep_cameras(w), base, sysm.without_imu(dx), dl, oracle)
    c.imu_constant = w.imu_constant
    if sysm.ni:
        c.imu = dict(c.imu)
        di = dx[sysm.P0:sysm.P0 + sysm.ni]
        with ha.Problem(_plain(w), lib=oracle) as o:
            for b, (first, size) in enumerate(IMU_BLOCKS):
                cols = sysm.imu_cols[first:first + size]
                if cols[0] < 0:
                    continue
                x = np.array(w.imu[IMU_NAMES[b]], float).reshape(-1)
                y = o.manifold_plus(ha.HS_MANIFOLD_SE3, x[None, :], di[cols][None, :])[0] if b == 0 else x + di[cols]
                c.imu[IMU_NAMES[b]] = y
                xs += (x ** 2).sum()
                ss += ((y - x) ** 2).sum()
    return c, xs, ss


def cost_of(w, oracle):
    with ha.Problem(_plain(w), lib=oracle) as c:
        return c.cost()


def solve(w, oracle, max_iterations=5, radius=1e4, mode=None):
    """LM::run on window w (free IMU blocks per w.imu_constant, free camera blocks per w.cam_constant). Returns (summary in the layout of
    Problem.solve, final window). The loop of calibration_solve_referee.solve."""
    w = copy.deepcopy(w)
    sysm = System(w, oracle, mode)
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
        rec["imu_step"] = float(np.abs(dx[sysm.P0:sysm.P0 + sysm.ni]).max()) if sysm.ni else 0.0  # (not a summary field: the admission rules read it)
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
            sysm = System(w, oracle, mode)
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


def condition(w, oracle, radius=1e4, mode=None):
    """cond of the scaled, damped reduced system at the window's values."""
    sysm = System(w, oracle, mode)
    s, sl = sysm.scaling()
    return np.linalg.cond(np.asarray(sysm.scaled_system(s, sl, radius)[0], float))


# ---- window admission (tests/test_gpu_imu_calibration_solve.py, tests/test_gpu_imu_calibration_routes.py): rules evaluated from the referee alone ----

def constant_twin(w):
    """The same window with every sensor block constant."""
    w0 = copy.copy(w)
    w0.imu_constant = w0.cam_constant = None
    return w0


def rule_condition(w, oracle, mode=None):
    """(a) cond of the scaled, damped system with the blocks free is at most twice the cond with them constant. Returns (ok, free, constant)."""
    free, const = condition(w, oracle, mode=mode), condition(constant_twin(w), oracle, mode=mode)
    return free <= 2.0 * const, free, const


def rule_margin(summary):
    """(b) no iteration has a relative decrease within 1e-3 of the 1e-3 threshold (iterations that computed one)."""
    return all(abs(it["relative_decrease"] - 1e-3) > 1e-3 for it in summary["iterations"][1:] if it["step_is_valid"] and it["cost_change"] != 0.0)


def accepted_imu_steps(summary):
    return sum(1 for it in summary["iterations"][1:] if it["step_is_successful"] and it.get("imu_step", 0.0) > 0.0)


def rule_accepted(summary):
    """(c) at least two accepted steps that change the IMU parameters."""
    return accepted_imu_steps(summary) >= 2


def has_rejected_between_accepted(summary):
    """(d) a rejected step between accepted ones."""
    ok = [it["step_is_successful"] for it in summary["iterations"][1:]]
    return any(not ok[i] and any(ok[:i]) and any(ok[i + 1:]) for i in range(len(ok)))


def middle_third(w):
    """The window with inertial stamps over the middle third of its valid range only."""
    lo, hi = w.valid_range()
    keep = (w.inertial_stamps >= lo + (hi - lo) / 3) & (w.inertial_stamps < lo + 2 * (hi - lo) / 3)
    w.inertial_stamps, w.inertial_measurements = w.inertial_stamps[keep], w.inertial_measurements[keep]
    return w


def free_imu_windows():
    """(name, window with free IMU blocks, Jacobian mode or None, iterations) — the windows of the device parity tests. The iteration count is
    the referee's: enough for two accepted steps that move the IMU parameters, at most 10 (rules (b) and (c) are asserted by the tests)."""
    from hyperslam_amd import synthetic
    w = synthetic.small_inertial(order=4, n_cp=16)
    w.imu_constant = imu_flags("t")
    yield "k4_T_bs", w, None, 4
    for mode, tag, n in ((ha.HS_INERTIAL_AS_REFERENCE, "as_reference", 4), (ha.HS_INERTIAL_EXACT, "exact", 3)):
        w = synthetic.small_inertial(order=4, n_cp=16)
        w.imu_constant = imu_flags("tgasx")
        yield f"k4_all_free_{tag}", w, mode, n
    w = synthetic.small_inertial(order=5, n_cp=20)
    w.imu_constant = imu_flags("gx")
    yield "k5_i_g_X_a", w, None, 4
    w = synthetic.small_inertial(order=6, n_cp=20, seed=5)
    w.cp_constant = np.r_[np.ones(6, np.uint8), np.zeros(14, np.uint8)]
    w.imu = dict(w.imu, bias_constant=True)
    w.imu_constant = imu_flags("s")
    yield "k6_frozen_prefix_constant_bias_S_g", w, None, 5
    w = synthetic.small_inertial(order=4, n_cp=16, seed=9)
    w.gravity_constant = True
    w.imu_constant = imu_flags("ta")
    yield "constant_gravity_T_bs_i_a", w, None, 3
    w = middle_third(synthetic.small_inertial(order=4, n_cp=24, n_inertial=240, seed=6))
    w.imu_constant = imu_flags("t")
    yield "middle_third_T_bs", w, None, 3
    w = synthetic.small_inertial(order=4, n_cp=16, seed=4)
    w.imu_constant = imu_flags("t")
    w.cam_constant = csr.flags(w, cam1="i")  # (not a camera's T_bs next to the IMU's: the body frame would be a gauge freedom)
    yield "T_bs_and_camera1_intrinsics", w, None, 5
