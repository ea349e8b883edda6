"""Numpy referee of the pixel residual under a per-camera distortion model (hs_set_camera_models).

The oracle knows the radial-tangential model alone and cannot learn another, so the referee is the oracle's PINHOLE chain plus the numpy
maps below. An oracle Problem on the same window with intrinsics [0, 0, 1, 1], zero distortion, zero pixels and robustify=False returns
r = n, the plane point ProjectToPlane(p_s), and dn / d(state, landmark, extrinsics). On top of it the referee composes
    r = c + f * d(n) - pixel,   J_x = diag(f) dd/dn dn/dx,   J_intrinsics = [I | diag(d)],   J_distortion = diag(f) dd/dk,
and the Huber corrector of the pixel factor (a = 0.5; rho'' <= 0, so Ceres' corrector scales rows and Jacobians by sqrt(rho')).
d is `radtan_map` (the formulas of the oracle, restated) or `equidistant_map`, row by row after the camera's model.

The seam to the existing referees (calibration_referee.reduced_system, calibration_solve_referee.solve, camera_covariance_referee.referee,
..): they take an oracle library and open `ha.Problem(window, lib=oracle)` on it, of which they call linearize, cost, num_residuals, dim_pose
and manifold_plus only. `RefereeProblem` is a Problem bound to the oracle that overrides the pixel rows and the cost; inside `with driving():`
the name ha.Problem builds one whenever the library is not the product's, so every existing referee then referees a window with
Window.cam_models unchanged. Product handles (lib = the HIP library, or none given) are built as ever."""
import contextlib
import copy

import numpy as np

import hyperslam_amd as ha

_Base = ha.Problem
HUBER_PIXEL = 0.5  # optimizer.cpp:226


def radtan_map(n, k):
    """d (N, 2), dd/dn (N, 2, 2), dd/dk (N, 2, 4) of the radial-tangential model [k1 k2 p1 p2] at the plane points n (N, 2)."""
    x, y = n[:, 0], n[:, 1]
    k1, k2, p1, p2 = k[:, 0], k[:, 1], k[:, 2], k[:, 3]
    r2 = x * x + y * y
    r4 = r2 * r2
    rad = 1 + k1 * r2 + k2 * r4
    d = np.stack([x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y], -1)
    drx, dry = 2 * k1 * x + 4 * k2 * r2 * x, 2 * k1 * y + 4 * k2 * r2 * y
    D = np.empty((len(n), 2, 2))
    D[:, 0, 0], D[:, 0, 1] = rad + x * drx + 2 * p1 * y + 6 * p2 * x, x * dry + 2 * p1 * x + 2 * p2 * y
    D[:, 1, 0], D[:, 1, 1] = y * drx + 2 * p1 * x + 2 * p2 * y, rad + y * dry + 6 * p1 * y + 2 * p2 * x
    Dk = np.empty((len(n), 2, 4))
    Dk[:, 0] = np.stack([x * r2, x * r4, 2 * x * y, r2 + 2 * x * x], -1)
    Dk[:, 1] = np.stack([y * r2, y * r4, r2 + 2 * y * y, 2 * x * y], -1)
    return d, D, Dk


def equidistant_map(n, k):
    """d = c n, dd/dn = c I + e n n', dd/dk_i = theta^(2i+1) / rho n of the equidistant model [k1 k2 k3 k4]; at rho = 0:
    c = 1, e = 0, dd/dk = 0."""
    x, y = n[:, 0], n[:, 1]
    rho2 = x * x + y * y
    rho = np.sqrt(rho2)
    zero = rho == 0
    rs, rs2 = np.where(zero, 1.0, rho), np.where(zero, 1.0, rho2)
    theta = np.arctan(rho)
    t = theta * theta
    s = theta * (1 + k[:, 0] * t + k[:, 1] * t ** 2 + k[:, 2] * t ** 3 + k[:, 3] * t ** 4)
    sp = 1 + 3 * k[:, 0] * t + 5 * k[:, 1] * t ** 2 + 7 * k[:, 2] * t ** 3 + 9 * k[:, 3] * t ** 4
    c = np.where(zero, 1.0, s / rs)
    e = np.where(zero, 0.0, (sp / (1 + rho2) - c) / rs2)
    d = c[:, None] * n
    D = c[:, None, None] * np.eye(2)[None] + e[:, None, None] * n[:, :, None] * n[:, None, :]
    pw = np.stack([theta ** 3, theta ** 5, theta ** 7, theta ** 9], -1) / rs[:, None]  # (N, 4); theta = 0 at rho = 0
    Dk = n[:, :, None] * pw[:, None, :]
    return d, D, Dk


def mp_equidistant(x, y, k):
    """(d, dd/dn, dd/dk) of the equidistant model at 50 digits, by mpmath's own differentiation of d(n) = s(atan |n|) n / |n|."""
    import mpmath as mp
    mp.mp.dps = 50
    x, y, k = mp.mpf(x), mp.mpf(y), [mp.mpf(v) for v in k]

    def d(xx, yy, kk=k):
        rho = mp.sqrt(xx * xx + yy * yy)
        if rho == 0:
            return xx, yy
        th = mp.atan(rho)
        s = th * (1 + sum(kk[i] * th ** (2 * i + 2) for i in range(4)))
        return s / rho * xx, s / rho * yy

    if x == 0 and y == 0:
        return (mp.mpf(0), mp.mpf(0)), [[1, 0], [0, 1]], [[0] * 4, [0] * 4]
    val = d(x, y)
    D = [[mp.diff(lambda a, c=c: d(a, y)[c], x), mp.diff(lambda b, c=c: d(x, b)[c], y)] for c in range(2)]
    Dk = [[mp.diff(lambda v, c=c, i=i: d(x, y, k[:i] + [v] + k[i + 1:])[c], k[i]) for i in range(4)] for c in range(2)]
    return val, D, Dk


def mp_equidistant_bearing(u, v, k):
    """Unit bearing of the distorted plane point (u, v) under the equidistant model at 50 digits: the root of s(theta) = |(u, v)|."""
    import mpmath as mp
    mp.mp.dps = 50
    u, v, k = mp.mpf(u), mp.mpf(v), [mp.mpf(x) for x in k]
    rho_d = mp.sqrt(u * u + v * v)
    if rho_d == 0:
        return mp.mpf(0), mp.mpf(0), mp.mpf(1)
    theta = mp.findroot(lambda th: th * (1 + sum(k[i] * th ** (2 * i + 2) for i in range(4))) - rho_d, rho_d)
    return mp.sin(theta) * u / rho_d, mp.sin(theta) * v / rho_d, mp.cos(theta)


def equidistant_bearing(nd, k):
    """Numpy inverse of the equidistant model: unit bearings (N, 3) of the distorted plane points nd (N, 2); Newton on s(theta) = |nd| from
    theta = |nd| until the step is below one ulp (at most 50 steps); the optical axis at |nd| = 0."""
    rho_d = np.hypot(nd[:, 0], nd[:, 1])
    theta = rho_d.copy()
    for _ in range(50):
        t = theta * theta
        s = theta * (1 + k[:, 0] * t + k[:, 1] * t ** 2 + k[:, 2] * t ** 3 + k[:, 3] * t ** 4)
        sp = 1 + 3 * k[:, 0] * t + 5 * k[:, 1] * t ** 2 + 7 * k[:, 2] * t ** 3 + 9 * k[:, 3] * t ** 4
        step = (s - rho_d) / sp
        theta = theta - step
        if np.abs(step).max() <= 1e-17:
            break
    zero = rho_d == 0
    w = np.where(zero, 0.0, np.sin(theta) / np.where(zero, 1.0, rho_d))
    return np.stack([w * nd[:, 0], w * nd[:, 1], np.where(zero, 1.0, np.cos(theta))], -1)


def radtan_bearing(nd, k):
    """Unit bearings of the distorted plane points nd under the radial-tangential model: twenty steps of the fixed-point iteration
    n <- (nd - tangential(n)) / radial(n), then normalised — what hs_process_tracks has always done."""
    x, y = nd[:, 0].copy(), nd[:, 1].copy()
    for _ in range(20):
        r2 = x * x + y * y
        rad = 1 + k[:, 0] * r2 + k[:, 1] * r2 * r2
        dx, dy = 2 * k[:, 2] * x * y + k[:, 3] * (r2 + 2 * x * x), k[:, 2] * (r2 + 2 * y * y) + 2 * k[:, 3] * x * y
        x, y = (nd[:, 0] - dx) / rad, (nd[:, 1] - dy) / rad
    nrm = np.sqrt(x * x + y * y + 1)
    return np.stack([x / nrm, y / nrm, 1 / nrm], -1)


def distort(n, k, model):
    """Row i through the map of model[i] (0: radial-tangential, 1: equidistant)."""
    eq = (np.asarray(model) != 0)
    a, b = radtan_map(n, k), equidistant_map(n, k)
    return tuple(np.where(eq.reshape((-1,) + (1,) * (x.ndim - 1)), y, x) for x, y in zip(a, b))


def huber(s, a=HUBER_PIXEL):
    """(rho(s), sqrt(rho'(s))) of Ceres' HuberLoss(a) at s = |r|^2."""
    out = s > a * a
    root = np.sqrt(np.where(out, s, 1.0))
    return np.where(out, 2 * a * root - a * a, s), np.where(out, np.sqrt(a / root), 1.0)


def models_of(w):
    n = len(np.asarray(w.cam_T_bs, float).reshape(-1, 7))
    return np.zeros(n, np.int32) if w.cam_models is None else np.asarray(w.cam_models, np.int32).reshape(n)


class RefereeProblem(_Base):
    """The oracle on window w, with the pixel rows and the cost of the window's camera models (module docstring)."""

    def __init__(self, window, lib, **kw):
        self._plane = self._rest = None
        super().__init__(window, lib=lib, **kw)

    def close(self):
        for p in (getattr(self, "_plane", None), getattr(self, "_rest", None)):
            if p is not None:
                p.close()
        self._plane = self._rest = None
        super().close()

    def upload(self, w):
        plain = copy.copy(w)
        plain.cam_models = plain.cam_constant = plain.imu_constant = None  # (the oracle is asked for nothing it does not know: no model, every sensor block constant)
        super().upload(plain)
        self.window = w
        for p in (self._plane, self._rest):
            if p is not None:
                p.close()
        n_cam, n_px = len(np.asarray(w.cam_T_bs).reshape(-1, 7)), len(w.pixel_stamps)
        empty = dict(bearing_stamps=np.zeros(0), bearings=np.zeros((0, 3)), bearing_landmark=np.zeros(0, np.int32), bearing_camera=np.zeros(0, np.int32),
                     prior_stamps=np.zeros(0), prior_poses=np.zeros((0, 7)), prior_sensor=np.zeros(0, np.int32), inertial_stamps=np.zeros(0),
                     inertial_measurements=np.zeros((0, 6)))
        plane = copy.copy(plain)
        plane.cam_constant, plane.imu, plane.imu_constant = None, None, None
        plane.cam_intrinsics, plane.cam_distortion = np.tile([0.0, 0.0, 1.0, 1.0], (n_cam, 1)), np.zeros((n_cam, 4))
        plane.pixels = np.zeros((n_px, 2))
        for key, v in empty.items():
            setattr(plane, key, v)
        self._plane = _Base(plane, lib=self.lib) if n_px else None
        rest = copy.copy(plain)
        rest.cam_constant, rest.imu_constant = None, None
        rest.pixel_stamps, rest.pixels = np.zeros(0), np.zeros((0, 2))
        rest.pixel_landmark, rest.pixel_camera = np.zeros(0, np.int32), np.zeros(0, np.int32)
        self._rest = _Base(rest, lib=self.lib) if rest.num_residual_blocks() else None

    def linearize(self, ftype, robustify=True, sensor_blocks=False):
        if ftype != ha.HS_PIXEL or self._plane is None:
            return super().linearize(ftype, robustify, sensor_blocks)
        w = self.window
        P = self._plane.linearize(ha.HS_PIXEL, robustify=False, sensor_blocks=True)
        cam = np.asarray(w.pixel_camera, int)
        intr = np.asarray(w.cam_intrinsics, float).reshape(-1, 4)[cam]
        k = np.asarray(w.cam_distortion, float).reshape(-1, 4)[cam]
        d, D, Dk = distort(P["r"], k, models_of(w)[cam])
        f = intr[:, 2:4]
        r = intr[:, 0:2] + f * d - np.asarray(w.pixels, float).reshape(-1, 2)
        A = f[:, :, None] * D
        rho, sr = huber((r * r).sum(1))
        if not robustify:
            sr = np.ones_like(sr)
        out = dict(r=sr[:, None] * r, first_cp=P["first_cp"], cost=0.5 * rho)
        for key in ("J_state", "J_landmark") + (("J_extrinsics",) if sensor_blocks else ()):
            out[key] = sr[:, None, None] * (A @ P[key])
        if sensor_blocks:
            Ji = np.zeros((len(r), 2, 4))
            Ji[:, 0, 0], Ji[:, 1, 1], Ji[:, 0, 2], Ji[:, 1, 3] = 1.0, 1.0, d[:, 0], d[:, 1]
            out["J_intrinsics"], out["J_distortion"] = sr[:, None, None] * Ji, sr[:, None, None] * (f[:, :, None] * Dk)
        return out

    def cost(self):
        total = self._rest.cost() if self._rest is not None else 0.0
        if self._plane is not None:
            total += float(self.linearize(ha.HS_PIXEL, robustify=False)["cost"].sum())
        return total


def _factory(window, lib=None, **kw):
    if lib is None or lib.prefix == "hs_":
        return _Base(window, lib=lib, **kw)
    return RefereeProblem(window, lib, **kw)


@contextlib.contextmanager
def driving():
    """Inside: ha.Problem(window, lib=oracle) is the referee of the window's camera models (the seam of the module docstring)."""
    ha.Problem = _factory
    try:
        yield
    finally:
        ha.Problem = _Base
