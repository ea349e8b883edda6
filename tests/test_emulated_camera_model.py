"""CPU tests (no GPU): the product's projection code under both distortion models — visual_measure (csrc/factors.hpp), the intrinsics and
distortion blocks of visual_sensor_jacobians (csrc/kernels_sensor.hpp) and pixel_to_bearing (csrc/kernels_aux.hpp) — compiled from the
product's SOURCES for the host (tests/emul/camera_model_harness.cpp) and run with unit intrinsics.

Equidistant side: against mpmath at 50 digits, absolute 1e-13, on the points of tests/test_camera_model_referee.py (plane radius 0 .. 3, four
angles) and, for the inverse, on distorted radii {0, 0.1, 0.7, 1.3}. Radial-tangential side: equal to the numpy restatement of the formulas
the product has always had (and, for the inverse, to twenty steps of the fixed-point iteration)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import camera_model_referee as cmr
import camera_model_windows as cw
from test_camera_model_referee import ANGLES, equidistant_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
K_EQ, K_RT = cw.EQUI_DISTORTION[0], np.array([-0.28340811, 0.07395907, 1.76187114e-05, 0.00019359])
RHO_D = (0.0, 0.1, 0.7, 1.3)


@pytest.fixture(scope="module")
def harness():
    exe = os.path.join(EMUL, "camera_model_harness")
    srcs = [os.path.join(EMUL, "camera_model_harness.cpp"), os.path.join(EMUL, "hip", "hip_runtime.h")]
    csrc = os.path.join(ROOT, "hyperslam_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-I", EMUL, "-o", exe, os.path.join(EMUL, "camera_model_harness.cpp")])
    return exe


def run(exe, model, points, pixels, k):
    """(r (n, 2), Jps (n, 2, 3), J_intrinsics (n, 2, 4), J_distortion (n, 2, 4), bearings (m, 3)) of the product's code."""
    line = lambda p: "%d %s\n" % (model, " ".join(repr(float(v)) for v in (*p, *k)))
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as f:
            f.write("%d\n" % len(points) + "".join(line(p) for p in points) + "%d\n" % len(pixels) + "".join(line(p) for p in pixels))
        subprocess.check_call([exe, fin, fout], timeout=120)
        rows = [np.array(l.split(), float) for l in open(fout)]
    fwd = np.array(rows[:len(points)]).reshape(len(points), 24)
    return fwd[:, 0:2], fwd[:, 2:8].reshape(-1, 2, 3), fwd[:, 8:16].reshape(-1, 2, 4), fwd[:, 16:24].reshape(-1, 2, 4), np.array(rows[len(points):]).reshape(-1, 3)


def test_equidistant_against_mpmath(harness):
    n = equidistant_points()
    nd = equidistant_points(RHO_D)
    r, Jps, Ji, Jd, b = run(harness, cw.EQUI, n, nd, K_EQ)
    assert all(np.isfinite(a).all() for a in (r, Jps, Ji, Jd, b))
    worst = dict(d=0.0, D=0.0, Dk=0.0, Ji=0.0, bearing=0.0)
    for i, (x, y) in enumerate(n):
        d, D, Dk = cmr.mp_equidistant(x, y, K_EQ)
        worst["d"] = max(worst["d"], *(abs(float(r[i, c] - d[c])) for c in range(2)))
        # p_s = (x, y, 1): d r / d p_s = [dd/dn | -dd/dn n]
        worst["D"] = max(worst["D"], *(abs(float(Jps[i, c, j] - D[c][j])) for c in range(2) for j in range(2)),
                         *(abs(float(Jps[i, c, 2] + D[c][0] * x + D[c][1] * y)) for c in range(2)))
        worst["Dk"] = max(worst["Dk"], *(abs(float(Jd[i, c, j] - Dk[c][j])) for c in range(2) for j in range(4)))
        want = [[1, 0, d[0], 0], [0, 1, 0, d[1]]]
        worst["Ji"] = max(worst["Ji"], *(abs(float(Ji[i, c, j] - want[c][j])) for c in range(2) for j in range(4)))
    for i, (u, v) in enumerate(nd):
        ref = cmr.mp_equidistant_bearing(u, v, K_EQ)
        worst["bearing"] = max(worst["bearing"], *(abs(float(b[i, c] - ref[c])) for c in range(3)))
    print("product sources against mpmath, worst absolute errors:", worst)
    assert max(worst.values()) <= 1e-13, worst
    assert np.array_equal(b[:len(ANGLES)], np.tile([0.0, 0.0, 1.0], (len(ANGLES), 1)))  # rho_d = 0 would be x = y = 0: the axis itself


def test_equidistant_on_the_axis_is_exact(harness):
    r, Jps, Ji, Jd, b = run(harness, cw.EQUI, [(0.0, 0.0)], [(0.0, 0.0)], K_EQ)
    assert np.array_equal(r[0], [0.0, 0.0]) and np.array_equal(Jps[0], [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.array_equal(Jd[0], np.zeros((2, 4))) and np.array_equal(Ji[0], [[1.0, 0, 0, 0], [0, 1.0, 0, 0]])
    assert np.array_equal(b[0], [0.0, 0.0, 1.0])


def test_radtan_is_the_formulas_it_has_always_been(harness):
    n = equidistant_points((0.0, 1e-6, 1e-3, 0.1, 0.5, 1.0))
    k = np.tile(K_RT, (len(n), 1))
    r, Jps, Ji, Jd, b = run(harness, cw.RADTAN, n, n, K_RT)
    d, D, Dk = cmr.radtan_map(n, k)
    eps = 4 * np.finfo(float).eps
    assert np.abs(r - d).max() <= eps * max(1.0, np.abs(d).max())
    assert np.abs(Jps[:, :, :2] - D).max() <= eps * np.abs(D).max()
    assert np.abs(Jps[:, :, 2] + np.einsum("nij,nj->ni", D, n)).max() <= eps * np.abs(D).max()
    assert np.abs(Jd - Dk).max() <= eps * max(1.0, np.abs(Dk).max())
    want = np.zeros((len(n), 2, 4))
    want[:, 0, 0], want[:, 1, 1], want[:, 0, 2], want[:, 1, 3] = 1.0, 1.0, d[:, 0], d[:, 1]
    assert np.abs(Ji - want).max() <= eps * max(1.0, np.abs(d).max())
    assert np.abs(b - cmr.radtan_bearing(n, k)).max() <= eps  # the inverse: twenty steps of the fixed-point iteration, then normalised
