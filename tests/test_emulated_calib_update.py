"""CPU test (no GPU): the update kernels of a window with free camera coordinates (Tables::nc > 0) — k_backsub_retract<true>,
k_update_visual<K, true>, k_calib_candidate, k_calib_commit — compiled from the product's kernel SOURCES for the host (tests/emul/) and
compared with numpy on fabricated landmark factors:
    y_l = L^-T (yh_l - Yh_l' (Sp o y_p) - Y_c,l y_c),  y_p = -step_p,  y_c = -dc,   candidate = lm - S_l o y_l   (DESIGN §13),
the decision terms (|x|^2, |x+ - x|^2, g.step, step'D^2 step) of the landmarks, the retraction of the free camera blocks with their norms, and
the (g_c - g_c,reduced) . dc share of the model cost change."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")


@pytest.fixture(scope="session")
def harness():
    exe = os.path.join(EMUL, "calib_update_harness")
    srcs = [os.path.join(EMUL, "calib_update_harness.cpp"), os.path.join(EMUL, "hip", "hip_runtime.h")]
    csrc = os.path.join(ROOT, "hyperslam_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-I", EMUL, "-o", exe, os.path.join(EMUL, "calib_update_harness.cpp")])
    return exe


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                     aw * bw - ax * bx - ay * by - az * bz])


def quat_plus(x, d):
    n = np.linalg.norm(d)
    return quat_mul(np.r_[np.sin(n) / n * d, np.cos(n)], x)


@pytest.mark.parametrize("k,free", [(4, {1: "tid"}), (5, {0: "id", 1: "id"}), (6, {0: "t", 1: "td"})])
def test_update_kernels_with_free_cameras(harness, k, free):
    rng = np.random.default_rng(100 + k)
    n_cp, bw, n_cam, per_group = 14, k + 2, 2, 5
    first, size = {"t": 0, "i": 6, "d": 10}, {"t": 6, "i": 4, "d": 4}
    calib_map = [c << 8 | (first[b] + j) for c in sorted(free) for b in "tid" if b in free[c] for j in range(size[b])]
    nc = len(calib_map)
    # landmarks grouped by first control point (a chunk = the landmarks of one group), the last two unobserved
    cfirst, ncp = [], []
    for cf in range(n_cp - k + 1):
        for _ in range(per_group):
            cfirst.append(cf)
            ncp.append(int(rng.integers(k, min(bw, n_cp - cf) + 1)))
    n_obs = len(cfirst)
    cfirst += [0, 0]
    ncp += [k, k]
    n_lm = len(cfirst)
    cfirst, ncp = np.array(cfirst, np.int32), np.array(ncp, np.int32)
    lm_ptr = np.r_[np.arange(n_obs + 1), [n_obs, n_obs]].astype(np.int32)
    lm_const = (np.arange(n_lm) % 7 == 3).astype(np.int32)
    yoff = np.r_[0, np.cumsum(18 * ncp)].astype(np.int32)
    Y = rng.standard_normal(yoff[-1] + 1)
    L = rng.standard_normal((n_lm, 6)) * 0.3
    L[:, [0, 2, 5]] = 1.0 + rng.random((n_lm, 3))  # [l00 l10 l11 l20 l21 l22]
    yhat, scale_l, sb, D2l = rng.standard_normal((n_lm, 3)), 0.1 + rng.random((n_lm, 3)), rng.standard_normal((n_lm, 3)), rng.random((n_lm, 3))
    lm = rng.standard_normal((n_lm, 3)) * 3
    cp = np.c_[rng.standard_normal((n_cp, 4)), rng.standard_normal((n_cp, 3)), np.arange(n_cp) * 0.1]
    cp[:, :4] /= np.linalg.norm(cp[:, :4], axis=1)[:, None]
    cam = np.zeros((n_cam, 16))
    cam[:, :4] = rng.standard_normal((n_cam, 4))
    cam[:, :4] /= np.linalg.norm(cam[:, :4], axis=1)[:, None]
    cam[:, 4:15] = np.c_[rng.standard_normal((n_cam, 3)) * 0.1, 300 + 100 * rng.random((n_cam, 4)), rng.standard_normal((n_cam, 4)) * 0.01]
    step_p, scale_p, D2p = 1e-2 * rng.standard_normal(6 * n_cp), 0.1 + rng.random(6 * n_cp), rng.random(6 * n_cp)
    dc, D2b = 1e-2 * rng.standard_normal(nc), rng.random(nc)
    Yc = rng.standard_normal((n_lm, 3, nc))
    g_full, g_red = rng.standard_normal(nc), rng.standard_normal(nc)
    desc = []
    for cf in range(n_cp - k + 1):
        desc += [cf * per_group, per_group, cf, 0, 0, 0, 0, 0]  # first landmark, landmarks, first control point, first residual, residuals
    n_chunk = len(desc) // 8
    f64, i32 = np.float64, np.int32
    parts = [np.array([k, n_cp, n_lm, bw, nc, 0, n_chunk, n_cam], i32), cp, cam, lm, lm_const, lm_ptr, cfirst, ncp, yoff, Y, L, yhat, scale_l, sb, D2l, step_p, scale_p,
             D2p, dc, D2b, Yc, g_full, g_red, np.array(calib_map, i32), np.array(desc, i32)]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            for a in parts:
                a = np.ascontiguousarray(a)
                f.write(a.astype(i32 if a.dtype.kind == "i" else f64).tobytes())
        subprocess.check_call([harness, fin, fout], timeout=600)
        raw = np.fromfile(fout, f64)
    lm_a, lm_b = raw[:3 * n_lm].reshape(n_lm, 3), raw[3 * n_lm:6 * n_lm].reshape(n_lm, 3)
    off = 6 * n_lm
    sums_a, sums_b = raw[off:off + 4], raw[off + 4:off + 8]
    off += 8
    cam_cand, cam_acc, cam_rej = (raw[off + i * 16 * n_cam:off + (i + 1) * 16 * n_cam].reshape(n_cam, 16) for i in range(3))
    xs_c, ss_c, g_corr = raw[off + 48 * n_cam:off + 48 * n_cam + 3]

    # numpy
    want = lm.copy()
    terms = np.zeros(4)
    for l in range(n_lm):
        observed = lm_ptr[l + 1] > lm_ptr[l]
        if not observed or lm_const[l]:
            continue
        rows = slice(6 * cfirst[l], 6 * (cfirst[l] + ncp[l]))
        Yh = Y[yoff[l]:yoff[l] + 18 * ncp[l]].reshape(6 * ncp[l], 3)
        y_p, y_c = -(step_p * scale_p)[rows], -dc
        z = yhat[l] - Yh.T @ y_p - Yc[l] @ y_c
        Lm = np.array([[L[l, 0], 0, 0], [L[l, 1], L[l, 2], 0], [L[l, 3], L[l, 4], L[l, 5]]])
        s = -np.linalg.solve(Lm.T, z)
        want[l] = lm[l] + scale_l[l] * s
        terms += [lm[l] @ lm[l], ((want[l] - lm[l]) ** 2).sum(), sb[l] @ s, (D2l[l] * s) @ s]
        without = -np.linalg.solve(Lm.T, yhat[l] - Yh.T @ y_p)
        assert np.abs(s - without).max() > 1e-6  # (the camera term matters in this case)
    assert np.abs(lm_a - want).max() <= 1e-12 * np.abs(want).max(), np.abs(lm_a - want).max()
    assert np.abs(lm_b[:n_obs] - want[:n_obs]).max() <= 1e-12 * np.abs(want).max(), np.abs(lm_b[:n_obs] - want[:n_obs]).max()
    assert np.array_equal(lm_b[n_obs:], lm[n_obs:])  # (unobserved landmarks: the fused path's norm workgroups copy them)
    assert np.abs(sums_a - terms).max() <= 1e-12 * np.abs(terms).max(), (sums_a, terms)
    assert np.abs(sums_b - terms).max() <= 1e-12 * np.abs(terms).max(), (sums_b, terms)

    want_cam, xs, ss = cam.copy(), 0.0, 0.0
    for j, m in enumerate(calib_map):
        c, col = m >> 8, m & 0xff
        if col == 0:
            want_cam[c, :4] = quat_plus(cam[c, :4], dc[j:j + 3])
            want_cam[c, 4:7] = cam[c, 4:7] + dc[j + 3:j + 6]
            xs += (cam[c, :7] ** 2).sum()
            ss += ((want_cam[c, :7] - cam[c, :7]) ** 2).sum()
        elif col >= 6:
            want_cam[c, 1 + col] = cam[c, 1 + col] + dc[j]
            xs += cam[c, 1 + col] ** 2
            ss += dc[j] ** 2
    assert np.abs(cam_cand - want_cam).max() <= 1e-13 * np.abs(want_cam).max()
    const_entries = np.ones((n_cam, 16), bool)
    for m in calib_map:
        if (m & 0xff) == 0:
            const_entries[m >> 8, 0:7] = False
        elif (m & 0xff) >= 6:
            const_entries[m >> 8, 1 + (m & 0xff)] = False
    assert np.array_equal(cam_cand[const_entries], cam[const_entries])  # constant blocks and cameras are copied
    assert abs(xs_c - xs) <= 1e-12 * xs and abs(ss_c - ss) <= 1e-9 * ss, (xs_c, xs, ss_c, ss)
    assert abs(g_corr - (g_full - g_red) @ dc) <= 1e-12 * np.abs(g_full - g_red) @ np.abs(dc)
    assert np.array_equal(cam_acc, cam_cand) and np.array_equal(cam_rej, cam)
