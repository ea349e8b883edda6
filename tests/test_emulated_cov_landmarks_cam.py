"""CPU test (no GPU): the landmark blocks of the covariance with free camera coordinates (hyperslam_amd/csrc/kernels_covariance.hpp:
k_cov_landmarks_cam), compiled from the product's kernel SOURCE for the host (tests/emul/: one thread per lane) and compared with numpy on
fabricated inputs — an SPD Sigma over [control points | border], random landmark factors L, Yh, Y_c and scales:
    Sigma_ll = S_l L^-T (I + G' Sigma_[p_l,c] G) L^-1 S_l,   G = [Yh ; Y_c']   (DESIGN §12),
for landmarks on 1, 4, 11 and 42 control points (one, several and the most rows of G a lane owns), 1 .. 64 camera columns behind 0 or 44
bias / gravity columns, constant and unobserved landmarks, and rank-deficient landmark factors. Bar: 1e-12 relative to each block's
max-norm — the inputs are well conditioned (Sigma = I + A A' / n, the diagonal of L in [0.5, 1.5]) and every term of G' Sigma G's diagonal
is positive, so the 316-term sums lose a few hundred ulps at most."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")

N_L = (1, 4, 11, 42)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("emul_cov_cam") / "cov_landmarks_cam_harness")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-Wno-psabi", "-I", EMUL, "-o", exe, os.path.join(EMUL, "cov_landmarks_cam_harness.cpp")])
    return exe


def band_rows(M, n, bw):
    ncb = 6 * bw
    B = np.zeros((n, ncb))
    for r in range(n):
        c0 = 6 * (r // 6)
        w = min(ncb, n - c0)
        B[r, :w] = M[r, c0:c0 + w]
    return B


def case(seed, nc, nbi, bw=42, n_cp=45):
    """Landmarks on every width of N_L (twice, at both ends of the window), then: a constant one, an unobserved one, and two whose factor is rank
    deficient (a pivot below 1e-12 of its row; a zero pivot)."""
    rng = np.random.default_rng(seed)
    n, nb = 6 * n_cp, nbi + nc
    A = rng.standard_normal((n + nb, n + nb))
    Sigma = np.eye(n + nb) + A @ A.T / (n + nb)
    ncp = np.array(list(N_L) + list(N_L) + [4, 4, 4, 4, 7], np.int32)
    n_lm = len(ncp)
    cfirst = np.array([0] * len(N_L) + [n_cp - m for m in N_L] + [3, 5, 6, 7, 20], np.int32)
    const = np.zeros(n_lm, np.int32)
    const[8] = 1
    observed = np.ones(n_lm, bool)
    observed[9] = False
    lm_ptr = np.r_[0, np.cumsum(np.where(observed, 2, 0))].astype(np.int32)
    yoff = np.r_[0, np.cumsum(18 * ncp)].astype(np.int32)
    Y = rng.standard_normal(yoff[-1])
    Yc = rng.standard_normal((n_lm, 3, nc))
    L = rng.standard_normal((n_lm, 6)) * 0.3
    L[:, [0, 2, 5]] = rng.uniform(0.5, 1.5, (n_lm, 3))
    L[10, 5] = 1e-7 * np.linalg.norm(L[10, 3:5])  # l22^2 = 1e-14 (l20^2 + l21^2): below kCovPivotTol of its row
    L[11, 0] = 0.0
    scale = rng.uniform(0.2, 2.0, (n_lm, 3))
    return dict(n_lm=n_lm, bw=bw, nc=nc, nbi=nbi, n=n, Sigma=Sigma, ncp=ncp, cfirst=cfirst, const=const, observed=observed, lm_ptr=lm_ptr, yoff=yoff,
                Y=Y, Yc=Yc, L=L, scale=scale, deficient=[10, 11])


def run(exe, tmp_path, c):
    n, nb = c["n"], c["nbi"] + c["nc"]
    S = c["Sigma"]
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("8i", c["n_lm"], c["bw"], c["nc"], c["nbi"], n, 0, 0, 0))
        for a in (c["const"], c["lm_ptr"], c["cfirst"], c["ncp"], c["yoff"]):
            f.write(np.ascontiguousarray(a, np.int32).tobytes())
        for a in (c["Y"], c["Yc"], c["L"], c["scale"], band_rows(S, n, c["bw"]), S[:n, n:], S[n:, n:]):
            f.write(np.ascontiguousarray(a, np.float64).tobytes())
    subprocess.check_call([exe, src, dst], timeout=600)
    raw = open(dst, "rb").read()
    status = np.frombuffer(raw[:4 * c["n_lm"]], np.int32)
    out = np.frombuffer(raw[4 * c["n_lm"]:], np.float64).reshape(c["n_lm"], 3, 3)
    assert nb == S.shape[0] - n
    return status, out


def reference(c, l):
    n, nbi, nc = c["n"], c["nbi"], c["nc"]
    rows = 6 * c["ncp"][l]
    idx = np.r_[6 * c["cfirst"][l] + np.arange(rows), n + nbi + np.arange(nc)]
    G = np.r_[c["Y"][c["yoff"][l]:c["yoff"][l + 1]].reshape(rows, 3), c["Yc"][l].T]
    l00, l10, l11, l20, l21, l22 = c["L"][l]
    N = np.linalg.inv(np.array([[l00, 0, 0], [l10, l11, 0], [l20, l21, l22]]))
    s = c["scale"][l]
    return s[:, None] * (N.T @ (np.eye(3) + G.T @ c["Sigma"][np.ix_(idx, idx)] @ G) @ N) * s[None, :]


@pytest.mark.parametrize("nbi", [0, 44])
@pytest.mark.parametrize("nc", [1, 6, 14, 28, 64])
def test_landmark_blocks_with_camera_columns(nc, nbi, harness, tmp_path):
    c = case(1000 * nc + nbi, nc, nbi)
    assert set(N_L) <= set(c["ncp"].tolist())
    status, out = run(harness, tmp_path, c)
    for l in range(c["n_lm"]):
        if not c["observed"][l]:
            assert status[l] == 0 and np.isnan(out[l]).all(), l
        elif c["const"][l]:
            assert status[l] == 0 and not out[l].any(), l
        elif l in c["deficient"]:
            assert status[l] == 1 and np.isnan(out[l]).all(), l
        else:
            want = reference(c, l)
            err = np.abs(out[l] - want).max() / np.abs(want).max()
            assert status[l] == 0 and err < 1e-12, (l, int(c["ncp"][l]), err)


def test_without_camera_term_equals_the_pose_formula(harness, tmp_path):
    """Y_c = 0: the block is S_l L^-T (I + Yh' Sigma_pp Yh) L^-1 S_l, whatever Sigma_pb and Sigma_bb hold."""
    c = case(5, 14, 44)
    c["Yc"][:] = 0.0
    status, out = run(harness, tmp_path, c)
    for l in range(8):
        rows = 6 * c["ncp"][l]
        idx = 6 * c["cfirst"][l] + np.arange(rows)
        Yh = c["Y"][c["yoff"][l]:c["yoff"][l + 1]].reshape(rows, 3)
        l00, l10, l11, l20, l21, l22 = c["L"][l]
        N = np.linalg.inv(np.array([[l00, 0, 0], [l10, l11, 0], [l20, l21, l22]]))
        s = c["scale"][l]
        want = s[:, None] * (N.T @ (np.eye(3) + Yh.T @ c["Sigma"][np.ix_(idx, idx)] @ Yh) @ N) * s[None, :]
        assert np.abs(out[l] - want).max() / np.abs(want).max() < 1e-12, l


def test_two_runs_bit_identical(harness, tmp_path):
    c = case(6, 28, 44)
    a, b = run(harness, tmp_path, c), run(harness, tmp_path, c)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)
