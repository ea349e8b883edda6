"""The selected inverse behind hs_compute_covariance (hyperslam_amd/csrc/kernels_covariance.hpp: k_cov_band — band Cholesky, Takahashi
recurrence, border Schur complement — and k_cov_finish) compiled from the product's source for the HOST (tests/emul/: one thread per lane)
and checked against numpy.linalg.inv restricted to the band: every band width from 1 to 42, with and without a frozen prefix of constant
control points, border widths 0 / 14 / 45, the LDS path (6 bw <= 128) and the global-memory path. A free coordinate without information is
reported, not inverted."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
LDS_MAX_BW = 128 // 6


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emul_cov") / "covariance_harness")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-Wno-psabi", "-I", EMUL, "-o", exe, os.path.join(EMUL, "covariance_harness.cpp")])
    return exe


def system(rng, n_blk, bw, nb, f0):
    """A Jacobi-scaled reduced system as the build writes it with zero damping: block band of half-width bw, border columns, every diagonal
    entry below 1; the f0 leading control points constant (decoupled rows, 1.0 on the diagonal)."""
    n = 6 * n_blk
    M = np.zeros((n + nb, n + nb))
    for s in range(f0, n_blk):
        e = min(s + bw, n_blk)
        J = rng.standard_normal((3 * (e - s) + 2, 6 * (e - s)))
        M[6 * s:6 * e, 6 * s:6 * e] += J.T @ J
    for _ in range(2 * nb):  # border rows (inertial factors): one window of control points and every border column
        s = int(rng.integers(f0, n_blk))
        e = min(s + bw, n_blk)
        row = np.zeros(n + nb)
        row[6 * s:6 * e] = rng.standard_normal(6 * (e - s))
        row[n:] = rng.standard_normal(nb)
        M += 0.3 * np.outer(row, row)
    free = np.ones(n + nb, bool)
    free[:6 * f0] = False
    idx = np.flatnonzero(free)
    M[idx, idx] += rng.uniform(0.5, 1.5, idx.size)
    d = np.sqrt(np.diag(M))
    d[d == 0.0] = 1.0
    M = M / d[:, None] / d[None, :] * 0.8  # scaled diagonal 0.8 < 1
    for r in range(6 * f0):
        M[r, :] = M[:, r] = 0.0
        M[r, r] = 1.0
    return M, free


def band_rows(M, n, bw):
    ncb = 6 * bw
    B = np.zeros((n, ncb))
    for r in range(n):
        c0 = 6 * (r // 6)
        w = min(ncb, n - c0)
        B[r, :w] = M[r, c0:c0 + w]
    return B


def run(exe, tmp_path, M, n, bw, nb, free, lds, scale=None):
    scale = np.ones(n + nb) if scale is None else scale
    src, dst = str(tmp_path / "sys.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("6i", n, bw, nb, int(lds), 0, 0))
        f.write(np.ascontiguousarray(band_rows(M, n, bw)).tobytes())
        f.write(np.ascontiguousarray(M[:n, n:]).tobytes())
        f.write(np.ascontiguousarray(M[n:, n:]).tobytes())
        f.write(scale[:n].tobytes())
        f.write(scale[n:].tobytes())
        f.write((~free).astype(np.int32).tobytes())
    subprocess.check_call([exe, src, dst], timeout=600)
    raw = open(dst, "rb").read()
    status = struct.unpack("4i", raw[:16])[0]
    v = np.frombuffer(raw[16:], dtype=np.float64)
    ncb = 6 * bw
    band, v = v[:n * ncb].reshape(n, ncb), v[n * ncb:]
    pb, v = v[:n * nb].reshape(n, nb), v[n * nb:]
    bb = v[:nb * nb].reshape(nb, nb)
    return status, band, pb, bb


def reference(M, free, scale):
    S = np.zeros_like(M)
    S[np.ix_(free, free)] = np.linalg.inv(M[np.ix_(free, free)])
    return S * scale[:, None] * scale[None, :]


def rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def check(harness, tmp_path, bw, nb, f0, lds, seed=0):
    rng = np.random.default_rng(1000 * bw + 10 * nb + f0 + seed)
    n_blk = f0 + bw + 3
    n = 6 * n_blk
    M, free = system(rng, n_blk, bw, nb, f0)
    scale = rng.uniform(0.2, 2.0, n + nb)
    status, band, pb, bb = run(harness, tmp_path, M, n, bw, nb, free, lds, scale)
    assert status == 0, status
    ref = reference(M, free, scale)
    want = band_rows(ref, n, bw)
    assert rel(band, want) < 1e-10, rel(band, want)
    if nb:
        assert rel(pb, ref[:n, n:]) < 1e-10, rel(pb, ref[:n, n:])
        assert rel(bb, ref[n:, n:]) < 1e-10, rel(bb, ref[n:, n:])


@pytest.mark.parametrize("bw", list(range(1, 43)))
def test_every_band_width(bw, harness, tmp_path):
    """One shape per band width: the LDS path wherever it holds the window, frozen prefix and border width varied along the way."""
    check(harness, tmp_path, bw, nb=[0, 14, 45][bw % 3], f0=2 * (bw % 2), lds=bw <= LDS_MAX_BW)


@pytest.mark.parametrize("bw,lds", [(2, True), (2, False), (21, True), (21, False), (22, False)])  # (6 bw > 128: global memory only)
@pytest.mark.parametrize("nb", [0, 14, 45])
@pytest.mark.parametrize("f0", [0, 3])
def test_paths_border_and_prefix(bw, lds, nb, f0, harness, tmp_path):
    check(harness, tmp_path, bw, nb, f0, lds)


@pytest.mark.parametrize("marker", [1.0, 0.0])
@pytest.mark.parametrize("lds", [True, False])
def test_zero_column_is_rank_deficient(marker, lds, harness, tmp_path):
    """A free coordinate no residual touches (the build writes 1.0 on its diagonal) or with a zero pivot is reported by its index."""
    rng = np.random.default_rng(7)
    bw, n_blk = 4, 9
    n = 6 * n_blk
    M, free = system(rng, n_blk, bw, 0, 0)
    col = 6 * 4 + 2
    M[col, :] = M[:, col] = 0.0
    M[col, col] = marker
    status, *_ = run(harness, tmp_path, M, n, bw, 0, free, lds)
    assert status == col + 1


def test_zero_border_column_is_rank_deficient(harness, tmp_path):
    rng = np.random.default_rng(8)
    bw, n_blk, nb = 3, 7, 14
    n = 6 * n_blk
    M, free = system(rng, n_blk, bw, nb, 0)
    col = n + 5
    M[col, :] = M[:, col] = 0.0
    M[col, col] = 1.0
    status, *_ = run(harness, tmp_path, M, n, bw, nb, free, True)
    assert status == col + 1


def test_constant_border_columns_have_zero_covariance(harness, tmp_path):
    rng = np.random.default_rng(9)
    bw, n_blk, nb = 3, 7, 14
    n = 6 * n_blk
    M, free = system(rng, n_blk, bw, nb, 1)
    const = [n + 1, n + 12]
    for c in const:
        M[c, :] = M[:, c] = 0.0
        M[c, c] = 1.0
        free[c] = False
    status, band, pb, bb = run(harness, tmp_path, M, n, bw, nb, free, True)
    assert status == 0
    ref = reference(M, free, np.ones(n + nb))
    assert rel(band, band_rows(ref, n, bw)) < 1e-10
    assert rel(pb, ref[:n, n:]) < 1e-10 and rel(bb, ref[n:, n:]) < 1e-10
    assert not bb[[1, 12], :].any() and not pb[:, [1, 12]].any() and not band[:6, :].any()
