"""The backward sweep with one phase per super-step (hyperslam_amd/csrc/kernels_backward_sb.hpp: k_band_backward_pm, its builders of the
stacked blocks [Winv_J ; U[above, J] Winv_J] and sb_sweep_pm) compiled from the product's source for the HOST (tests/emul/: one thread per
lane) and run, next to the two-phase sweep it replaces (k_band_backward_sb), on the factor the product's factorisation kernels leave of a
random banded SPD system: step against numpy's solve, new against old, the exact relations between solution, step and scaled step, both
ends' shares of the model cost change, and one stacked block per job against numpy. Bars: test_emulated_factor.py's.

The far sweep redoes the middle rows itself (phase A) while they span at most kSbPrefetch = 5 super-blocks. They are bw - 1 <= 15 block rows
(the two-ended factorisations hold bands of at most 16 control points), which touch at most 5 super-blocks of four: no two-ended shape with
6 (bw - 1) <= 96 reaches the other arrangement (the near sweep publishes, the far one waits); test_middle_rows_never_exceed_the_prefetch
checks that on what the harness reports for every residue of the split point."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from test_emulated_factor import band_rows, banded_spd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
K_SB, K_PREFETCH = 4, 5


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emul_backward_pm") / "backward_pm_harness")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-Wno-psabi", "-I", EMUL, "-o", exe, os.path.join(EMUL, "backward_pm_harness.cpp")])
    return exe


def dense_rows(Ub, bw, n_own):
    """Band storage -> dense rows, columns >= n_own dropped (band_entry's rule: they belong to the other job)."""
    n = len(Ub)
    U = np.zeros((n, n + 6 * bw))
    for r in range(n):
        c0 = 6 * (r // 6)
        U[r, c0:c0 + 6 * bw] = Ub[r]
    return U[:n_own, :n_own]


def check_stacked(Mb, U, s, bw, n_own):
    """Stacked block of super-block s against numpy on the upper factor U (job coordinates; rows and columns of the super-block must be
    rows of U that numpy knows): rows 0 .. 23 = inv(U_JJ), row 24 + p = U[r0 - 1 - p, J] inv(U_JJ); zero rows / columns where the system ends
    inside the super-block and for rows above the matrix."""
    n_above, r0 = 6 * (bw - 1), 24 * s
    nr = min(24, n_own - r0)
    blk = Mb[s * (24 + n_above) * 24:(s + 1) * (24 + n_above) * 24].reshape(24 + n_above, 24)
    Winv = np.linalg.inv(U[r0:r0 + nr, r0:r0 + nr])
    want = np.zeros_like(blk)
    want[:nr, :nr] = Winv
    for p in range(n_above):
        rho = r0 - 1 - p
        if rho >= 0:
            want[24 + p, :nr] = U[rho, r0:r0 + nr] @ Winv
    tol = 1e-9 * max(1.0, np.abs(want).max())
    print("stacked block", s, "max", np.abs(want).max(), "error", np.abs(blk - want).max())
    assert np.allclose(blk, want, rtol=0, atol=tol)
    assert np.array_equal(blk[:24][np.tril_indices(24, -1)], np.zeros(276))  # Winv is upper triangular to the bit


def run(exe, tmp_path, n_blk, bw, two_ended, f0=0):
    rng = np.random.default_rng(7 * n_blk + bw + 1000 * f0)
    M = banded_spd(rng, n_blk, bw)
    n = 6 * n_blk
    g = rng.standard_normal(n)
    if f0:  # sliding window: the leading block rows belong to constant control points (test_emulated_factor.test_frozen_prefix_against_numpy)
        k = 6 * f0
        M[:k, :], M[:, :k] = 0.0, 0.0
        M[:k, :k] = np.eye(k)
        g[:k] = 0.0
    P = np.arange(n)[::-1]
    aux = np.random.default_rng(n + bw)
    scale, g_full, d2 = aux.uniform(0.5, 2.0, n), aux.standard_normal(n), aux.uniform(0.0, 1.0, n)  # operands of the step outputs
    src, dst = str(tmp_path / "sys.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("=4i", n, bw, int(two_ended) | (f0 << 8), 0))
        for a in (band_rows(M, bw), g, band_rows(M[np.ix_(P, P)], bw), g[P], scale, g_full, d2):
            f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
    subprocess.check_call([exe, src, dst], timeout=180)
    raw = open(dst, "rb").read()
    m, mB, failed, mid_span = struct.unpack("=4i", raw[:16])
    v = np.frombuffer(raw[16:], dtype="<f8")
    ncb, nM = 6 * bw, (-(-n_blk // K_SB) + 1) * (24 + 6 * (bw - 1)) * 24
    parts, o = [], 0
    for size in (n * ncb, n * ncb, nM, nM) + 2 * (n, n, n, 4):
        parts.append(v[o:o + size])
        o += size
    assert failed == 0 and o == len(v)
    Ub, Ub2, Mb, Mb2 = parts[0].reshape(n, ncb), parts[1].reshape(n, ncb), parts[2], parts[3]
    old, new = parts[4:8], parts[8:12]
    x = np.linalg.solve(M, g)
    tol = 1e-9 * max(1.0, np.abs(x).max())
    for name, (xsol, step, delta, sums) in (("two-phase", old), ("one-phase", new)):
        print(name, "max |step + x|", np.abs(step + x).max(), "bar", tol)
        assert np.allclose(step, -x, rtol=0, atol=tol)
        assert np.array_equal(xsol, -step)
        assert np.array_equal(delta, scale * step)
        assert abs(sums[0] + sums[2] - g_full @ step) <= 1e-12 * np.abs(g_full * step).sum()
        assert abs(sums[1] + sums[3] - (d2 * step) @ step) <= 1e-12 * (d2 * step * step).sum()
    print("max |new - old|", np.abs(new[1] - old[1]).max())
    assert np.allclose(new[1], old[1], rtol=0, atol=tol)
    # ---- one stacked block per job against numpy ----
    U = np.linalg.cholesky(M).T
    if two_ended:
        assert m + (bw - 1) + mB == n_blk
        # near job: its rows below 6 m are the leading rows of the factor of M — the last super-block that lies inside them
        n_own = 6 * (m + bw - 1)
        Uj = dense_rows(Ub, bw, n_own)
        assert np.allclose(np.triu(Uj[:6 * m], 1), np.triu(U[:6 * m, :n_own], 1), rtol=0, atol=1e-10)
        check_stacked(Mb, U, 6 * m // 24 - 1, bw, n_own)
        # far job: the leading 6 mB rows of the factor of the reversed matrix, the last super-block (partial unless mB is a multiple of 4)
        U2 = np.linalg.cholesky(M[np.ix_(P, P)]).T
        check_stacked(Mb2, U2, -(-mB // K_SB) - 1, bw, 6 * mB)
    else:
        check_stacked(Mb, U, -(-n_blk // K_SB) - 1, bw, n)
    return m, mB, mid_span


@pytest.mark.parametrize("n_blk,bw", [(12, 3), (21, 4), (31, 6), (58, 14), (64, 16)])
def test_two_ended_sweeps_against_numpy(n_blk, bw, harness, tmp_path):
    """(12, 3) the shortest two-ended system; (21, 4), (31, 6) rows of either job no multiple of 4: a partial last super-block; (58, 14) the
    band of configs[1]; (64, 16) the WIDE factor, the most pending rows that still come with 16 block rows."""
    m, mB, mid_span = run(harness, tmp_path, n_blk, bw, True)
    print("m", m, "mB", mB, "sA_top - sA_pub", mid_span)
    if (n_blk, bw) in ((21, 4), (31, 6)):
        assert (m + bw - 1) % K_SB or mB % K_SB
    assert mid_span + 1 <= K_PREFETCH  # phase A


@pytest.mark.parametrize("n_blk,bw", [(65, 16), (67, 16), (69, 16)])
def test_middle_rows_never_exceed_the_prefetch(n_blk, bw, harness, tmp_path):
    """The widest two-ended band at the other residues of the split point m modulo 4 (m = 27, 28, 29; (64, 16) above has 26): the middle
    rows span at most kSbPrefetch super-blocks, so the far sweep always redoes them (see the module docstring)."""
    m, mB, mid_span = run(harness, tmp_path, n_blk, bw, True)
    print("m", m, "mB", mB, "sA_top - sA_pub", mid_span)
    assert mid_span + 1 <= K_PREFETCH


@pytest.mark.parametrize("n_blk,bw,f0", [(9, 5, 0), (30, 14, 0), (30, 14, 9)])
def test_one_ended_sweeps_against_numpy(n_blk, bw, f0, harness, tmp_path):
    """The one-ended launch (bordered systems, short windows): workgroup 0 sweeps the whole factor down to block row f0, the frozen prefix."""
    run(harness, tmp_path, n_blk, bw, False, f0)
