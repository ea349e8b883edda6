"""The verdict of every factorisation kernel of the reduced system: DevState::chol_failed == 1 if and only if a pivot the kernel computes is
not a positive finite number. decide_step (kernels_update.hpp) consumes the verdict as Ceres' invalid-step branch (nothing committed, radius
halved, FAILURE after five in a row); where it is not raised, a NaN factor and a NaN step go on as if they were a solution.
The kernels are compiled from the product's source for the host (tests/emul/factor_harness.cpp, the harness of test_emulated_factor.py) and
run on a positive definite band system with ONE diagonal entry replaced:
  negative  -0.5
  nan, inf  a non-finite entry: the pivot of that row is the entry itself
  zero      the row decoupled (zero off-diagonals) with a zero diagonal: the pivot is 0 in exact arithmetic AND in the kernel (a diagonal
            lowered by the exact pivot lands on either side of zero by rounding)
at the first and last row of the system, the first and last scalar row (a = 0, a = 5) of the last block row and of a middle one, in either
job, at both ends of the junction of a two-ended run, in the border, in the frozen prefix. The last block row is where a kernel that only
notices a NaN through the NEXT pivot has nothing left to notice it with (fmin(good, NaN) = good; +inf > 0).
Negative controls at the same shapes and positions keep the verdict from over-reporting: the clean matrix, and the same diagonal entry
lowered until the matrix is 1e-3 of the way from singular — numpy's Cholesky still succeeds, every pivot >= 1e-6 of its diagonal entry,
asserted here — give failed == 0 and pass run()'s comparison with numpy's solve."""
import time

import numpy as np
import pytest

from test_emulated_factor import banded_spd, bordered, harness, run, run_border_mode_raw, run_raw  # noqa: F401  (harness: the fixture)

KINDS = ("negative", "nan", "inf", "zero")


def with_defect(A, r, kind):
    A2 = A.copy()
    if kind == "zero":
        A2[r, :], A2[:, r] = 0.0, 0.0
    else:
        A2[r, r] = {"negative": -0.5, "nan": np.nan, "inf": np.inf}[kind]
    return A2


def with_small_pivot(A, Ainv, r):
    """A - delta e_r e_r' is positive definite iff delta < 1 / inv(A)[r][r] (then det = det A (1 - delta inv(A)[r][r])), in every elimination
    order. delta = 0.999 of that bound: the product of the pivots shrinks by 1e-3, wherever the kernel's order puts the small one."""
    A2 = A.copy()
    A2[r, r] -= (1.0 - 1e-3) / Ainv[r, r]
    U = np.linalg.cholesky(A2).T  # (raises if the matrix is not positive definite)
    ratio = np.diag(U) ** 2 / np.diag(A2)
    assert ratio.min() >= 1e-6, (r, ratio.min())
    return A2


def join(M, border):
    return M if border is None else np.block([[M, border[0]], [border[0].T, border[1]]])


def split(A, n, border):
    if border is None:
        return A, None
    return np.ascontiguousarray(A[:n, :n]), (np.ascontiguousarray(A[:n, n:]), np.ascontiguousarray(A[n:, n:]), border[2], border[3])


def block_rows(i):
    return {"a0": 6 * i, "a5": 6 * i + 5}


def band_positions(n_blk, bw, two_ended, m, mB):
    """Rows by the job split the harness returned for the clean matrix. One-ended: the chain ends in block row n_blk - 1. Two-ended: near job
    [0, m), far job (m + w, n_blk) factored from the far end, the w = bw - 1 middle rows last (the junction: block row m + w - 1 ends the chain)."""
    n, pos = 6 * n_blk, {"row0": 0}
    pos["row_last"] = n - 1
    if not two_ended:
        for k, r in block_rows(n_blk - 1).items():
            pos["last_block_" + k] = r
        for k, r in block_rows(n_blk // 2).items():
            pos["middle_block_" + k] = r
        return pos
    w = bw - 1
    assert m + w + mB == n_blk
    for k, r in block_rows(m // 2).items():  # a middle block row, in the near job
        pos["near_job_" + k] = r
    pos["far_job_last_block_a5"] = 6 * (m + w)  # (the far job runs from row n - 1 down: row 6 (m + w) is the last scalar row of its last block row)
    pos["junction_first_row"] = 6 * m
    pos["last_block_a0"], pos["junction_last_row"] = 6 * (m + w - 1), 6 * (m + w) - 1  # the chain's last block row
    return pos


def check_verdicts(exe, tmp_path, M, g, bw, two_ended, variant, f0=0, border=None, positions=None, zero_step=False):
    n = len(M)
    t0 = time.monotonic()
    m, mB = run(exe, tmp_path, M, g, bw, two_ended, variant, f0, border)[:2]  # the clean matrix: failed == 0, numpy's solution
    t_clean = time.monotonic() - t0
    A = join(M, border)
    Ainv = np.linalg.inv(A)
    pos = positions(m, mB) if callable(positions) else positions
    wrong = []
    for label, r in pos.items():
        M2, b2 = split(with_small_pivot(A, Ainv, r), n, border)
        run(exe, tmp_path, M2, g, bw, two_ended, variant, f0, b2)  # small but safely positive: failed == 0, numpy's solution
        for kind in KINDS:
            M2, b2 = split(with_defect(A, r, kind), n, border)
            t0 = time.monotonic()
            rc, failed, out = run_raw(exe, tmp_path, M2, g, bw, two_ended, variant, f0, b2)
            dt = time.monotonic() - t0
            # No hang and no wait that ran out: the run of a failed factorisation takes what the clean one took (a bounded wait that gives up
            # costs 2 s on the device and marks the run with failed == 2; on the emulator's clock it would never end).
            if rc != 0 or failed != 1 or dt > t_clean + 1.0:
                wrong.append((label, r, kind, "rc %s failed %s %.2f s (clean %.2f s)" % (rc, failed, dt, t_clean)))
            elif zero_step:  # k_dense_solve_mx: the step of a failed factorisation is zero (kernels_dense_mx.hpp)
                step, delta, xb = out[2][7], out[2][8], out[2][10]
                if not (np.all(step == 0.0) and np.all(delta == 0.0) and np.all(xb == 0.0)):
                    wrong.append((label, r, kind, "step / scaled step / x_b not exactly zero"))
    assert not wrong, wrong


@pytest.mark.parametrize("variant,n_blk,bw,two_ended", [
    (0, 20, 4, False), (0, 20, 4, True),  # k_band_factor_la
    (1, 20, 12, False), (2, 24, 18, False),  # k_band_factor<1>, <2>
    (3, 20, 24, False),  # k_band_factor_wide
    (4, 24, 20, False),  # k_dense_factor
    (5, 20, 4, True), (5, 30, 14, False), (5, 58, 14, True), (5, 60, 15, True)])  # k_band_factor_mx; (60, 15): the WIDE instance
def test_band_factor_verdict(variant, n_blk, bw, two_ended, harness, tmp_path):
    rng = np.random.default_rng(4000 + 100 * variant + n_blk + bw + int(two_ended))
    M = banded_spd(rng, n_blk, bw)
    g = rng.standard_normal(6 * n_blk)
    check_verdicts(harness, tmp_path, M, g, bw, two_ended, variant, positions=lambda m, mB: band_positions(n_blk, bw, two_ended, m, mB))


@pytest.mark.parametrize("n_blk,bw,n_b", [(5, 4, 0), (33, 33, 0), (34, 34, 51)])
def test_dense_solve_mx_verdict(n_blk, bw, n_b, harness, tmp_path):
    """k_dense_solve_mx: first row, both sides of the first panel's edge (rows 15 and 16), the last real row in front of the identity padding,
    and with a border its first and last column. A failed factorisation leaves step, scaled step and x_b exactly zero."""
    rng = np.random.default_rng(4600 + n_blk + bw + n_b)
    M = banded_spd(rng, n_blk, bw)
    n = 6 * n_blk
    g = rng.standard_normal(n)
    border = None
    pos = {"row0": 0, "row15": 15, "row16": 16, "last_pose_row": n - 1}
    if n_b:
        border = bordered(rng, M, n_b, n_blk)
        pos.update({"border_first": n, "border_last": n + n_b - 1})  # (n + n_b - 1: the last real row)
    check_verdicts(harness, tmp_path, M, g, bw, False, 6, border=border, positions=pos, zero_step=True)


@pytest.mark.parametrize("n_b", [1, 17, 64])
def test_dense_solve_mx_border_mode_verdict(n_b, harness, tmp_path):
    """k_dense_solve_mx in border mode: the verdict on the border Schur complement of a two-ended bordered system; x_b of a failed
    factorisation is exactly zero (nothing behind this kernel looks at the numbers again before k_border_apply uses them)."""
    rng = np.random.default_rng(4700 + n_b)
    B = rng.standard_normal((n_b, n_b + 8))
    C = B @ B.T + np.diag(rng.uniform(0.5, 1.5, n_b))
    h = rng.standard_normal(n_b)
    Cinv = np.linalg.inv(C)

    def solves(C2):
        failed, xb = run_border_mode_raw(harness, tmp_path, C2, h)
        want = np.linalg.solve(C2, h)
        assert failed == 0 and np.allclose(xb, want, rtol=0, atol=1e-10 * max(1.0, np.abs(want).max()))

    t0 = time.monotonic()
    solves(C)
    t_clean = time.monotonic() - t0
    wrong = []
    for r in sorted({0, 15, 16, n_b // 2, n_b - 1} & set(range(n_b))):
        solves(with_small_pivot(C, Cinv, r))
        for kind in KINDS:
            t0 = time.monotonic()
            failed, xb = run_border_mode_raw(harness, tmp_path, with_defect(C, r, kind), h)
            dt = time.monotonic() - t0
            if failed != 1 or dt > t_clean + 1.0 or len(xb) != n_b or not np.all(xb == 0.0):
                wrong.append((r, kind, failed, dt, xb))
    assert not wrong, wrong


@pytest.mark.parametrize("n_blk,bw,n_b,two_ended", [(24, 6, 9, False), (31, 6, 3, True), (26, 5, 131, False)])  # (131: k_border_solve, not _reg)
def test_border_solve_verdict(n_blk, bw, n_b, two_ended, harness, tmp_path):
    """The bordered chain behind k_band_factor_la: the pose part clean, the defect on the diagonal of S_bb — first, middle and last border
    column (the last one: the odd tail of k_border_solve_reg, the last column of k_border_solve). The verdict comes from the border solve."""
    rng = np.random.default_rng(4800 + n_blk + bw + n_b)
    M = banded_spd(rng, n_blk, bw)
    n = 6 * n_blk
    g = rng.standard_normal(n)
    pos = {"border_first": n, "border_second": n + 1, "border_middle": n + n_b // 2, "border_last": n + n_b - 1}
    check_verdicts(harness, tmp_path, M, g, bw, two_ended, 0, border=bordered(rng, M, n_b, n_blk), positions=pos)


@pytest.mark.parametrize("variant,n_blk,bw,f0", [(0, 24, 6, 23), (4, 36, 18, 14)])
def test_frozen_prefix_verdict(variant, n_blk, bw, f0, harness, tmp_path):
    """Sliding window: the defect in the first free block row (the chain's first pivot, and with f0 = 23 of 24 also its last block row) and
    inside the frozen prefix, whose decoupled rows are factored one wave each (k_factor_decoupled_rows; extra workgroups of k_dense_factor)."""
    rng = np.random.default_rng(4900 + variant + n_blk + bw + f0)
    M = banded_spd(rng, n_blk, bw)
    g = rng.standard_normal(6 * n_blk)
    k = 6 * f0
    M[:k, :], M[:, :k] = 0.0, 0.0
    M[:k, :k] = np.eye(k)
    g[:k] = 0.0
    pos = {"first_free_row": k, "first_free_block_a5": k + 5, "last_row": 6 * n_blk - 1,
           "prefix_first_row": 0, "prefix_middle_a0": 6 * (f0 // 2), "prefix_last_row": k - 1}
    check_verdicts(harness, tmp_path, M, g, bw, False, variant, f0, positions=pos)
