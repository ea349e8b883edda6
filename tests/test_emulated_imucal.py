"""CPU test (no GPU): the gathers of the free IMU columns (hyperslam_amd/csrc/kernels_imucal.hpp: k_imucal_pi, _bb, _ii, _finish) compiled
from the product's kernel SOURCE for the host (tests/emul/) and compared with numpy on fabricated inertial records:
    H_pi = sum A'C,   H_{b_g,j ; i} = sum wg[j] C[0:3, :],   H_{b_a,j ; i} = sum wa[j] C[3:6, :],   H_gi = sum Jg'C,   H_ii = sum C'C,   g_i = sum C'r.
Bar: 1e-12 relative to each block's max-norm — the inputs are O(1) and a sum has at most a few thousand terms of either sign, each rounded
to 2^-53 relative to a partial sum of that size."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
FIRST, SIZE = (0, 36, 72, 108, 162), (6, 6, 6, 9, 9)  # [T_bs | i_g | i_a | S_g | X_a] inside a record of sensor Jacobians (6 rows each)


@pytest.fixture(scope="session")
def harness():
    exe = os.path.join(EMUL, "imucal_harness")
    srcs = [os.path.join(EMUL, "imucal_harness.cpp"), os.path.join(EMUL, "hip", "hip_runtime.h")]
    csrc = os.path.join(ROOT, "hyperslam_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-I", EMUL, "-o", exe, os.path.join(EMUL, "imucal_harness.cpp")])
    return exe


def column_map(free):
    """Map entries (entry of row 0 | row stride << 16) of the free blocks, e.g. (1, 4) = i_g + X_a."""
    return [(FIRST[b] + j) | SIZE[b] << 16 for b in free for j in range(SIZE[b])]


CASES = [
    # K, kb, n_ine, free blocks, n_splits, slices of k_imucal_bb
    (4, 4, 1, (0,), 1, 1),
    (4, 4, 63, (3,), 2, 2),
    (5, 4, 64, (1, 4), 1, 1),
    (6, 4, 65, (0, 1, 2, 3, 4), 3, 3),
    (4, 3, 257, (0,), 2, 8),
]


@pytest.mark.parametrize("K,kb,n_ine,free,n_splits,n_slices", CASES)
def test_imu_gathers_against_numpy(harness, K, kb, n_ine, free, n_splits, n_slices):
    rng = np.random.default_rng(1000 * K + n_ine + kb)
    n_cp, n_bias, nc = K + 4, kb + 3, 3
    n_seg = n_cp - K + 1
    cmap = column_map(free)
    ni = len(cmap)
    assert ni in (6, 9, 15, 36)
    # records: segment-major, first_bias non-decreasing; the last segment and the last two bias points are never reached
    seg = np.sort(rng.integers(0, n_seg - 2, n_ine))
    fb = np.sort(rng.integers(0, n_bias - kb - 1, n_ine))
    if n_ine > 60:
        seg[seg == 2] = 3  # an empty segment in the middle
    seg_ptr = np.searchsorted(seg, np.arange(n_seg + 1)).astype(np.int32)
    bias_ptr = np.searchsorted(fb, np.arange(n_bias + 2)).astype(np.int32)
    irec = 18 + 36 * K + 2 * kb
    rec = rng.standard_normal((n_ine, irec))
    sj = rng.standard_normal((n_ine, 216))
    hdr = np.array([K, kb, n_cp, n_bias, n_ine, ni, n_splits, nc, n_slices], np.int32)
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            for a in (hdr, np.array(cmap, np.int32), seg_ptr, fb.astype(np.int32), bias_ptr, rec, sj):
                f.write(np.ascontiguousarray(a).tobytes())
        subprocess.check_call([harness, fin, fout], timeout=600)
        raw = np.fromfile(fout, np.float64)
    np_, nbi = 6 * n_cp, 6 * n_bias + 2
    nb = nbi + ni + nc
    per = n_splits * np_ * nb + nb * nb + nb
    assert raw.size == 2 * per
    assert np.array_equal(raw[:per], raw[per:])  # two runs: bit for bit
    part = raw[:n_splits * np_ * nb].reshape(n_splits, np_, nb)
    Hbb = raw[n_splits * np_ * nb:n_splits * np_ * nb + nb * nb].reshape(nb, nb)
    gb = raw[per - nb:per]

    # numpy
    r = rec[:, :6]
    A = rec[:, 6:6 + 36 * K].reshape(n_ine, 6, 6 * K)
    wg, wa = rec[:, 6 + 36 * K:6 + 36 * K + kb], rec[:, 6 + 36 * K + kb:6 + 36 * K + 2 * kb]
    Jg = rec[:, 6 + 36 * K + 2 * kb:].reshape(n_ine, 6, 2)
    C = np.stack([sj[:, (m & 0xffff) + np.arange(6) * (m >> 16)] for m in cmap], 2)  # (n, 6, ni)
    Hpi = np.zeros((np_, ni))
    Hbi = np.zeros((nbi, ni))
    for n in range(n_ine):
        Hpi[6 * seg[n]:6 * (seg[n] + K)] += A[n].T @ C[n]
        for j in range(kb):
            Hbi[3 * (fb[n] + j):3 * (fb[n] + j) + 3] += wg[n, j] * C[n, :3]
            Hbi[3 * n_bias + 3 * (fb[n] + j):3 * n_bias + 3 * (fb[n] + j) + 3] += wa[n, j] * C[n, 3:]
        Hbi[6 * n_bias:] += Jg[n].T @ C[n]
    Hii = np.einsum("nri,nrj->ij", C, C)
    gi = np.einsum("nri,nr->i", C, r)

    def close(got, want):
        return np.abs(got - want).max() <= 1e-12 * np.abs(want).max()

    imu = slice(nbi, nbi + ni)
    assert close(part[0][:, imu], Hpi), np.abs(part[0][:, imu] - Hpi).max()
    assert np.all(part[1:, :, imu] == 0.0)  # the other accumulation splits of the IMU columns are written zero
    other = np.ones(nb, bool)
    other[imu] = False
    assert np.all(part[:, :, other] == 7.0)  # bias / gravity / camera columns of the partials: not this file's
    assert close(Hbb[:nbi, imu], Hbi), np.abs(Hbb[:nbi, imu] - Hbi).max()
    assert close(Hbb[imu, imu], Hii), np.abs(Hbb[imu, imu] - Hii).max()
    assert close(gb[imu], gi), np.abs(gb[imu] - gi).max()
    assert np.array_equal(Hbb, Hbb.T)  # exact symmetry: every entry is written with its mirror
    assert np.all(Hbb[:nbi, :nbi] == 0.0) and np.all(Hbb[nbi + ni:, :] == 0.0) and np.all(gb[other] == 0.0)  # nothing else is touched
    # a control point no record reaches, a bias point whose range is empty: exact zeros
    reached = np.zeros(n_cp, bool)
    for s in seg:
        reached[s:s + K] = True
    assert not reached.all()
    for i in np.nonzero(~reached)[0]:
        assert np.all(part[0][6 * i:6 * i + 6, imu] == 0.0)
    covered = np.zeros(n_bias, bool)
    for f in fb:
        covered[f:f + kb] = True
    assert not covered.all()
    for b in np.nonzero(~covered)[0]:
        assert np.all(Hbb[3 * b:3 * b + 3, imu] == 0.0) and np.all(Hbb[3 * n_bias + 3 * b:3 * n_bias + 3 * b + 3, imu] == 0.0)
