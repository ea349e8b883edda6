"""The wave primitives under the product's kernels, on the hardware, against their statement in tests/primitive_models.py — the statement
tests/test_emulator_primitives.py holds the host emulator to, bit for bit. tests/device/libhs_probe.so (built by __graft_entry__.build() from
tests/device/primitives_probe.hpp with the product's flags) runs one workgroup per call through hs_probe_run.

Lane maps (DPP moves, row broadcasts, shuffles, readlane, ballot), the fixed-order sums and the fused f64 statements: equality on the bits.
The f64 MFMA: its operand / result layout on integer-valued inputs (exact in any order) on the bits; on random inputs against the emulator's
order of accumulation (MFMA_ORDER below). The rsq estimate: its largest relative error over the sweep is printed and must stay within half of
the error the emulator gives its own estimate (kRsqRelErr in tests/emul/hip/hip_runtime.h), and the specials the `fail` / `bad` paths of the
factorisations rely on are asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import primitive_models as pm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "device", "libhs_probe.so")


@pytest.fixture(scope="module")
def probe():
    assert os.path.exists(LIB), LIB + " is missing: __graft_entry__.build() makes it"
    lib = C.CDLL(LIB)
    lib.hs_probe_run.restype = C.c_int
    lib.hs_probe_run.argtypes = [C.c_int, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, C.c_int]

    def run(family, x, threads, n_out=None):
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        out = np.zeros(pm.OUT_PER_LANE[family] * threads if n_out is None else n_out)
        status = lib.hs_probe_run(family, x.ctypes.data_as(C.POINTER(C.c_double)), len(x), out.ctypes.data_as(C.POINTER(C.c_double)), len(out), threads)
        assert status == 0, "hs_probe_run(%s): status %d" % (pm.NAMES[family], status)
        return out

    return run


@pytest.mark.parametrize("case", [c for c in pm.CASES if c[0] != pm.MFMA], ids=pm.case_id)
def test_probe_equals_model(case, probe):
    family, threads, integers = case
    x = pm.inputs(family, threads, integers)
    pm.assert_probe_equals_model(family, x, probe(family, x, threads), threads)


def test_mfma_layout_on_integers(probe):
    """Integer-valued operands: every order of accumulation gives the same bits, so this pins the layout alone — A[l & 15][l >> 4],
    B[l >> 4][l & 15], D[(l >> 4) + 4 r][l & 15] — for one instruction and for two chained through the accumulator."""
    x = pm.inputs(pm.MFMA, 64, True)
    pm.assert_probe_equals_model(pm.MFMA, x, probe(pm.MFMA, x, 64), 64)


def test_mfma_order_of_accumulation(probe):
    """Random operands against the emulator's order (k = 0 .. 3, one fma each onto c). Measured on an MI355X: the hardware gives the chain's bits on all 256 + 256
    entries (largest distance from the exact value 1.8 x 2^-53 of |c| + sum |a b|), so bit equality is what is asserted: emulated matrix-core
    kernels are faithful to the bit. The bound below holds for any order of four products, fused or not; it is asserted first so that a part
    which accumulates in another order fails with the figure that says so."""
    x = pm.inputs(pm.MFMA, 64, False)
    got = probe(pm.MFMA, x, 64).reshape(8, 64)
    chain1, exact1, scale1 = pm.mfma(x[0], x[1], x[2:6])
    chain2, _, _ = pm.mfma(x[6], x[7], chain1)
    _, exact2, scale2 = pm.mfma(x[6], x[7], got[:4])  # (the second instruction on the accumulator the hardware handed it)
    differ = int((pm.bits(got[:4]) != pm.bits(chain1)).sum()), int((pm.bits(got[4:]) != pm.bits(chain2)).sum())
    excess = max((np.abs(got[:4] - exact1) / scale1).max(), (np.abs(got[4:] - exact2) / scale2).max()) / 2.0 ** -53
    print("f64 MFMA against the sequential fma chain: %d + %d of 256 + 256 entries differ; largest |got - exact| = %.3g x 2^-53 (|c| + sum |a b|)" % (*differ, excess))
    assert excess <= 8.0
    assert differ == (0, 0)


def test_rsq_estimate_error(probe):
    """The largest relative error of v_rsq_f64 over d = m 2^k (4096 mantissas in [1, 4), nine exponents), both spellings, against long double.
    Measured on an MI355X: 5.117e-08 = 2^-24.22 (at d = 8.884e-181), hence kRsqRelErr = 2^-23: the smallest power of two that is at least
    twice the measurement (the factor two: the sweep is a sample)."""
    eps = pm.emulator_rsq_epsilon()
    d = pm.rsq_sweep()
    got = probe(pm.RSQ, d, 256, 2 * len(d)).reshape(2, len(d))
    for name, y in zip(("__builtin_amdgcn_rsq", "dx_rsq"), got):
        err = pm.rsq_relative_error(y, d)
        worst = int(np.argmax(err))
        print("%s: largest relative error %.4g = 2^%.2f at d = %r; emulator's kRsqRelErr = 2^%d" % (name, float(err[worst]), np.log2(float(err[worst])), float(d[worst]), round(np.log2(eps))))
        assert np.isfinite(y).all() and float(err.max()) <= eps / 2
    print("the two spellings agree on the bits:", pm.same_bits(got[0], got[1]))


def test_rsq_specials(probe):
    """+0 -> +inf, -1 -> NaN, NaN -> NaN, +inf -> 0: what the `fail` / `bad` tests behind the pivots see. The others are printed next to what
    the emulator's statement gives; on an MI355X -0 gives -inf, the smallest normal 2^-1022 gives 2^511 and the denormal 2^-1040 gives 2^520 (denormal
    arguments are taken at their value, not flushed), and the emulator agrees in kind (-inf, and the two values off by its kRsqRelErr)."""
    eps = pm.emulator_rsq_epsilon()
    d = pm.RSQ_SPECIALS
    got = probe(pm.RSQ, d, 64, 2 * len(d)).reshape(2, len(d))
    emul = pm.emulator_rsq(d)
    for i, name in enumerate(pm.RSQ_SPECIAL_NAMES):
        print("rsq(%s): builtin %r dx_rsq %r emulator %r" % (name, float(got[0][i]), float(got[1][i]), float(emul[i])))
    for y in got:
        s = dict(zip(pm.RSQ_SPECIAL_NAMES, y))
        assert s["+0"] == np.inf and np.isnan(s["-1"]) and np.isnan(s["nan"]) and s["+inf"] == 0.0 and not np.signbit(s["+inf"])
        assert s["-0"] == -np.inf
        for name in pm.RSQ_SPECIAL_NAMES[5:]:
            arg = float(d[pm.RSQ_SPECIAL_NAMES.index(name)])
            assert float(pm.rsq_relative_error(s[name], arg)) <= eps / 2, name


def test_sizes_that_are_not_the_family_s_are_refused():
    lib = C.CDLL(LIB)
    x, out = np.zeros(255), np.zeros(9 * 256)
    assert lib.hs_probe_run(pm.DPP, x.ctypes.data_as(C.POINTER(C.c_double)), 255, out.ctypes.data_as(C.POINTER(C.c_double)), len(out), 256) == -1
