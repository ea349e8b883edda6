"""What the wave primitives under the product's kernels compute, stated in numpy as lane maps (TEST INFRASTRUCTURE).

tests/device/primitives_probe.hpp calls the product's spelling of each primitive and writes every lane's result; this module says what those
results must be. Two tests hold the same statement against the two compilations of that one kernel: tests/test_emulator_primitives.py (the host
emulator, tests/emul/hip/hip_runtime.h) and tests/test_gpu_primitives.py (gfx950). Lane maps move bits, so equality is on the bits; fused
operations are computed exactly in fractions.Fraction and rounded once; the rsq reference is numpy.longdouble.

Layout of every array: (values per lane, lanes) — value e of lane t at [e, t], as the probe reads and writes them."""
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_HEADER = os.path.join(ROOT, "tests", "emul", "hip", "hip_runtime.h")

DPP, SUMS, SHFL, READLANE, BALLOT, BCAST, ARITH, MFMA, RSQ = range(9)
NAMES = ["dpp", "sums", "shfl", "readlane", "ballot", "bcast", "arith", "mfma", "rsq"]
IN_PER_LANE = [1, 5, 2, 1, 1, 3, 3, 8, 0]     # hs_probe::kInPerLane
OUT_PER_LANE = [9, 7, 18, 64, 4, 48, 6, 8, 0]  # hs_probe::kOutPerLane


def emulator_rsq_epsilon():
    """The relative error the emulator gives its rsq estimate: the one statement of it is the constant in the emulator's header."""
    m = re.search(r"kRsqRelErr\s*=\s*(0x[0-9a-fA-F.]+p[-+]?\d+)\s*;", open(EMUL_HEADER).read())
    assert m, "kRsqRelErr not found in " + EMUL_HEADER
    return float.fromhex(m.group(1))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(got, want):
    return np.array_equal(bits(got), bits(want))


def fma(a, b, c):
    """a * b + c rounded once (exact in rationals; int / int division in Python rounds correctly, to nearest even)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, float), np.asarray(b, float), np.asarray(c, float))
    out = np.empty(a.shape)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


def inputs(family, threads, integers, seed=20240519):
    """Distinct values per lane: random f64, or small non-zero integers (every sum and product exact, no sum of two of them a signed zero)."""
    rng = np.random.default_rng(seed + 1000 * family + threads + int(integers))
    shape = (IN_PER_LANE[family], threads)
    if family == BALLOT:
        return rng.standard_normal(shape)  # (the predicate is x > 0)
    if integers:
        return (rng.integers(1, 10, shape) * rng.choice([-1, 1], shape) + 32 * np.arange(threads)[None, :] * (family in (DPP, SHFL, READLANE))).astype(float)
    x = rng.standard_normal(shape)
    if family == SHFL:
        x[1] = rng.integers(-(1 << 30), 1 << 30, threads)  # (the int the probe shuffles)
    return x


# ---- lane maps: source lane (index into the workgroup) of every lane, -1 = no source (a DPP move then keeps `old`, which the kernels set to 0) ----

def dpp_source(ctrl, threads):
    t = np.arange(threads)
    lane, row = t & 63, t & 15
    if ctrl < 0x100:  # quad_perm: two bits per lane of the quad
        return (t & ~3) | ((ctrl >> (2 * (t & 3))) & 3)
    n = ctrl & 15
    if 0x100 < ctrl < 0x110:  # row_shl:n — lane i reads lane i + n of its row of 16
        return np.where(row + n < 16, t + n, -1)
    if 0x110 < ctrl < 0x120:  # row_shr:n — lane i reads lane i - n of its row
        return np.where(row - n >= 0, t - n, -1)
    if 0x120 < ctrl < 0x130:  # row_ror:n — rotation inside the row
        return (t & ~15) | ((row - n) & 15)
    raise ValueError(hex(ctrl))


def dpp_move(v, ctrl):
    src = dpp_source(ctrl, len(v))
    return np.where(src >= 0, v[np.maximum(src, 0)], 0.0)


def lane_xor(v, mask):
    return v[np.arange(len(v)) ^ mask]


def wave_sum(v):
    """kernels_common.hpp: the butterfly over lane ^ 32, 16, 8, 4, 2, 1 in this order; every lane ends with the same bits."""
    v = np.array(v, float)
    for mask in (32, 16, 8, 4, 2, 1):
        v = v + lane_xor(v, mask)
    return v


def block_sum(v):
    """The wave sums added in wave order, from 0."""
    s = 0.0
    for w in wave_sum(v)[::64]:
        s = s + w
    return s


def model(family, x, threads):
    """Expected output of the probe, (OUT_PER_LANE, threads), and a mask of the entries the primitive specifies."""
    t = np.arange(threads)
    out = np.zeros((OUT_PER_LANE[family], threads))
    valid = np.ones(out.shape, bool)
    if family == DPP:
        v = x[0]
        for e, ctrl in enumerate((0xB1, 0x4E, 0x104, 0x114, 0x128)):
            out[e] = dpp_move(v, ctrl)
        out[5], out[6], out[7] = lane_xor(v, 1), lane_xor(v, 2), lane_xor(v, 4)
        out[8] = v + lane_xor(v, 1)  # pair_sum
    elif family == SUMS:
        out[0] = wave_sum(x[0])
        out[1, 0] = block_sum(x[0])
        for e in range(5):
            out[2 + e, 0] = block_sum(x[e])
        valid[1:, 1:] = False  # block sums: thread 0
    elif family == SHFL:
        iv = x[1].astype(np.int64).astype(float)
        for b in range(6):
            out[b], out[6 + b] = lane_xor(x[0], 1 << b), lane_xor(iv, 1 << b)
            out[12 + b] = iv[np.where((t & 63) >= (1 << b), t - (1 << b), t)]  # __shfl_up: a lane without a source keeps its own value
    elif family == READLANE:
        for s in range(64):
            out[s] = x[0][(t & ~63) + s]
    elif family == BALLOT:
        pred = x[0] > 0.0
        for w0 in range(0, threads, 64):
            lanes = np.arange(w0, min(w0 + 64, threads))  # a partial last wave: lanes that do not exist vote 0
            m = sum(1 << int(l - w0) for l in lanes if pred[l])
            out[0, lanes], out[1, lanes], out[2, lanes] = m & 0xffffffff, m >> 32, bin(m).count("1")
            out[3, lanes] = [bin(m & ((1 << int(l - w0)) - 1)).count("1") for l in lanes]
    elif family == BCAST:
        u, m, acc = x
        for r in range(16):
            ub = u[(t & ~15) | r]  # row_newbcast:R — lane R of the caller's row of 16
            out[3 * r], out[3 * r + 1], out[3 * r + 2] = ub, fma(ub, m, acc), fma(ub, -m, acc)
    elif family == ARITH:
        a, b, c = x
        out[0], out[1], out[2], out[3] = a * b, fma(a, b, c), fma(-a, b, 1.0), fma(a, b, 0.5)
        out[4], out[5] = a * c, b * c
    elif family == MFMA:
        one, _, _ = mfma(x[0], x[1], x[2:6])
        two, _, _ = mfma(x[6], x[7], one)
        out[:4], out[4:] = one, two
    return out, valid


def mfma(a, b, c):
    """v_mfma_f64_16x16x4_f64 on one wave: lane l supplies A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; register r of lane l holds
    D[(l >> 4) + 4 r][l & 15]. Returns, in the register layout (4, 64): the sequential chain (k = 0 .. 3, one fma each onto c: the emulator's
    order), the exact value rounded once, and |c| + sum_k |a_ik b_kj| (the scale of the bound that holds for any order of the four products)."""
    l = np.arange(64)
    A, B = np.zeros((16, 4)), np.zeros((4, 16))
    A[l & 15, l >> 4], B[l >> 4, l & 15] = a, b
    chain, exact, scale = np.zeros((4, 64)), np.zeros((4, 64)), np.zeros((4, 64))
    for r in range(4):
        for ln in range(64):
            i, j = (ln >> 4) + 4 * r, ln & 15
            acc, ex = float(c[r][ln]), Fraction(float(c[r][ln]))
            for k in range(4):
                p = Fraction(float(A[i, k])) * Fraction(float(B[k, j]))
                acc, ex = float(p + Fraction(acc)), ex + p
            chain[r, ln], exact[r, ln] = acc, float(ex)
            scale[r, ln] = abs(c[r][ln]) + np.abs(A[i] * B[:, j]).sum()
    return chain, exact, scale


# ---- rsq ---------------------------------------------------------------------------------------------------------------------------------

RSQ_EXPONENTS = (-600, -200, -40, -2, 0, 1, 40, 200, 600)
RSQ_SPECIALS = np.array([0.0, -0.0, -1.0, np.inf, np.nan, 2.0 ** -1022, 2.0 ** -1040])  # .., the smallest normal, a denormal
RSQ_SPECIAL_NAMES = ["+0", "-0", "-1", "+inf", "nan", "smallest normal", "denormal 2^-1040"]


def rsq_sweep():
    """d = m 2^k: 4096 evenly spaced mantissas in [1, 4) (both parities of the exponent the square root halves) for each k."""
    m = 1.0 + 3.0 * np.arange(4096) / 4096.0
    return np.concatenate([np.ldexp(m, k) for k in RSQ_EXPONENTS])


def rsq_relative_error(y, d):
    """|y sqrt(d) - 1| in long double (64-bit mantissa: 2^-39 below the errors measured here)."""
    dl = np.asarray(d, np.longdouble)
    return np.abs(np.asarray(y, np.longdouble) * np.sqrt(dl) - 1.0)


def emulator_rsq(d):
    """The emulator's statement of the estimate: the correctly rounded 1 / sqrt(d), times 1 + eps where the lowest mantissa bit of d is set and
    1 - eps where it is clear (a pure function of d's bits); zeros, infinities and NaN pass through."""
    eps = emulator_rsq_epsilon()
    d = np.asarray(d, float)
    with np.errstate(all="ignore"):
        y = 1.0 / np.sqrt(d)
        pert = y * np.where(bits(d) & np.uint64(1), 1.0 + eps, 1.0 - eps)
    return np.where(np.isfinite(y) & (y > 0.0), pert, y)


# ---- the cases both tests run: (family, lanes, integer inputs) — 256 lanes = four waves unless the primitive asks otherwise -------------------

CASES = [(f, 256, i) for f in (DPP, SUMS, SHFL, READLANE, BCAST, ARITH) for i in (False, True)] + [(BALLOT, 256, False), (BALLOT, 96, False),
                                                                                                  (MFMA, 64, True), (MFMA, 64, False)]


def case_id(case):
    return "%s-%d-%s" % (NAMES[case[0]], case[1], "int" if case[2] else "f64")


def assert_probe_equals_model(family, x, got, threads):
    """Bit equality of a probe's output with the model, on every entry the primitive specifies; names the first entries that differ."""
    want, valid = model(family, x, threads)
    got = np.asarray(got, float).reshape(want.shape)
    differ = (bits(got) != bits(want)) & valid
    where = np.argwhere(differ)
    assert not differ.any(), "%s: %d entries differ from the model; first (value, lane): %s got %s want %s" % (
        NAMES[family], len(where), where[:6].tolist(), got[differ][:6].tolist(), want[differ][:6].tolist())
