"""CPU tests (no GPU): the product's spline routines — spline_pose, spline_pose_pre, spline_pose_jac, spline_pose_jac_pre, spline_full<K, true / false>,
spline_full_col (csrc/device_spline.hpp) with basis_weights<K> and segment_of (csrc/device_math.hpp) — compiled from the product's SOURCES
for the host (tests/emul/spline_harness.cpp) and run on the control points of tests/golden/factors_degenerate.json.gz: at rest, on both sides
of every threshold of rel_log / exp_scaled / jr_inv_coef, with flipped quaternion signs and with norms a few ulp off one.

Against the 100-digit vectors: q (up to sign), p, G and dth absolutely to 1e-13 (the bar of test_emulated_camera_model.py); w, alpha, dw, dal
to 1e-12 of the largest entry of the reference array (the vectors' own nested differences carry ~1e-14 of it), w and alpha with the floor that
the rounding of the inputs sets where the reference is zero (FLOOR below). Between the routines: bit for bit."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from util import golden_cases_degenerate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
DT = 0.1
# A platform at rest has w = alpha = 0 exactly, and a bar relative to the reference is then zero, which no double code can meet: R_{j-1}^T R_j of
# two EQUAL unit quaternions is a sum of four products of size <= 1 per component and comes out as 0 +- 4 ulp, not 0, so d_j = Log(.) is off by up
# to 8 eps, and w = sum_j dlam_j d_j, alpha ~ sum_j ddlam_j d_j with sum |dlam_j| <= 2 / dt, sum |ddlam_j| <= 2 / dt^2 (K <= 6). The same
# absolute error sits in every small relative rotation (the inputs are doubles of size 1, whatever the angle between them). That input
# rounding is the floor of the two bars (3.6e-14 rad/s and 3.6e-13 rad/s^2 at dt = 0.1); the vectors' own floor (1e-100 through the nested
# differences of make_golden.py) is far below it.
EPS = float(np.finfo(float).eps)
FLOOR = {"w": 16 * EPS / DT, "alpha": 16 * EPS / DT ** 2}


@pytest.fixture(scope="module")
def harness():
    exe = os.path.join(EMUL, "spline_harness")
    srcs = [os.path.join(EMUL, "spline_harness.cpp"), os.path.join(EMUL, "hip", "hip_runtime.h")]
    csrc = os.path.join(ROOT, "hyperslam_amd", "csrc")
    srcs += [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".hpp")]
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in srcs):
        subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-I", EMUL, "-o", exe, os.path.join(EMUL, "spline_harness.cpp")])
    return exe


def run(exe, cases):
    """Per case a dict name -> values of the product's routines (names as in spline_harness.cpp)."""
    text = ["%d\n" % len(cases)]
    for c in cases:
        P = c["inputs"]
        cps = np.array(P["cps"], float)
        text.append("%d %r %r %r\n" % (P["k"], float(P["stamp"]), float(cps[0, 7]), DT))
        text += [" ".join(repr(float(v)) for v in row) + "\n" for row in cps]
    with tempfile.TemporaryDirectory() as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as f:
            f.write("".join(text))
        subprocess.check_call([exe, fin, fout], timeout=120)
        lines = [l.split() for l in open(fout)]
    out, at = [], 0
    for c in cases:
        n = 7 + c["inputs"]["k"]
        out.append({l[0]: np.array(l[1:], float) for l in lines[at:at + n]})
        at += n
    assert at == len(lines)
    return out


@pytest.fixture(scope="module")
def results(harness):
    cases = golden_cases_degenerate()
    return cases, run(harness, cases)


def quat_err(q, ref):
    ref = np.asarray(ref, float)
    return float(min(np.abs(q - ref).max(), np.abs(q + ref).max()))


def test_against_the_degenerate_vectors(results):
    cases, outs = results
    worst = dict.fromkeys(("q", "p", "G", "dth", "w", "alpha", "v", "a", "dw", "dal"), 0.0)
    n_spline = n_rates = 0
    at_rest = {}
    for c, o in zip(cases, outs):
        ref, k = c["outputs"], c["inputs"]["k"]
        tag = (c["type"], c["pattern"], c["variant"], k)
        assert all(np.isfinite(v).all() for v in o.values()), tag
        for name in ("pose", "jac", "full", "full_value"):
            worst["q"] = max(worst["q"], quat_err(o[name][:4], ref["pose"][:4]))
            worst["p"] = max(worst["p"], float(np.abs(o[name][4:7] - ref["pose"][4:]).max()))
        full = o["full"]

        def relative(name, got, want):
            want = np.asarray(want, float)
            e = float(np.abs(np.asarray(got).reshape(want.shape) - want).max())
            scale = float(np.abs(want).max())
            assert e <= 1e-12 * scale + FLOOR.get(name, 0.0), (tag, name, e, scale)
            if FLOOR.get(name, 0.0) <= 1e-12 * scale:
                worst[name] = max(worst[name], e / scale)
            else:  # at rest or next to it (|w| < 3.6e-2 rad/s, |alpha| < 0.36 rad/s^2): the floor is the larger part of the bar
                at_rest[name] = max(at_rest.get(name, 0.0), e)

        if "w_b" in ref:
            n_rates += 1
            for name in ("full", "full_value"):
                relative("w", o[name][7:10], ref["w_b"])
                relative("alpha", o[name][10:13], ref["alpha_b"])
        if "v_w" in ref:
            relative("v", full[13:16], ref["v_w"])
            relative("a", full[16:19], ref["a_w"])
        if "G" in ref:
            n_spline += 1
            G = np.array(ref["G"])
            worst["G"] = max(worst["G"], float(np.abs(o["jac"][7:].reshape(k, 3, 3) - G).max()))
            worst["dth"] = max(worst["dth"], float(np.abs(full[19:19 + 9 * k].reshape(k, 3, 3) - G).max()))
            relative("dw", full[19 + 9 * k:19 + 18 * k], ref["dw"])
            relative("dal", full[19 + 18 * k:19 + 27 * k], ref["dal"])
    print("product spline sources against the 100-digit vectors, worst errors (q, p, G, dth absolute; the others relative to the largest entry):", worst,
          "; absolute, where the floor governs:", at_rest)
    assert n_spline == 33 and n_rates == 33 + 51
    assert max(worst[n] for n in ("q", "p", "G", "dth")) <= 1e-13, worst


def test_the_routines_agree_bit_for_bit(results):
    """spline_pose_jac == spline_pose_jac_pre; spline_pose == spline_pose_pre == the value part of spline_pose_jac; spline_full_col for every m ==
    the blocks of spline_full; the value part of spline_full does not depend on JAC."""
    cases, outs = results
    assert {c["inputs"]["k"] for c in cases} == {4, 5, 6}
    for c, o in zip(cases, outs):
        k = c["inputs"]["k"]
        tag = (c["type"], c["pattern"], c["variant"], k)
        assert np.array_equal(o["jac"], o["jac_pre"]), tag
        assert np.array_equal(o["pose"], o["pose_pre"]) and np.array_equal(o["pose"], o["jac"][:7]), tag
        full = o["full"]
        assert np.array_equal(full[:19], o["full_value"]), tag
        for m in range(k):
            col = o["col%d" % m]
            assert np.array_equal(col[:19], full[:19]), (tag, m)
            for n, name in enumerate(("dth", "dw", "dal")):
                blk = full[19 + 9 * k * n + 9 * m:19 + 9 * k * n + 9 * m + 9]
                assert np.array_equal(col[19 + 9 * n:28 + 9 * n], blk), (tag, m, name)
            assert col[46] == full[19 + 27 * k + 2 * k + m], (tag, m)


def test_weights_against_cox_de_boor(results):
    """basis_weights<K> at the stamps of the vectors (u = 1e-9, interior, 1 - 1e-9) against the recursion, which shares nothing with the
    blending matrix: cumulative weights to 1e-15, lam_0 = 1 to the last bit but one."""
    from test_degenerate_golden import cumulative_weights
    cases, outs = results
    worst = 0.0
    for c, o in zip(cases, outs):
        P = c["inputs"]
        k, t0 = P["k"], P["cps"][0][7]
        x = (P["stamp"] - t0) / 0.1
        lam = cumulative_weights(k, x - np.floor(x))
        worst = max(worst, float(np.abs(o["lam"] - lam).max()))
    print("basis_weights against Cox-de Boor, worst absolute error:", worst)
    assert worst <= 1e-15
