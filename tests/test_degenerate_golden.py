"""CPU tests (no GPU): the oracle against tests/golden/factors_degenerate.json.gz — control points at rest, at the thresholds of the rotation
helpers and with flipped quaternion signs (tests/golden/make_degenerate_golden.py) — and a count, from the case inputs alone, of how often
each branch of those helpers is taken: the vectors are not vacuous.

The oracle (oracle/hs_math.hpp) has the same thresholds as the product (csrc/device_spline.hpp, csrc/device_math.hpp); the vectors come
from mpmath at 100 digits, which has none."""
import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic
from util import check_against_golden, golden_cases_degenerate, golden_window

ORDERS = (4, 5, 6)
PATTERNS = ("zero", "tiny", "log_series", "exp_series", "below_t2", "above_t2", "mixed", "flip", "flip_small", "near_pi_flip", "unit_ulp")


@pytest.fixture(scope="module")
def cases():
    return golden_cases_degenerate()


def test_file_is_complete(cases):
    assert len(cases) == 222
    for k in ORDERS:
        for t in ("pixel", "bearing", "prior", "inertial"):
            have = {(c["pattern"], c["variant"]) for c in cases if c["type"] == t and c["inputs"]["k"] == k}
            want = {(p, None) for p in PATTERNS} | {(p, v) for p in ("zero", "above_t2", "flip") for v in ("u0", "u1")}
            if t == "prior":
                want |= {("zero", "prior_small"), ("regular", "prior_small")}
            assert have == want, (k, t, have ^ want)
        small = sorted(c["prior_angle"] for c in cases if c["variant"] == "prior_small" and c["inputs"]["k"] == k)
        assert small == [1e-9, 1e-9, 0.99e-4, 0.99e-4, 1.01e-4, 1.01e-4]
        spline = [c["pattern"] for c in cases if "G" in c["outputs"] and c["inputs"]["k"] == k]
        assert sorted(spline) == sorted(PATTERNS)  # one set of spline derivatives per pattern and order


def test_oracle_matches_degenerate_golden(cases, oracle):
    """Every case at the bar the oracle has on factors.json (1e-9; prior_small: 1e3 times that, like small_angle)."""
    worst = {}
    for case in cases:
        with ha.Problem(golden_window(case), lib=oracle) as p:
            errs = check_against_golden(p, case, 1e-9)
        key = case["type"] + (":prior_small" if case["variant"] == "prior_small" else "")
        if max(errs.values()) > worst.get(key, (0.0,))[0]:
            worst[key] = (max(errs.values()), case["pattern"], case["inputs"]["k"], max(errs, key=errs.get))
    print("oracle against the degenerate vectors, worst relative error per factor:", worst)


# ---- which branch does a case take? A numpy restatement of the four conditions, from the inputs alone -------------------------------
def relative_quaternion(a, b):
    return synthetic.quat_mul(np.asarray(a, float) * [-1, -1, -1, 1], np.asarray(b, float))


def log_conditions(r):
    """(w < 0, n2, t2) of the logarithm of quaternion r as the helpers compute them."""
    neg = bool(r[3] < 0)
    if neg:
        r = -r
    n2 = float(r[:3] @ r[:3])
    s = 2.0 / r[3] * (1.0 - n2 / (3.0 * r[3] * r[3])) if n2 < 1e-16 else 2.0 * np.arctan2(np.sqrt(n2), r[3]) / np.sqrt(n2)
    return neg, n2, s * s * n2


def cumulative_weights(k, u):
    """Cumulative uniform B-spline weights on [0, 1) by the Cox-de Boor recursion."""
    def N(j, order, x):
        if order == 1:
            return 1.0 if j <= x < j + 1 else 0.0
        return (x - j) / (order - 1) * N(j, order - 1, x) + (j + order - x) / (order - 1) * N(j + 1, order - 1, x)
    b = [N(j, k, u) for j in range(-(k - 1), 1)]
    return [sum(b[j:]) for j in range(k)]


def branch_counts(cases):
    count = {k: dict.fromkeys(("w<0", "w>=0", "n2<", "n2>=", "t2<", "t2>=", "a2<", "a2>=", "prior w<0", "prior w>=0", "prior n2<", "prior n2>=",
                               "prior t2<", "prior t2>="), 0) for k in ORDERS}
    for c in cases:
        P = c["inputs"]
        k, cps = P["k"], np.array(P["cps"], float)
        i = (k - 1) // 2
        lam = cumulative_weights(k, (P["stamp"] - cps[i, 7]) / (cps[i + 1, 7] - cps[i, 7]))
        n = count[k]
        for j in range(1, k):
            neg, n2, t2 = log_conditions(relative_quaternion(cps[j - 1, :4], cps[j, :4]))
            n["w<0" if neg else "w>=0"] += 1
            n["n2<" if n2 < 1e-16 else "n2>="] += 1
            n["t2<" if t2 < 1e-8 else "t2>="] += 1
            n["a2<" if lam[j] * lam[j] * t2 < 1e-10 else "a2>="] += 1
        if c["type"] == "prior":  # the residual rotation Log(R_m^T R_ws): so3_log and so3_coef in prior_linearize
            q = np.array(c["outputs"]["pose"][:4])
            neg, n2, t2 = log_conditions(relative_quaternion(P["meas"][:4], synthetic.quat_mul(q, np.array(P["T_bs"][:4]))))
            n["prior w<0" if neg else "prior w>=0"] += 1
            n["prior n2<" if n2 < 1e-16 else "prior n2>="] += 1
            n["prior t2<" if t2 < 1e-8 else "prior t2>="] += 1
    return count


def test_every_branch_is_taken_on_both_sides(cases):
    count = branch_counts(cases)
    print("control-point pairs (and prior residual rotations) per branch and order:", count)
    for k in ORDERS:
        for name, n in count[k].items():
            # (a prior 1e-9 rad from its measurement exists twice per order: on the zero and on the regular control points)
            assert n >= (2 if name == "prior n2<" else 3), (k, name, n)
    # the patterns do what their names say: every pair of these is on the named side of its threshold
    for c in cases:
        P = c["inputs"]
        cps = np.array(P["cps"], float)
        conds = [log_conditions(relative_quaternion(cps[j - 1, :4], cps[j, :4])) for j in range(1, P["k"])]
        if c["pattern"] in ("zero", "tiny"):
            assert all(n2 < 1e-16 and not neg for neg, n2, _ in conds)
        if c["pattern"] == "below_t2":
            assert all(1e-16 <= n2 and 0.97e-8 < t2 < 1e-8 for _, n2, t2 in conds)
        if c["pattern"] == "above_t2":
            assert all(1e-8 <= t2 < 1.03e-8 for _, _, t2 in conds)
        if c["pattern"] == "log_series":
            assert {n2 < 1e-16 for _, n2, _ in conds} == {True, False}
        if c["pattern"] in ("flip", "flip_small", "near_pi_flip"):
            assert sum(neg for neg, _, _ in conds) >= 2
        if c["pattern"] == "unit_ulp":
            norms = np.linalg.norm(cps[:, :4], axis=1)
            assert np.abs(norms - 1).max() < 1e-15 and np.abs(norms - 1).max() > 1e-16
