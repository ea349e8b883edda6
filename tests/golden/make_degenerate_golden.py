#!/usr/bin/env python3
"""Generates tests/golden/factors_degenerate.json.gz — the 100-digit restatement of make_golden.py on
control points that take the SECOND branch of every rotation helper of the spline (csrc/device_spline.hpp, csrc/device_math.hpp):

  n2 < 1e-16  (rel_log, so3_log)        relative rotation below ~2e-8 rad: series of the logarithm
  r.w < 0     (rel_log, so3_log)        consecutive control points stored with opposite quaternion signs (double cover)
  a2 < 1e-10  (exp_scaled)              lam_j * theta_j below 1e-5 rad: series of the half-angle quaternion and of J_r
  t2 < 1e-8   (jr_inv_coef, so3_coef)   relative rotation, or a prior's residual rotation, below 1e-4 rad

The factors, retractions and differences are the functions of make_golden.py; only the control points are built here: a random unit
quaternion, then step j multiplies by Exp(angle_j * axis_j) with a fresh random unit axis, then the quaternions listed under "flip" are
negated. Inputs are rounded to doubles before any output is computed. No threshold of the product appears in what is computed: mpmath's
exp / log at 100 digits have no small-angle branch besides the exact zero.

Outputs per case: r, J_state, J_landmark / J_bias_g / J_bias_a / J_gravity where they exist, pose, and w_b, alpha_b, v_w, a_w for inertial
cases (no sensor-block Jacobians: check_against_golden skips absent keys). One case per pattern and order (the bearing case at the interior
stamp) also carries G, dw, dal: K x 3 x 3 derivatives of the spline rotation (left perturbation), body angular rate and body angular
acceleration with respect to a world-frame perturbation Exp(phi_j) R_j, by central differences.

The file is the JSON of the other factor files, gzip-compressed (a megabyte of digits otherwise; written with mtime 0, so byte for byte
reproducible).
Run:  python tests/golden/make_degenerate_golden.py [processes]   (deterministic; half a minute on 8 processes)
"""
import gzip
import json
import multiprocessing
import os
import sys

import mpmath as mp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (sets mp.mp.dps = 100)
from make_golden import RES, SplitMix64, body_rates, jacobian, qconj, qexp, qlog, qmul, spline_pose, tofloat  # noqa: E402

PI = mp.pi
# name -> (relative angles in rad, cycled to K - 1 values; control points whose quaternion is negated)
PATTERNS = {
    "zero": ([0], ()),
    "tiny": (["1e-9"], ()),
    "log_series": (["1.9e-8", "2.1e-8", "1e-8", "4e-8", "2e-8"], ()),     # both sides of n2 = 1e-16
    "exp_series": (["2e-5", "3e-5", "5e-5", "8e-5", "2.5e-5"], ()),       # both sides of a2 = 1e-10 once multiplied by lam_j
    "below_t2": (["0.99e-4"], ()),
    "above_t2": (["1.01e-4"], ()),
    "mixed": ([0, "0.3", "1e-6", "1e-4", "0.2"], ()),
    "flip": (["0.1", "0.2", "0.15", "0.1", "0.2"], (1, 3)),
    "flip_small": (["1e-9", 0, "1e-5", "1e-4", 0], (1, 2)),
    "near_pi_flip": (["0.1", PI - mp.mpf("1e-2"), "0.2", PI - mp.mpf("1e-3"), "0.1"], (2,)),
    "unit_ulp": (["0.1", "1e-5", "0.15", 0, "0.2"], ()),                  # each quaternion scaled by 1 + m 2^-52, m in -3 .. 3
}
STAMP_VARIANTS = ("zero", "above_t2", "flip")  # also at the u0 and u1 stamps
PRIOR_SMALL = ("1e-9", "0.99e-4", "1.01e-4")   # prior_small: measurement rotation this far from the predicted sensor rotation
ORDERS = (4, 5, 6)
FACTORS = ("pixel", "bearing", "prior", "inertial")


def rand_axis(rng):
    while True:
        a = [mp.mpf(rng.uniform(lo=-1.0, hi=1.0)) for _ in range(3)]
        n = mp.sqrt(sum(x * x for x in a))
        if n > mp.mpf("0.1") and n <= 1:
            return [x / n for x in a]


def control_points(k, pattern, rng):
    angles, flip = PATTERNS[pattern]
    q = mg.rand_quat(rng)
    rows = []
    for j in range(k):
        if j > 0:
            ang = mp.mpf(angles[(j - 1) % len(angles)])
            axis = rand_axis(rng)
            q = qmul(q, qexp([ang * x for x in axis]))
        rows.append(list(q) + [mp.mpf(rng.uniform(lo=-1.0, hi=1.0)) for _ in range(3)])
    for j in flip:
        if j < k:
            rows[j][:4] = [-x for x in rows[j][:4]]
    if pattern == "unit_ulp":
        for j in range(k):
            m = (-3, 2, -1, 3, 1, -2)[j]
            rows[j][:4] = [mp.mpf(float(x)) * (1 + m * mp.mpf(2) ** -52) for x in rows[j][:4]]
    return rows


def plan():
    """[(index, ftype, k, pattern, variant, prior angle or None, with spline derivatives)] in the order of the file."""
    out = []
    for pattern in PATTERNS:
        for k in ORDERS:
            for ftype in FACTORS:
                for variant in (None,) + (("u0", "u1") if pattern in STAMP_VARIANTS else ()):
                    out.append((ftype, k, pattern, variant, None, ftype == "bearing" and variant is None))
    for pattern in ("zero", "regular"):
        for k in ORDERS:
            for ang in PRIOR_SMALL:
                out.append(("prior", k, pattern, "prior_small", ang, False))
    return [(i,) + c for i, c in enumerate(out)]


def to_mp(P):
    return {key: ([[mp.mpf(x) for x in r] for r in v] if isinstance(v, list) and isinstance(v[0], list)
                  else ([mp.mpf(x) for x in v] if isinstance(v, list) else (mp.mpf(v) if isinstance(v, float) else v)))
            for key, v in P.items()}


def make_inputs(index, ftype, k, pattern, variant, prior_angle):
    rng = SplitMix64(0x48595045 ^ (0xDE6E0000 + index))  # a stream per case: a case keeps its values when the plan grows
    cps = None if pattern == "regular" else control_points(k, pattern, rng)
    P = mg.make_case(ftype, k, rng, variant if variant in ("u0", "u1") else None, control_points=cps)
    if variant == "prior_small":  # R_m = R_ws Exp(-angle axis): Log(R_m^T R_ws) has this angle (the so3_coef branch of prior_linearize)
        P = to_mp({key: (tofloat(v) if not isinstance(v, int) else v) for key, v in P.items()})
        qw, _ = spline_pose(P["cps"], k, P["stamp"])
        axis = rand_axis(rng)
        P["meas"][:4] = qmul(qmul(qw, P["T_bs"][:4]), qexp([-mp.mpf(prior_angle) * x for x in axis]))
    return {key: (tofloat(v) if not isinstance(v, int) else v) for key, v in P.items()}


def spline_derivatives(cps, k, t):
    """G, dw, dal [j][row][col]: d (theta, w_b, alpha_b) / d phi_j for R_j <- Exp(phi_j) R_j; theta is the left perturbation of R(t)."""
    h = mg.H
    G, dw, dal = [], [], []
    for j in range(k):
        cols = []
        for c in range(3):
            side = []
            for s in (1, -1):
                phi = [mp.mpf(0)] * 3
                phi[c] = s * h
                Q = [list(r) for r in cps]
                Q[j][:4] = qmul(qexp(phi), cps[j][:4])
                q, _ = spline_pose(Q, k, t)
                w, al, _, _ = body_rates(Q, k, t)
                side.append((q, w, al))
            (qp, wp, ap), (qm, wm, am) = side
            th = qlog(qmul(qp, qconj(qm)))
            cols.append(([x / (2 * h) for x in th], [(a - b) / (2 * h) for a, b in zip(wp, wm)], [(a - b) / (2 * h) for a, b in zip(ap, am)]))
        for dst, n in ((G, 0), (dw, 1), (dal, 2)):
            dst.append([[tofloat(cols[c][n][r]) for c in range(3)] for r in range(3)])
    return G, dw, dal


def compute(job):
    index, ftype, k, pattern, variant, prior_angle, with_spline = job
    P = make_inputs(index, ftype, k, pattern, variant, prior_angle)
    Pm = to_mp(P)
    out = {"r": tofloat(RES[ftype](Pm))}
    Js = [[] for _ in out["r"]]
    for j in range(k):
        Jr = jacobian(ftype, Pm, ("cp_rot", j), 3)
        Jt = jacobian(ftype, Pm, ("cp_trans", j), 3)
        for r in range(len(out["r"])):
            Js[r] += tofloat(Jr[r]) + tofloat(Jt[r])
    out["J_state"] = Js
    if ftype in ("pixel", "bearing"):
        out["J_landmark"] = tofloat(jacobian(ftype, Pm, ("landmark", 0), 3))
    if ftype == "inertial":
        Jg, Ja = [[] for _ in range(6)], [[] for _ in range(6)]
        for j in range(P["kb"]):
            a = jacobian(ftype, Pm, ("bias_g", j), 3)
            b = jacobian(ftype, Pm, ("bias_a", j), 3)
            for r in range(6):
                Jg[r] += tofloat(a[r])
                Ja[r] += tofloat(b[r])
        out["J_bias_g"], out["J_bias_a"] = Jg, Ja
        out["J_gravity"] = tofloat(jacobian(ftype, Pm, ("gravity", 0), 2))
        w, al, v, a = body_rates(Pm["cps"], k, Pm["stamp"])
        out["w_b"], out["alpha_b"], out["v_w"], out["a_w"] = tofloat(w), tofloat(al), tofloat(v), tofloat(a)
    q, p = spline_pose(Pm["cps"], k, Pm["stamp"])
    out["pose"] = tofloat(q + p)
    if with_spline:
        w, al, _, _ = body_rates(Pm["cps"], k, Pm["stamp"])
        out["w_b"], out["alpha_b"] = tofloat(w), tofloat(al)
        out["G"], out["dw"], out["dal"] = spline_derivatives(Pm["cps"], k, Pm["stamp"])
    case = {"type": ftype, "variant": variant, "pattern": pattern, "inputs": P, "outputs": out}
    if prior_angle is not None:
        case["prior_angle"] = float(prior_angle)
    print(index, ftype, k, pattern, variant, "ok", flush=True)
    return case


def main():
    jobs = plan()
    nproc = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    with multiprocessing.Pool(nproc) as pool:
        cases = pool.map(compute, jobs, chunksize=1)
    text = json.dumps({"generator": "tests/golden/make_degenerate_golden.py (mpmath, 100 digits)", "cases": cases}, indent=None, separators=(",", ":"))
    with open(os.path.join(HERE, "factors_degenerate.json.gz"), "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, compresslevel=9, mtime=0) as z:
            z.write(text.encode())
    print("wrote", len(cases), "cases,", len(text), "bytes of JSON")


if __name__ == "__main__":
    main()
