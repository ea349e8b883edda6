"""The host emulator's wave primitives (tests/emul/hip/hip_runtime.h) against their statement in tests/primitive_models.py, bit for bit.

tests/device/primitives_probe.hpp — one kernel that calls the product's spelling of every primitive (DPP moves and sums of kernels_common.hpp,
the row broadcasts and ordered f64 statements of dpp_f64.hpp, pair_sum of kernels_backward_sb.hpp, __shfl_xor / __shfl_up / readlane / __ballot,
the f64 MFMA, rsq) — is compiled for the host (tests/emul/primitives_harness.cpp) and run with one thread per lane.
tests/test_gpu_primitives.py holds the same kernel, compiled for gfx950, against the same model: together they say that what the emulated
suites compute lane by lane is what the hardware computes. The rsq estimate is compared with the emulator's own statement: the correctly
rounded value off by kRsqRelErr, sign from the lowest mantissa bit of the argument."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import primitive_models as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path_factory.mktemp("emul_primitives") / "primitives_harness")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-Wno-psabi", "-I", EMUL, "-o", exe, os.path.join(EMUL, "primitives_harness.cpp")])
    return exe


def run(exe, tmp_path, family, x, threads):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(x, dtype="<f8").tofile(src)
    subprocess.check_call([exe, str(family), str(threads), src, dst], timeout=120)
    return np.fromfile(dst, dtype="<f8")


@pytest.mark.parametrize("case", pm.CASES, ids=pm.case_id)
def test_probe_equals_model(case, harness, tmp_path):
    family, threads, integers = case
    x = pm.inputs(family, threads, integers)
    pm.assert_probe_equals_model(family, x, run(harness, tmp_path, family, x, threads), threads)


def test_rsq_is_the_stated_estimate(harness, tmp_path):
    """Both spellings (__builtin_amdgcn_rsq, dx_rsq) equal the stated model on the sweep and the specials, and the model is what it says: off
    by kRsqRelErr (never below the 2^-24 the kernels' comments claim for the hardware), to either side, and a function of the argument alone."""
    eps = pm.emulator_rsq_epsilon()
    assert eps >= 2.0 ** -24 and np.log2(eps) == round(np.log2(eps))
    sweep = pm.rsq_sweep()  # (evenly spaced mantissas: the lowest bit clear; their upper neighbours have it set)
    d = np.r_[sweep, np.nextafter(sweep, np.inf), pm.RSQ_SPECIALS]
    got = run(harness, tmp_path, pm.RSQ, d, 256).reshape(2, len(d))
    want = pm.emulator_rsq(d)
    assert pm.same_bits(got[0], want) and pm.same_bits(got[1], want)
    n = len(d) - len(pm.RSQ_SPECIALS)
    err = (np.asarray(got[0][:n], np.longdouble) * np.sqrt(np.asarray(d[:n], np.longdouble)) - 1.0).astype(float)
    print("emulated rsq: relative error %.4g .. %.4g of eps = 2^%d" % (err.min() / eps, err.max() / eps, round(np.log2(eps))))
    assert err.min() < -0.99 * eps and err.max() > 0.99 * eps and np.abs(err).max() < 1.01 * eps
    specials = dict(zip(pm.RSQ_SPECIAL_NAMES, got[0][n:]))
    assert specials["+0"] == np.inf and specials["-0"] == -np.inf and np.isnan(specials["-1"]) and np.isnan(specials["nan"]) and specials["+inf"] == 0.0
    # the same argument in two lanes of one launch and in two launches: the same bits (the panels compute a pivot redundantly in several lanes)
    twice = run(harness, tmp_path, pm.RSQ, np.r_[d[:n][::-1], d[:n]], 96).reshape(2, 2 * n)
    assert pm.same_bits(twice[0][:n][::-1], got[0][:n]) and pm.same_bits(twice[0][n:], got[0][:n])


def test_harness_refuses_sizes_that_are_not_the_family_s(harness, tmp_path):
    src = str(tmp_path / "in.bin")
    np.zeros(255).tofile(src)
    assert subprocess.run([harness, str(pm.DPP), "256", src, str(tmp_path / "out.bin")], capture_output=True).returncode == 3
