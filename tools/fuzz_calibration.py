"""Randomised sweep of the free-camera build and solve, HIP against the numpy referees (TEST TOOLING): the windows of
tests/calibration_windows.py::cases — spline order, length, band width, pixel / bearing rows, IMU borders of varying size, priors, frozen
prefixes, constant landmarks, rotation- / translation-only splines, a random non-empty subset of the six camera blocks free. Per case:
hs_reduced_system against calibration_referee.reduced_system (1e-9, symmetric, two calls bit-identical), and — on the windows the acceptance
rule of calibration_windows.solve_acceptance takes, which consults the CPU only — solve(4) against calibration_solve_referee.solve at the bars of
tests/test_gpu_calibration_solve.py. Prints one line per case and the failures at the end; exit code = number of failures.
usage (GPU box): python tools/fuzz_calibration.py [cases=40] [seed=1]"""
import os
import sys

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
from hyperslam_amd import _lib

import calibration_referee
import calibration_windows as cw


def main():
    n_cases = int(sys.argv[1]) if len(sys.argv) > 1 else 40
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    hip = _lib.load()
    if os.environ.get("HS_GUARD") == "1":
        hip.set_guard(1)
    oracle = _lib.Library(os.path.join("oracle", "liboracle.so"), "hso_")
    failures, solved = [], 0
    for tag, w in cw.cases(n_cases, seed):
        note = ""
        try:
            cw.check_build(w, hip, calibration_referee.reduced_system(w, oracle, 1e4))
            ok, why, sr, wf = cw.solve_acceptance(w, oracle, 4)
            if ok:
                import contextlib
                import io
                with contextlib.redirect_stdout(io.StringIO()):
                    cw.check_solve(w, hip, sr, wf, 4, tag)
                solved += 1
            note = ("build + solve ok | " if ok else "build ok, solve left out | ") + why
        except Exception as e:
            note = f"<-- FAIL {type(e).__name__}: {str(e)[:300]}"
            failures.append((tag, note))
        print(tag, "|", note, flush=True)
    print(f"{n_cases} cases ({solved} solved), {len(failures)} failures, seed {seed}")
    for f in failures:
        print("FAILED", f)
    sys.exit(min(len(failures), 100))


if __name__ == "__main__":
    main()
