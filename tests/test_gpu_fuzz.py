"""Randomised parity sweeps in the driver's suite (`-m gpu`): window shapes the fixed tests do not enumerate, NEW ones whenever the kernels change.

tools/fuzz_parity.py (HIP against the oracle on random windows: spline order, length, band width 4 .. window-wide, IMU, frozen prefixes, constant
landmarks, priors, rotation- / translation-only) and tools/fuzz_shards.py (two landmark shards under torch.distributed against the single-process
solve) run as subprocesses under HS_GUARD=1 (every device table at its exact size with a checked pattern behind it). The seed is a hash of the
kernel sources — the GPU box has no .git, and a round that changes a kernel gets shapes no earlier round has seen. Round 5 found two
out-of-bounds writes this way that four rounds of fixed tests had not; those sweeps were builder-run, these are not.

The free-camera build and solve have sweeps of their own, in process and under the suite's guard mode: windows of
tests/calibration_windows.py::cases against the numpy referees (tools/fuzz_calibration.py runs the same comparisons for longer sweeps)."""
import hashlib
import os
import subprocess
import sys

import pytest

import calibration_windows as cw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_seed():
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "hyperslam_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name), "rb") as f:
            h.update(f.read())
    return int(h.hexdigest()[:6], 16) + 1


def run(cmd, timeout):
    env = dict(os.environ, HS_GUARD="1", MASTER_ADDR="127.0.0.1")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)
    return out.returncode, out.stdout, out.stderr


@pytest.mark.gpu
def test_random_windows_against_the_oracle():
    """270 windows of up to 150 control points + 30 of BASELINE size (100 .. 512 control points, 500 .. 5 000 landmarks), bars of
    tests/test_gpu_edge_cases.py::compare; the long-double oracle referees ill-conditioned windows by the rule written in tools/fuzz_parity.py."""
    seed = source_seed()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tools", "fuzz_parity.py"), str(n), str(seed + i)] + extra, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT, text=True, cwd=ROOT, env=dict(os.environ, HS_GUARD="1"))
             for i, (n, extra) in enumerate(((135, []), (135, []), (30, ["large"])))]
    for p, n in zip(procs, (135, 135, 30)):
        out, _ = p.communicate(timeout=1500)
        assert p.returncode == 0 and f"{n} cases, 0 failures" in out, f"seed {seed}\n" + out[-3000:]


@pytest.mark.gpu
def test_random_windows_on_two_shards():
    """100 random windows sharded by landmark over two ranks (gloo hook, one GPU) against the single-process solve."""
    seed = source_seed()
    rc, out, err = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29533",
                        os.path.join(ROOT, "tools", "fuzz_shards.py"), "100", str(seed)], 1500)
    assert rc == 0 and "100 cases on 2 ranks, 0 failures" in out, f"seed {seed}\n" + out[-3000:] + err[-1500:]


@pytest.fixture(params=["fused", "records"])
def build_path(request, monkeypatch):
    monkeypatch.setenv("HS_BUILD_PATH", request.param)
    return request.param


@pytest.fixture(scope="module")
def build_cases(oracle):
    """(seed, [(description, window, referee's reduced system)]): computed once, shared by both build paths."""
    import calibration_referee
    seed = source_seed()
    return seed, [(tag, w, calibration_referee.reduced_system(w, oracle, 1e4)) for tag, w in cw.cases(24, seed)]


@pytest.fixture(scope="module")
def solve_cases(oracle):
    """(seed, draws, [(description, window, referee's summary, referee's end point)]): candidates of the generator in order until ten are accepted."""
    seed = source_seed() + 1
    taken, draws = [], 0
    for tag, w in cw.cases(30, seed):
        draws += 1
        ok, why, sr, wf = cw.solve_acceptance(w, oracle, 4)
        print(("take " if ok else "leave") + " " + tag + " | " + why)
        if ok:
            taken.append((tag, w, sr, wf))
        if len(taken) == 10:
            break
    return seed, draws, taken


@pytest.mark.gpu
def test_random_camera_windows_build(hip, build_cases, build_path):
    """24 windows of tests/calibration_windows.py::cases (free camera blocks next to every other option of a window): hs_reduced_system against
    calibration_referee.reduced_system at 1e-9, symmetric, two calls bit-identical — the bars of test_reduced_system_against_referee.
    Wall time on an MI355X box: 0.5 s for the 24 referees (once), 0.5 s per build path."""
    seed, windows = build_cases
    for tag, w, reference in windows:
        try:
            cw.check_build(w, hip, reference)
        except Exception as e:
            raise AssertionError(f"seed {seed} ({build_path})\n{tag}\n{type(e).__name__}: {e}") from e


@pytest.mark.gpu
def test_random_camera_windows_solve(hip, solve_cases, build_path):
    """10 windows of the same generator (seed + 1): solve(4) estimating the free camera blocks against calibration_solve_referee.solve at the bars of
    check_trajectory / check_end_point. A candidate is taken by calibration_windows.solve_acceptance from CPU quantities alone (conditioning rule of
    test_solve_against_referee; no relative decrease of the referee's solve within 1e-3 of the decision threshold) — the device is never consulted.
    The test fails if 30 draws do not yield 10 windows. On the CPU, 68 seeds (1 .. 8, 1000 .. 1059) needed between 10 and 15 draws (worst case 15).
    Wall time on an MI355X box: 6 s for the referee's ten solves and the candidates' condition numbers (once, shared by both build paths), 0.2 s per path on the device."""
    seed, draws, windows = solve_cases
    assert len(windows) == 10, f"seed {seed}: only {len(windows)} of {draws} candidates accepted"
    for tag, w, sr, wf in windows:
        try:
            cw.check_solve(w, hip, sr, wf, 4, tag)
        except Exception as e:
            raise AssertionError(f"seed {seed} ({build_path})\n{tag}\n{type(e).__name__}: {e}") from e
