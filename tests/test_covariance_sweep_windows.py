"""The generator behind tests/test_gpu_covariance.py::test_random_windows, on the CPU: sweep_windows must hand check_window sixteen windows it
can pass, whatever the seed. The seed of the GPU test is a hash of the kernel sources, so a seed whose draw holds a window check_window cannot
take (no visual residual: no landmark block to compare; a band beyond the 42 control points the library takes) failed the GPU suite of whichever
change happened to hash to it. Those windows are left out as restrictions of the generator, next to the size limits; windows the numpy referee
finds rank deficient are replaced and counted, and the count has a cap.

Seeds here: 5491227, 9422553 and 106 drew a window without visual residuals among their first sixteen, 9097370 one with a band above 42 control
points, 129 is the seed with the most rank-deficient draws found before (20 replacements while windows without visual residuals still counted
among them, 15 now), and the seed of the kernel sources as they are.

The same four assertions over seeds 1 .. 300 and 1000 .. 1059, run once on the CPU (not part of the suite: ~3 s a seed): all 360 seeds pass; the
replacements are 0 .. 16 (mean 5.3), the worst count 16 at seed 274, half of the cap of 32."""
import numpy as np
import pytest

from calibration_windows import MAX_BAND, band_blocks
from test_gpu_covariance import MAX_REPLACEMENTS, sweep_windows
from test_gpu_fuzz import source_seed


def check_seed(seed, oracle):
    windows, replaced = sweep_windows(seed, oracle)
    print(f"seed {seed}: {len(windows)} windows, {replaced} replacements, bands {[band_blocks(w) for _, w in windows]}")
    assert len(windows) == 16
    assert replaced <= MAX_REPLACEMENTS == 32
    for tag, w in windows:
        assert len(w.pixel_stamps) + len(w.bearing_stamps) > 0, tag
        assert len(w.landmarks) > 0, tag
        assert band_blocks(w) <= MAX_BAND == 42, tag
    return windows, replaced


@pytest.mark.parametrize("seed", [5491227, 9422553, 106, 9097370, 129, "source"])
def test_sweep_windows_are_passable(seed, oracle):
    check_seed(source_seed() if seed == "source" else seed, oracle)


def test_band_restatement_counts_control_points_of_a_track():
    """band_blocks on a window whose band is known by construction (tests/test_gpu_covariance.py::test_band_at_the_limit asserts the device's
    own figure for the same window on the GPU: 36 .. 42)."""
    from hyperslam_amd import synthetic
    w = synthetic.small_visual(order=4, n_cp=44, n_landmarks=60, obs_pairs=8, seed=41, span=3.75)
    assert 36 <= band_blocks(w) <= 42
