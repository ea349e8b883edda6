"""GPU tests: the fused build on the even split of the landmark groups and the dispatch order by records (host_structure.hpp:
build_chunks_balanced, order_chunks_by_records — what prepare() takes when no compute unit gets more than two chunks, as on these windows;
HS_BUILD_SPLIT=greedy selects the greedy fill and its pairing),
through the C ABI against the oracle, on small windows whose chunk limits (HS_BUILD_L) make the two splits differ: groups of
5 - 9 landmarks in chunks of at most 4 or 3, a landmark that fills a chunk's records on its own, frozen leading control points.
Tolerances: those of tests/test_gpu_build_stream_sums.py for the same quantities. The rules of the split themselves are pinned on the CPU
(tests/test_host_chunks_balanced.py)."""
import copy

import numpy as np
import pytest

import hyperslam_amd as ha
from hyperslam_amd import synthetic

pytestmark = pytest.mark.gpu


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-300, np.abs(np.asarray(b)).max())


def window_pixels():
    return synthetic.small_visual(order=4, n_cp=12, n_landmarks=60, obs_pairs=5)  # 600 pixel rows


def window_bearings():
    return synthetic.small_visual(order=6, n_cp=14, n_landmarks=40, obs_pairs=4, bearing=True)


def window_full_landmark():
    """Every tenth landmark keeps its 128 records (= R at order 4: a chunk of its own), the others keep their first six."""
    w = copy.copy(synthetic.small_visual(order=4, n_cp=12, n_landmarks=60, obs_pairs=64))
    nth = np.zeros(len(w.pixel_stamps), np.int64)  # position of the row among the rows of its landmark
    seen = {}
    for i, l in enumerate(w.pixel_landmark):
        nth[i] = seen.get(int(l), 0)
        seen[int(l)] = nth[i] + 1
    assert max(seen.values()) == 128
    m = (w.pixel_landmark % 10 == 0) | (nth < 6)
    w.pixel_stamps, w.pixels, w.pixel_landmark, w.pixel_camera = w.pixel_stamps[m], w.pixels[m], w.pixel_landmark[m], w.pixel_camera[m]
    return w


def window_frozen():
    w = window_pixels()
    w.cp_constant = np.r_[np.ones(4, np.uint8), np.zeros(8, np.uint8)]
    return w


WINDOWS = {
    "pixels_k4_L4": (window_pixels, {"HS_BUILD_L": "4"}),
    "bearings_k6_L3": (window_bearings, {"HS_BUILD_L": "3"}),
    "full_landmark_R128": (window_full_landmark, {"HS_BUILD_L": "4"}),
    "frozen_k4_L4": (window_frozen, {"HS_BUILD_L": "4"}),
}
_oracle_results = {}


def run_window(w, lib):
    """Reduced system and gradient at the start point, then the state after solve(5), of a fresh handle."""
    with ha.Problem(w, lib=lib) as p:
        S, g = p.reduced_system(1e4)
        s = p.solve(5)
        return dict(S=S, g=g, summary=s, cp=p.control_points(), lm=p.landmarks())


def oracle_result(name, oracle):
    if name not in _oracle_results:
        _oracle_results[name] = run_window(WINDOWS[name][0](), oracle)
    return _oracle_results[name]


def check_against(got, ref, name):
    """The bounds of tests/test_gpu_build_stream_sums.py."""
    assert rel(got["S"], ref["S"]) < 1e-9, rel(got["S"], ref["S"])
    assert rel(got["g"], ref["g"]) < 1e-9, rel(got["g"], ref["g"])
    sg, sc = got["summary"], ref["summary"]
    assert sg["num_iterations"] == sc["num_iterations"] and sg["termination"] == sc["termination"]
    for ig, ic in zip(sg["iterations"], sc["iterations"]):
        assert ig["step_is_successful"] == ic["step_is_successful"]
        assert abs(ig["cost"] - ic["cost"]) <= 1e-6 * abs(ic["cost"]) + 1e-8 * sc["initial_cost"], (name, ig["iteration"], ig["cost"], ic["cost"])
    assert rel(got["cp"], ref["cp"]) < 1e-6
    assert rel(got["lm"], ref["lm"]) < 1e-6


@pytest.fixture
def geometry(request, monkeypatch):
    """The chunk limits of the window, set before any handle of the test is created; the fused build everywhere."""
    monkeypatch.setenv("HS_BUILD_PATH", "fused")
    monkeypatch.delenv("HS_BUILD_SPLIT", raising=False)
    for key, value in WINDOWS[request.param][1].items():
        monkeypatch.setenv(key, value)
    return request.param


by_window = pytest.mark.parametrize("geometry", list(WINDOWS), indirect=True)


@by_window
def test_balanced_split_against_oracle(geometry, hip, oracle):
    got = run_window(WINDOWS[geometry][0](), hip)
    assert np.array_equal(got["S"], got["S"].T)
    check_against(got, oracle_result(geometry, oracle), geometry)


@by_window
def test_two_handles_bit_identical(geometry, hip):
    a, b = run_window(WINDOWS[geometry][0](), hip), run_window(WINDOWS[geometry][0](), hip)
    for key in ("S", "g", "cp", "lm"):
        assert np.array_equal(a[key], b[key]), key
    assert [it["cost"] for it in a["summary"]["iterations"]] == [it["cost"] for it in b["summary"]["iterations"]]


@by_window
def test_greedy_switch_agrees(geometry, hip, oracle, monkeypatch):
    balanced = run_window(WINDOWS[geometry][0](), hip)
    monkeypatch.setenv("HS_BUILD_SPLIT", "greedy")
    greedy = run_window(WINDOWS[geometry][0](), hip)
    check_against(greedy, oracle_result(geometry, oracle), geometry)
    check_against(balanced, greedy, geometry)
    # other chunk boundaries are other partial sums: on these windows the two splits differ, and so do the last bits
    assert not (np.array_equal(balanced["S"], greedy["S"]) and np.array_equal(balanced["g"], greedy["g"]))
