"""CPU tests (no GPU): the stream sums of the fused build's J_p'J_p phase (hyperslam_amd/csrc/kernels_build.hpp, phase 3) are a fixed tree of
additions, ((s0 + s1) + (s2 + s3)) + ... over the record streams of a tile. The kernel evaluates the tree by recursive halving — every level
halves the values a lane still holds, and the finished tile is written by all lanes of its group — where it used to run butterflies over all 42
values of every lane. The operands of every addition are the same pairs, so the emulated build must reproduce, BIT FOR BIT, what the butterfly
version delivered: tests/golden/build_streams.npz, recorded by tests/golden/make_build_streams_golden.py with a harness compiled from the
sources before the change. The windows reach one, two, four, eight and sixteen streams per tile, uneven groups inside one wave included."""
import os
import sys

import numpy as np
import pytest

from hyperslam_amd import synthetic
import test_emulated_build as teb
from test_emulated_build import harness  # noqa: F401  (the session fixture that compiles the harness)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
sys.path.insert(0, GOLDEN)
from make_build_streams_golden import WINDOWS  # noqa: E402


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(GOLDEN, "build_streams.npz"))


@pytest.mark.parametrize("name,wkw,rkw", WINDOWS, ids=[w[0] for w in WINDOWS])
def test_emulated_build_stream_sums_bit_identical(harness, recorded, name, wkw, rkw):  # noqa: F811
    out = teb.run_emulated_build(harness, synthetic.small_visual(**wkw), **rkw)
    for key in ("S", "g", "Y"):
        want = recorded[name + "." + key]
        assert out[key].shape == want.shape, (key, out[key].shape, want.shape)
        # (compared as bit patterns: a zero of the other sign counts as a difference)
        differ = out[key].view(np.uint64) != want.view(np.uint64)
        assert not differ.any(), (key, int(differ.sum()), float(np.abs(out[key] - want).max()))
