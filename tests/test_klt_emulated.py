"""The front-end kernels (hyperslam_amd/csrc/kernels_klt.hpp) compiled for the HOST through tests/emul/ (one thread per lane) and compared
with the numpy restatement (tests/klt_numpy.py) on small images: pyramid and derivatives bit for bit, the corner response bit for bit, the
corner list identical (ties included), Lucas-Kanade positions and statuses identical. The `-m gpu` tests (tests/test_gpu_klt.py) remain
the parity tests of the compiled kernels; this one makes their arithmetic and index work checkable without a GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import klt_numpy as K
import klt_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL = os.path.join(ROOT, "tests", "emul")
W, H = 160, 120


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    d = tmp_path_factory.mktemp("emul_klt")
    exe = str(d / "klt_harness")
    subprocess.check_call(["g++", "-std=c++20", "-O1", "-pthread", "-Wno-psabi", "-I", EMUL, "-o", exe, os.path.join(EMUL, "klt_harness.cpp")])

    def run(mode, payload):
        i, o = str(d / "in.bin"), str(d / "out.bin")
        with open(i, "wb") as f:
            f.write(payload)
        subprocess.check_call([exe, mode, i, o], timeout=600)
        with open(o, "rb") as f:
            return f.read()
    return run


def test_pyramid_and_derivatives(harness):
    for w, h in ((W, H), (W - 1, H - 3)):
        img = S.image(S.Texture(11), w, h, t=(2.2, 0.4))
        out = harness("pyr", struct.pack("4i", w, h, 7, 2) + img.tobytes())
        levels, derivs = K.build_pyramid(img, 2, 7)
        n = struct.unpack_from("i", out)[0]
        assert n == len(levels) == 3
        o = 4
        for l in levels:
            assert np.array_equal(np.frombuffer(out, np.uint8, l.size, o).reshape(l.shape), l)
            o += l.size
        for d in derivs:
            assert np.array_equal(np.frombuffer(out, np.int16, d.size, o).reshape(d.shape), d)
            o += 2 * d.size


def test_response(harness):
    img = S.image(S.Texture(12), W, H)
    out = np.frombuffer(harness("eig", struct.pack("2i", W, H) + img.tobytes()), np.float32).reshape(H, W)
    assert np.array_equal(out.view(np.uint32), K.min_eigen(img).view(np.uint32))


@pytest.mark.parametrize("case", ["texture", "mask", "ties", "ties_limited"])
def test_good_features(harness, case):
    img = S.tie_image(W, H, period=6) if case.startswith("ties") else S.image(S.Texture(13), W, H)
    yy, xx = np.mgrid[0:H, 0:W]
    mask = ((xx - 80) ** 2 + (yy - 60) ** 2 > 30 ** 2).astype(np.uint8) if case == "mask" else None
    mc, md = {"texture": (0, 5), "mask": (40, 8), "ties": (0, 1), "ties_limited": (70, 4)}[case]
    payload = struct.pack("2i", W, H) + img.tobytes() + struct.pack("2i2d", mask is not None, mc, 0.01, md)
    if mask is not None:
        payload += mask.tobytes()
    out = harness("gft", payload)
    n = struct.unpack_from("i", out)[0]
    got = np.frombuffer(out, np.float32, 2 * n, 4).reshape(n, 2)
    ref = K.good_features(img, mc, 0.01, md, mask)
    assert len(ref) > 10 and np.array_equal(got, ref)


@pytest.mark.parametrize("use_init", [False, True])
def test_optical_flow(harness, use_init):
    tex = S.Texture(14)
    img0, img1 = S.image(tex, W, H), S.image(tex, W, H, t=(-3.7, 2.2))
    rng = np.random.default_rng(5)
    pts = np.vstack([np.stack([rng.uniform(0, W, 24), rng.uniform(0, H, 24)], -1), [[-4, 50], [W + 2, 10], [2, H - 1]]]).astype(np.float32)
    init = (pts + np.array([3.0, -2.0], np.float32)).astype(np.float32)
    payload = struct.pack("6i", W, H, 7, 2, len(pts), int(use_init)) + img0.tobytes() + img1.tobytes() + pts.tobytes()
    if use_init:
        payload += init.tobytes()
    out = harness("flow", payload)
    got = np.frombuffer(out, np.float32, 2 * len(pts)).reshape(-1, 2)
    st = np.frombuffer(out, np.uint8, len(pts), 8 * len(pts))
    ref, rs = K.optical_flow(K.build_pyramid(img0, 2, 7), K.build_pyramid(img1, 2, 7), pts, init if use_init else None, patch=7)
    assert np.array_equal(st, rs) and 0 < rs.sum() < len(rs)
    assert np.array_equal(got, ref)
