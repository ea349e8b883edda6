"""Analytic test images for the KLT front-end (tests/test_klt_*.py, tests/test_gpu_klt.py): a smooth texture evaluated exactly at each
pixel and quantised to uint8, seen through sub-pixel translations, small affine warps and a stereo pair moving over a textured plane.
Not a test module: pytest does not collect it (no test_ prefix)."""
from __future__ import annotations

import numpy as np

WIDTH, HEIGHT = 752, 480
FX = FY = 458.0
CX, CY = 367.0, 248.0
BASELINE = 0.11      # camera 1 sits at +x of camera 0, same orientation
PLANE_Z = 3.0        # the textured plane z = PLANE_Z in the world frame


class Texture:
    """f(u, v): low-frequency sinusoids plus Gaussian blobs, values in [0, 255]; (u, v) in texture units (pixels for the 2-D tests)."""

    def __init__(self, seed=0, extent=1000.0, n_waves=24, n_blobs=48, min_wavelength=9.0, max_wavelength=60.0, blob_sigma=(3.0, 9.0)):
        rng = np.random.default_rng(seed)
        ang = rng.uniform(0, np.pi, n_waves)
        lam = rng.uniform(min_wavelength, max_wavelength, n_waves)
        self.k = np.stack([np.cos(ang), np.sin(ang)], -1) * (2 * np.pi / lam)[:, None]
        self.phase = rng.uniform(0, 2 * np.pi, n_waves)
        self.amp = rng.uniform(0.5, 1.0, n_waves) / np.sqrt(n_waves)
        self.c = rng.uniform(-0.1 * extent, 1.1 * extent, (n_blobs, 2))
        self.s = rng.uniform(blob_sigma[0], blob_sigma[1], n_blobs) * extent / 1000.0 * 10
        self.b = rng.uniform(-1.0, 1.0, n_blobs)
        self.extent = extent

    def __call__(self, u, v):
        u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
        out = np.zeros(np.broadcast(u, v).shape)
        for k, ph, a in zip(self.k, self.phase, self.amp):
            out += a * np.sin(k[0] * u + k[1] * v + ph)
        for c, s, b in zip(self.c, self.s, self.b):
            out += b * np.exp(-((u - c[0]) ** 2 + (v - c[1]) ** 2) / (2 * s * s))
        return out


def quantise(vals):
    return np.clip(np.rint(127.5 + 60.0 * vals), 0, 255).astype(np.uint8)


def image(tex, w, h, A=np.eye(2), t=(0.0, 0.0)):
    """Pixel (x, y) shows the texture at A (x, y) + t."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    u = A[0, 0] * x + A[0, 1] * y + t[0]
    v = A[1, 0] * x + A[1, 1] * y + t[1]
    return quantise(tex(u, v))


def tie_image(w, h, period=8):
    """A repeated pattern: many corners of exactly equal response (the raster-index tie rule of the corner order)."""
    y, x = np.mgrid[0:h, 0:w]
    return np.where(((x // period) + (y // period)) % 2 == 0, 40, 210).astype(np.uint8)


def camera_position(k):
    """World position of camera 0 at frame k (orientation = identity: looking along +z at the plane)."""
    return np.array([0.004 * k + 0.0005 * k * k, 0.002 * np.sin(0.3 * k), 0.003 * k])


class StereoPlane:
    """A stereo pair with EuRoC-like intrinsics over the textured plane z = PLANE_Z; the texture is parameterised in millimetres."""

    def __init__(self, seed=0, w=WIDTH, h=HEIGHT):
        self.tex = Texture(seed, extent=3000.0, min_wavelength=55.0, max_wavelength=300.0)
        self.w, self.h = w, h

    def render(self, cam):
        y, x = np.mgrid[0:self.h, 0:self.w].astype(np.float64)
        depth = PLANE_Z - cam[2]
        X = cam[0] + (x - CX) / FX * depth
        Y = cam[1] + (y - CY) / FY * depth
        return quantise(self.tex(1000.0 * X, 1000.0 * Y))

    def frame(self, k):
        c0 = camera_position(k)
        return self.render(c0), self.render(c0 + np.array([BASELINE, 0.0, 0.0]))

    @staticmethod
    def backproject(px, k):
        """Plane point seen at left pixel px in frame k."""
        c = camera_position(k)
        depth = PLANE_Z - c[2]
        return np.stack([c[0] + (px[:, 0] - CX) / FX * depth, c[1] + (px[:, 1] - CY) / FY * depth, np.full(len(px), PLANE_Z)], -1)

    @staticmethod
    def project(P, k, right=False):
        c = camera_position(k) + (np.array([BASELINE, 0.0, 0.0]) if right else 0.0)
        d = P - c
        return np.stack([FX * d[:, 0] / d[:, 2] + CX, FY * d[:, 1] / d[:, 2] + CY], -1)
