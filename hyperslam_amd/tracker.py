"""Host-side handle of the stereo KLT front-end (hs_tracker_* of include/hyperslam_hip.h): HyperSLAM's VisualFrontend on the GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import TrackerOptions
from .problem import HsError

_f = C.POINTER(C.c_float)


def _u8(a):
    return a.ctypes.data_as(_lib.c_uint8_p)


def _fp(a):
    return a.ctypes.data_as(_f)


class Tracker:
    """Tracker(width, height, device=0, **options); options are the fields of hs_tracker_options (max_num_tracks, patch_size, ...)."""

    def __init__(self, width: int, height: int, device: int = 0, lib: _lib.Library | None = None, **options):
        self.lib = lib if lib is not None else _lib.load()
        self.width, self.height = int(width), int(height)
        o = TrackerOptions()
        self.lib.tracker_default_options(C.byref(o))
        for k, v in options.items():
            if not hasattr(o, k) or k == "reserved":
                raise TypeError(f"unknown tracker option {k!r}")
            setattr(o, k, v)
        self.options = o
        h = C.c_void_p()
        rc = self.lib.tracker_create(device, None, self.width, self.height, C.byref(o), C.byref(h))
        if rc != 0 or not h:
            raise HsError(f"hs_tracker_create failed with code {rc} (invalid options or no usable GPU)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.tracker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc, what):
        if rc != 0:
            msg = self.lib.tracker_last_error(self.h)
            raise HsError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")

    def _image(self, img):
        a = np.ascontiguousarray(img, np.uint8)
        if a.shape != (self.height, self.width):
            raise ValueError(f"image of shape {a.shape}, tracker is {(self.height, self.width)}")
        return a

    def level_sizes(self, n_levels):
        w, h, out = self.width, self.height, []
        for _ in range(n_levels):
            out.append((h, w))
            w, h = (w + 1) // 2, (h + 1) // 2
        return out

    def build_pyramid(self, image):
        """([level arrays (h_l, w_l) uint8], [derivatives (h_l, w_l, 2) int16])."""
        img = self._image(image)
        n = C.c_int32()
        self._check(self.lib.tracker_build_pyramid(self.h, _u8(img), C.byref(n), None, None), "hs_tracker_build_pyramid")
        sizes = self.level_sizes(n.value)
        total = sum(h * w for h, w in sizes)
        lv, dr = np.zeros(total, np.uint8), np.zeros(2 * total, np.int16)
        self._check(self.lib.tracker_build_pyramid(self.h, _u8(img), C.byref(n), _u8(lv), dr.ctypes.data_as(C.POINTER(C.c_int16))),
                    "hs_tracker_build_pyramid")
        levels, derivs, o = [], [], 0
        for h, w in sizes:
            levels.append(lv[o:o + h * w].reshape(h, w))
            derivs.append(dr[2 * o:2 * (o + h * w)].reshape(h, w, 2))
            o += h * w
        return levels, derivs

    def min_eigen(self, image):
        img = self._image(image)
        out = np.zeros((self.height, self.width), np.float32)
        self._check(self.lib.tracker_min_eigen(self.h, _u8(img), _fp(out)), "hs_tracker_min_eigen")
        return out

    def good_features(self, image, max_corners, quality, min_distance, mask=None):
        img = self._image(image)
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        cap = max_corners if max_corners > 0 else self.width * self.height
        out = np.zeros((cap, 2), np.float32)
        n = C.c_int32()
        self._check(self.lib.tracker_good_features(self.h, _u8(img), None if m is None else _u8(m), int(max_corners), float(quality),
                                                   float(min_distance), C.byref(n), _fp(out)), "hs_tracker_good_features")
        return out[:n.value].copy()

    def optical_flow(self, image0, image1, points, initial=None):
        """(points1 (n, 2) float32, status (n,) uint8)."""
        i0, i1 = self._image(image0), self._image(image1)
        p0 = np.ascontiguousarray(points, np.float32).reshape(-1, 2)
        n = len(p0)
        p1 = np.ascontiguousarray(initial, np.float32).reshape(-1, 2).copy() if initial is not None else np.zeros((n, 2), np.float32)
        if len(p1) != n:
            raise ValueError("initial must have one row per point")
        st = np.zeros(n, np.uint8)
        self._check(self.lib.tracker_optical_flow(self.h, _u8(i0), _u8(i1), n, _fp(p0), _fp(p1), _u8(st), int(initial is not None)),
                    "hs_tracker_optical_flow")
        return p1, st

    def process(self, stamp, left, right):
        """None on the first call after creation / reset, else the previous frame's message {stamp, ids, lengths, pixels0, pixels1}."""
        l, r = self._image(left), self._image(right)
        cap = int(self.options.max_num_tracks)
        has, n, ms = C.c_int32(), C.c_int32(), C.c_double()
        ids, lengths = np.zeros(cap, np.int64), np.zeros(cap, np.int32)
        p0, p1 = np.zeros((cap, 2), np.float32), np.zeros((cap, 2), np.float32)
        self._check(self.lib.tracker_process(self.h, float(stamp), _u8(l), _u8(r), C.byref(has), C.byref(ms), C.byref(n),
                                             ids.ctypes.data_as(C.POINTER(C.c_int64)), lengths.ctypes.data_as(_lib.c_int32_p), _fp(p0), _fp(p1)),
                    "hs_tracker_process")
        if not has.value:
            return None
        k = n.value
        return dict(stamp=ms.value, ids=ids[:k].copy(), lengths=lengths[:k].copy(), pixels0=p0[:k].copy(), pixels1=p1[:k].copy())

    def reset(self):
        self._check(self.lib.tracker_reset(self.h), "hs_tracker_reset")
