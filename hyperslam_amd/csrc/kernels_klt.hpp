// kernels_klt.hpp — the stereo KLT front-end on the device (hs_tracker_*, tracker.hpp; part of kernels.hpp, included once by capi.hip).
//
// What VisualFrontend (HyperSLAM's klt.cpp) asks of OpenCV, restated with exact integer sums (DESIGN.md "Front-end: stereo KLT on the
// device"; tests/klt_numpy.py is the same arithmetic in numpy and the tests compare bit for bit). Parity with OpenCV itself is unpinned.
//   k_klt_pyramid    one launch per level for one or two images (gridDim.z): padded level L (pyrDown of L-1, REFLECT_101 border) and the
//                    Scharr derivatives of level L-1 (zero border)
//   k_klt_flow       pyramidal Lucas-Kanade, one wave per point, up to four independent passes per launch (gridDim.y)
//   k_klt_min_eigen  Shi-Tomasi response (Sobel 3, block 3) + the maximum over the mask (one atomic per wave)
//   k_klt_candidates threshold, 3x3 non-maximum test, mask -> 64-bit keys (response bits, raster index)
//   k_klt_rank       descending order of the keys by counting (every key is distinct)
//   k_klt_select     the exact sequential greedy of goodFeaturesToTrack (one workgroup, 64 candidates per step)
#pragma once
#include <cstdint>

namespace hs {

constexpr int kKltMaxLevels = 8;
constexpr int kKltMaxPatch = 31;                                          // 31 x 31 = 961 pixels: at most 16 per lane
constexpr int kKltPixPerLane = (kKltMaxPatch * kKltMaxPatch + 63) / 64;
constexpr int kKltWBits = 14;

/// Padded pyramid layout shared by every image of a tracker: level l starts at element off[l] of the image (uint8) and derivative (int16 x 2)
/// buffers; its content pixel (x, y) is element off[l] + (y + pad) * stride[l] + x + pad, stride[l] = w[l] + 2 pad, rows h[l] + 2 pad.
struct KltGeom {
  int n_levels, pad, patch, reserved;
  int w[kKltMaxLevels], h[kKltMaxLevels], stride[kKltMaxLevels];
  long long off[kKltMaxLevels];
};

struct KltPass {        // one calcOpticalFlowPyrLK call: I -> J
  const uint8_t* I;     // padded pyramid of I
  const short* dI;      // its derivatives
  const uint8_t* J;     // padded pyramid of J
  const float* pts;     // n x 2
  const float* init;    // n x 2 initial flow (OPTFLOW_USE_INITIAL_FLOW) or null
  float* out;           // n x 2
  uint8_t* status;      // n
  int n, reserved;
};
struct KltPasses {
  KltPass p[4];
};

struct KltMask {        // mask of goodFeaturesToTrack: an image (non-zero = allowed), or the complement of discs around kept tracks, or none
  const uint8_t* img;
  const float* disc;    // n_disc x 2; free iff (x - cx)^2 + (y - cy)^2 > r^2 for every cvRound(disc)
  int n_disc, r;
};

HSD int reflect101(int p, int n) {
  if (n == 1) return 0;
  while (p < 0 || p >= n) p = p < 0 ? -p : 2 * n - 2 - p;
  return p;
}

HSD bool klt_mask_at(const KltMask& m, int x, int y, int w) {
  if (m.img) return m.img[size_t(y) * w + x] != 0;
  for (int i = 0; i < m.n_disc; ++i) {
    const int cx = int(rintf(m.disc[2 * i])), cy = int(rintf(m.disc[2 * i + 1]));
    const int dx = x - cx, dy = y - cy;
    if (dx * dx + dy * dy <= m.r * m.r) return false;
  }
  return true;
}

/// Level `level` of the pyramid (if level < n_levels) and the derivatives of level - 1 (if level >= 1), for image blockIdx.z.
__global__ void __launch_bounds__(256) k_klt_pyramid(KltGeom g, int level, const uint8_t* raw0, const uint8_t* raw1, uint8_t* img0, uint8_t* img1,
                                                     short* der0, short* der1, int raw_w, int raw_h) {
  const uint8_t* raw = blockIdx.z ? raw1 : raw0;
  uint8_t* img = blockIdx.z ? img1 : img0;
  short* der = blockIdx.z ? der1 : der0;
  const int px = blockIdx.x * 16 + (threadIdx.x & 15), py = blockIdx.y * 16 + (threadIdx.x >> 4);
  const int P = g.pad;
  if (level < g.n_levels) {
    const int w = g.w[level], h = g.h[level], st = g.stride[level];
    if (px < st && py < h + 2 * P) {
      const int x = reflect101(px - P, w), y = reflect101(py - P, h);
      int v;
      if (level == 0) {
        v = raw[size_t(y) * raw_w + x];
      } else {
        const int w0 = g.w[level - 1], h0 = g.h[level - 1], st0 = g.stride[level - 1];
        const uint8_t* src = img + g.off[level - 1] + size_t(P) * st0 + P;
        const int k[5] = {1, 4, 6, 4, 1};
        int acc = 0;
        for (int j = 0; j < 5; ++j) {
          const uint8_t* row = src + size_t(reflect101(2 * y + j - 2, h0)) * st0;
          int r = 0;
          for (int i = 0; i < 5; ++i) r += k[i] * row[reflect101(2 * x + i - 2, w0)];
          acc += k[j] * r;
        }
        v = (acc + 128) >> 8;
      }
      img[g.off[level] + size_t(py) * st + px] = uint8_t(v);
    }
  }
  if (level >= 1) {
    const int l = level - 1, w = g.w[l], h = g.h[l], st = g.stride[l];
    if (px < st && py < h + 2 * P) {
      const int x = px - P, y = py - P;
      int dx = 0, dy = 0;
      if (x >= 0 && x < w && y >= 0 && y < h) {
        const uint8_t* src = img + g.off[l] + size_t(P) * st + P;
        const int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h), xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
        auto r = [&](int yy, int xx) { return int(src[size_t(yy) * st + xx]); };
        const int t0p = 3 * (r(ym, xp) + r(yp, xp)) + 10 * r(y, xp), t0m = 3 * (r(ym, xm) + r(yp, xm)) + 10 * r(y, xm);
        dx = t0p - t0m;
        const int t1m = r(yp, xm) - r(ym, xm), t1p = r(yp, xp) - r(ym, xp), t1 = r(yp, x) - r(ym, x);
        dy = 3 * (t1m + t1p) + 10 * t1;
      }
      short* d = der + 2 * (g.off[l] + size_t(py) * st + px);
      d[0] = short(dx), d[1] = short(dy);
    }
  }
}

struct KltWeights {
  int ix, iy, w00, w01, w10, w11;
};
HSD KltWeights klt_weights(float x, float y) {
#pragma clang fp contract(off)
  KltWeights k;
  const float fx = floorf(x), fy = floorf(y);
  k.ix = int(fx), k.iy = int(fy);
  const float a = x - float(k.ix), b = y - float(k.iy);
  const float sc = float(1 << kKltWBits);
  k.w00 = int(rintf((1.f - a) * (1.f - b) * sc));
  k.w01 = int(rintf(a * (1.f - b) * sc));
  k.w10 = int(rintf((1.f - a) * b * sc));
  k.w11 = (1 << kKltWBits) - k.w00 - k.w01 - k.w10;
  return k;
}

/// calcOpticalFlowPyrLK for one point, executed by one wave (every lane computes the same scalars; lane l holds patch pixels l + 64 k).
HSD void klt_lk_point(const KltGeom& g, const KltPass& ps, int i, int max_iter, double eps2, float min_eig) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, patch = g.patch, P = g.pad, npix = patch * patch;
  const float half = float(patch - 1) * 0.5f;
  int pxk[kKltPixPerLane], pyk[kKltPixPerLane];
#pragma unroll
  for (int k = 0; k < kKltPixPerLane; ++k) {
    const int idx = lane + 64 * k;
    pyk[k] = idx < npix ? idx / patch : 0;
    pxk[k] = idx < npix ? idx - pyk[k] * patch : 0;
  }
  const float p0x = ps.pts[2 * i], p0y = ps.pts[2 * i + 1];
  const int L = g.n_levels - 1;
  bool status = true;
  float nx = 0.f, ny = 0.f;  // nextPts[i]
  const float denom = float(2 * patch * patch);
  for (int level = L; level >= 0; --level) {
    const int cols = g.w[level], rows = g.h[level], st = g.stride[level];
    const float sc = float(1.0 / double(1 << level));
    float prx = p0x * sc, pry = p0y * sc;
    if (level == L) {
      if (ps.init) nx = ps.init[2 * i] * sc, ny = ps.init[2 * i + 1] * sc;
      else nx = prx, ny = pry;
    } else {
      nx = nx * 2.f, ny = ny * 2.f;
    }
    prx = prx - half, pry = pry - half;
    const KltWeights wi = klt_weights(prx, pry);
    if (wi.ix < -patch || wi.ix >= cols || wi.iy < -patch || wi.iy >= rows) {
      if (level == 0) status = false;
      continue;
    }
    const uint8_t* I = ps.I + g.off[level] + size_t(P) * st + P;
    const short* dI = ps.dI + 2 * (g.off[level] + size_t(P) * st + P);
    const uint8_t* J = ps.J + g.off[level] + size_t(P) * st + P;
    int Iv[kKltPixPerLane], Ix[kKltPixPerLane], Iy[kKltPixPerLane];
    int a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
    for (int k = 0; k < kKltPixPerLane; ++k) {
      Iv[k] = Ix[k] = Iy[k] = 0;
      if (lane + 64 * k < npix) {
        const long o = long(wi.iy + pyk[k]) * st + (wi.ix + pxk[k]);
        const uint8_t* s = I + o;
        Iv[k] = (s[0] * wi.w00 + s[1] * wi.w01 + s[st] * wi.w10 + s[st + 1] * wi.w11 + (1 << (kKltWBits - 6))) >> (kKltWBits - 5);
        const short* d = dI + 2 * o;
        const long st2 = 2 * long(st);
        Ix[k] = (d[0] * wi.w00 + d[2] * wi.w01 + d[st2] * wi.w10 + d[st2 + 2] * wi.w11 + (1 << (kKltWBits - 1))) >> kKltWBits;
        Iy[k] = (d[1] * wi.w00 + d[3] * wi.w01 + d[st2 + 1] * wi.w10 + d[st2 + 3] * wi.w11 + (1 << (kKltWBits - 1))) >> kKltWBits;
        a11 += Ix[k] * Ix[k], a12 += Ix[k] * Iy[k], a22 += Iy[k] * Iy[k];
      }
    }
    const float s20 = 1.f / 1048576.f;
    const float A11 = float(wave_sum(double(a11))) * s20, A12 = float(wave_sum(double(a12))) * s20, A22 = float(wave_sum(double(a22))) * s20;
    const float D = A11 * A22 - A12 * A12;
    const float dd = A11 - A22;
    const float minEig = (A22 + A11 - sqrtf(dd * dd + 4.f * A12 * A12)) / denom;
    if (minEig < min_eig || D < __FLT_EPSILON__) {
      if (level == 0) status = false;
      continue;
    }
    const float Dinv = 1.f / D;
    float cx = nx - half, cy = ny - half;
    float pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < max_iter; ++j) {
      const KltWeights wj = klt_weights(cx, cy);
      if (wj.ix < -patch || wj.ix >= cols || wj.iy < -patch || wj.iy >= rows) {
        if (level == 0) status = false;
        break;
      }
      int b1i = 0, b2i = 0;
#pragma unroll
      for (int k = 0; k < kKltPixPerLane; ++k) {
        if (lane + 64 * k < npix) {
          const uint8_t* s = J + long(wj.iy + pyk[k]) * st + (wj.ix + pxk[k]);
          const int diff = ((s[0] * wj.w00 + s[1] * wj.w01 + s[st] * wj.w10 + s[st + 1] * wj.w11 + (1 << (kKltWBits - 6))) >> (kKltWBits - 5)) - Iv[k];
          b1i += diff * Ix[k], b2i += diff * Iy[k];
        }
      }
      const float b1 = float(wave_sum(double(b1i))) * s20, b2 = float(wave_sum(double(b2i))) * s20;
      const float dx = (A12 * b2 - A22 * b1) * Dinv, dy = (A12 * b1 - A11 * b2) * Dinv;
      cx = cx + dx, cy = cy + dy;
      nx = cx + half, ny = cy + half;
      if (double(dx) * double(dx) + double(dy) * double(dy) <= eps2) break;
      if (j > 0 && fabs(double(dx + pdx)) < 0.01 && fabs(double(dy + pdy)) < 0.01) {
        nx = nx - dx * 0.5f, ny = ny - dy * 0.5f;
        break;
      }
      pdx = dx, pdy = dy;
    }
  }
  if (lane == 0) {
    ps.out[2 * i] = nx, ps.out[2 * i + 1] = ny;
    ps.status[i] = status ? 1 : 0;
  }
}

/// One wave per point (four per workgroup) of pass blockIdx.y.
__global__ void __launch_bounds__(256) k_klt_flow(KltGeom g, KltPasses passes, int max_iter, double eps2, float min_eig) {
  const KltPass& ps = passes.p[blockIdx.y];
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= ps.n) return;
  klt_lk_point(g, ps, i, max_iter, eps2, min_eig);
}

HSD unsigned klt_order_key(float v) {  // monotone map of float to unsigned; 0 lies below every real value
  const unsigned b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
HSD float klt_order_value(unsigned k) {
  if (k == 0) return 0.f;
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

HSD int klt_sobel_x(const uint8_t* im, int w, int h, int x, int y) {
  const int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h), xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
  auto r = [&](int yy, int xx) { return int(im[size_t(yy) * w + xx]); };
  return (r(ym, xp) - r(ym, xm)) + 2 * (r(y, xp) - r(y, xm)) + (r(yp, xp) - r(yp, xm));
}
HSD int klt_sobel_y(const uint8_t* im, int w, int h, int x, int y) {
  const int ym = reflect101(y - 1, h), yp = reflect101(y + 1, h), xm = reflect101(x - 1, w), xp = reflect101(x + 1, w);
  auto r = [&](int yy, int xx) { return int(im[size_t(yy) * w + xx]); };
  return (r(yp, xm) - r(ym, xm)) + 2 * (r(yp, x) - r(ym, x)) + (r(yp, xp) - r(ym, xp));
}

/// cornerMinEigenVal (block 3, Sobel 3, 8-bit): eig[y w + x]; *max_key = klt_order_key of the maximum over the mask.
__global__ void __launch_bounds__(256) k_klt_min_eigen(const uint8_t* im, int w, int h, float* eig, unsigned* max_key, KltMask mask) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  unsigned key = 0;
  if (x < w && y < h) {
    int sxx = 0, sxy = 0, syy = 0;
    for (int j = -1; j <= 1; ++j)
      for (int i = -1; i <= 1; ++i) {
        const int xx = reflect101(x + i, w), yy = reflect101(y + j, h);
        const int gx = klt_sobel_x(im, w, h, xx, yy), gy = klt_sobel_y(im, w, h, xx, yy);
        sxx += gx * gx, sxy += gx * gy, syy += gy * gy;
      }
    const float s = float(1.0 / (3060.0 * 3060.0));
    const float a = 0.5f * float(sxx) * s, b = float(sxy) * s, c = 0.5f * float(syy) * s;
    const float d = a - c;
    const float lam = (a + c) - sqrtf(d * d + b * b);
    eig[size_t(y) * w + x] = lam;
    if (max_key && klt_mask_at(mask, x, y, w)) key = klt_order_key(lam);
  }
  if (max_key) {
    for (int o = 32; o >= 1; o >>= 1) key = max(key, unsigned(__shfl_xor(int(key), o)));
    if ((threadIdx.x & 63) == 0 && key) atomicMax(max_key, key);
  }
}

/// Corners of goodFeaturesToTrack before the distance test: keys (response bits << 32 | raster index), in no particular order; *count.
__global__ void __launch_bounds__(256) k_klt_candidates(const float* eig, int w, int h, const unsigned* max_key, double quality, KltMask mask,
                                                        unsigned long long* keys, int* count) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * 16 + (threadIdx.x & 15), y = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (x < 1 || y < 1 || x > w - 2 || y > h - 2) return;
  const float thr = float(double(klt_order_value(*max_key)) * quality);
  auto e = [&](int xx, int yy) {
    const float v = eig[size_t(yy) * w + xx];
    return v > thr ? v : 0.f;
  };
  const float v = e(x, y);
  if (v == 0.f) return;
  float m = v;
  for (int j = -1; j <= 1; ++j)
    for (int i = -1; i <= 1; ++i) m = fmaxf(m, e(x + i, y + j));
  if (v != m || !klt_mask_at(mask, x, y, w)) return;
  const int at = atomicAdd(count, 1);
  keys[at] = (static_cast<unsigned long long>(klt_order_key(v)) << 32) | unsigned(y * w + x);
}

/// sorted[rank] = key, rank = number of larger keys (descending: response, then raster index — OpenCV 4's greaterThanPtr).
__global__ void __launch_bounds__(256) k_klt_rank(const unsigned long long* keys, const int* count, unsigned long long* sorted) {
  __shared__ unsigned long long tile[256];
  const int n = *count;
  if (int(blockIdx.x) * 256 >= n) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const unsigned long long mine = i < n ? keys[i] : 0ull;
  int rank = 0;
  for (int t0 = 0; t0 < n; t0 += 256) {
    __syncthreads();
    if (t0 + int(threadIdx.x) < n) tile[threadIdx.x] = keys[t0 + threadIdx.x];
    __syncthreads();
    const int m = min(256, n - t0);
    for (int j = 0; j < m; ++j) rank += tile[j] > mine ? 1 : 0;
  }
  if (i < n) sorted[rank] = mine;
}

/// The greedy of goodFeaturesToTrack on the sorted candidates, one workgroup of 1024: 64 candidates per step are tested against every
/// accepted corner by 16 groups of 64 lanes, then wave 0 settles the conflicts inside the step in rank order. corners: n_out x 2.
__global__ void __launch_bounds__(1024) k_klt_select(const unsigned long long* sorted, const int* count, int w, int max_corners, double min_distance,
                                                     float* corners, int* n_out) {
  __shared__ int bad[64];
  __shared__ int s_acc, s_stop;
  const int n = *count, t = threadIdx.x, c = t & 63, grp = t >> 6;
  const int limit = max_corners > 0 ? max_corners : n;
  const bool check = min_distance >= 1.0;
  const double md2 = min_distance * min_distance;
  if (t == 0) s_acc = 0, s_stop = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 64) {
    const int acc = s_acc;
    if (s_stop) break;
    if (t < 64) bad[t] = 0;
    __syncthreads();
    const int ci = base + c;
    int cx = 0, cy = 0;
    if (ci < n) {
      const unsigned idx = unsigned(sorted[ci] & 0xffffffffull);
      cy = int(idx / unsigned(w)), cx = int(idx - unsigned(cy) * unsigned(w));
    }
    if (check && ci < n) {
      for (int j = grp; j < acc; j += 16) {
        const int dx = cx - int(corners[2 * j]), dy = cy - int(corners[2 * j + 1]);
        if (double(dx * dx + dy * dy) < md2) {
          bad[c] = 1;
          break;
        }
      }
    }
    __syncthreads();
    if (t < 64) {
      bool good = ci < n && !bad[c];
      if (check)
        for (int s = 0; s < 64; ++s) {
          const int gs = __shfl(int(good), s), xs = __shfl(cx, s), ys = __shfl(cy, s);
          if (gs && c > s) {
            const int dx = cx - xs, dy = cy - ys;
            if (double(dx * dx + dy * dy) < md2) good = false;
          }
        }
      const unsigned long long bal = __ballot(good);
      const int before = __popcll(bal & ((1ull << c) - 1ull));
      const int total = __popcll(bal);
      if (good && acc + before < limit) {
        corners[2 * (acc + before)] = float(cx);
        corners[2 * (acc + before) + 1] = float(cy);
      }
      if (t == 0) {
        s_acc = min(limit, acc + total);
        if (s_acc >= limit) s_stop = 1;
      }
    }
    __syncthreads();
  }
  if (t == 0) *n_out = s_acc;
}

}  // namespace hs
