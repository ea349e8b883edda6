// kernels_covariance.hpp — marginal covariances of the window state (hs_compute_covariance). Not on the per-iteration path.
//
// The covariance is the inverse of the undamped Gauss-Newton matrix J'J at the device-resident point, in Ceres-local coordinates. Its
// ingredients are what one build of the solver writes without damping (hs_reduced_system's launch sequence at radius = 1e300, capi.hip):
//   S~ = D_p S_pp D_p (Tables::Sb, band rows)   the Jacobi-scaled reduced pose system, landmarks eliminated (S_pp = H_pp - Yh Yh')
//   S~_pb, S~_bb (Tables::Spb, Sbb)             the border blocks of the bias splines and gravity, scaled the same way
//   L_l, Yh (Tables::lm_L, Y)                   per landmark: V = S_l H_ll S_l = L L', Yh = H_pl S_l L^-T (pose side unscaled)
// and the kernels below turn them into
//   k_cov_band       (one workgroup)  S~ = U'U (band Cholesky, natural order), Z = U^-T S~_pb, X = U^-1 Z, C = (S~_bb - Z'Z)^-1 and the
//                                     selected inverse of S~ on the band pattern (Takahashi recurrence, backward over the rows):
//                                       Sig(i, j) = -1/U_ii sum_k U_ik Sig(k, j),  Sig(i, i) = 1/U_ii (1/U_ii - sum_k U_ik Sig(i, k)),  k, j in (i, e_i)
//                                     every operand lies in the band rows of the block-aligned layout, so the recurrence closes on it.
//   k_cov_finish     (block rows)     Sig_pp = Sig + X C X', Sig_pb = -X C, Sig_bb = C, unscaled: Sigma = D Sig D
//   k_cov_landmarks  (wave/landmark)  Sigma_ll = S_l L^-T (I + Yh' Sigma_pp Yh) L^-1 S_l from the <= bw band blocks the landmark touches
//   k_cov_landmarks_cam (wave/landmark)  the same with free camera coordinates in the border (hs_set_camera_covariance): G = [Yh ; Y_c'] over
//                                     the landmark's pose rows and the camera columns, Sigma from the band, Sigma_pb and Sigma_bb
//   k_cov_sample     (wave/stamp)     J(t) Sigma_cp J(t)', J(t) = the state Jacobian of the pose prior with its measurement at the pose at t
//   k_cov_sample_sensor (wave/stamp)  the same for a sensor pose T_wb(t) o T_bs; a free T_bs (camera, IMU) adds its columns of Sigma_pb and its
//                                     block of Sigma_bb through the extrinsics Jacobian (hs_sample_sensor_covariance)
// Constant coordinates are decoupled rows (identity in the factor, zero covariance); a free coordinate whose pivot is not positive or falls
// below kCovPivotTol of its scaled diagonal — the build's marker 1.0 of a structurally zero column included — ends the factorisation and
// is reported through CovBand::status. Owner-computes everywhere, one fixed order per sum: two computations are bit-identical.
#pragma once
#include "kernels_common.hpp"

namespace hs {

constexpr double kCovPivotTol = 1e-12;  // a pivot below this fraction of its Jacobi-scaled diagonal is rank deficiency
constexpr int kCovLdsMaxCols = 128;     // 6 bw <= 128: k_cov_band keeps its trailing window (6 bw x 6 bw) in LDS, global memory beyond

/// Operands of k_cov_band and k_cov_finish.
struct CovBand {
  const double* Sb;          // np x ncb  scaled, undamped band rows (input)
  const double* Spb;         // np x nb   scaled border columns (input)
  const double* Sbb;         // nb x nb   scaled border block (input)
  const uint8_t* col_const;  // np + nb   1: coordinate held constant (zero covariance)
  double* Ub;                // np x ncb  factor rows (the working rows of the factorisation)
  double* Sig;               // np x ncb  selected inverse of S~ (scaled, band layout of Sb; both triangles of the diagonal blocks)
  double* Zb;                // np x nb   working border rows, then Z = U^-T S~_pb
  double* Xb;                // np x nb   X = U^-1 Z
  double* Cb;                // nb x nb   S~_bb - Z'Z, its Cholesky factor (lower), then C
  double* Lb;                // nb x nb   inverse of that factor (lower)
  const double* scale_p;     // np
  const double* scale_b;     // nb
  double* cov;               // np x ncb  Sigma_pp, unscaled, band layout
  double* cov_pb;            // np x nb   Sigma_pb, unscaled
  double* cov_bb;            // nb x nb   Sigma_bb, unscaled
  int* status;               // 0, or 1 + the first rank-deficient coordinate (pose rows first, then the border)
  int np, ncb, nb;
};

/// Dynamic LDS of k_cov_band<LDS>, in doubles.
inline size_t cov_band_lds_doubles(bool lds, int ncb) { return (lds ? size_t(ncb) * ncb : 0) + kBlock + ncb; }

template <bool LDS>
HSD double* cov_row(const CovBand& B, double* win, double* glob, int r) {
  return LDS ? win + size_t(r % B.ncb) * B.ncb : glob + size_t(r) * B.ncb;
}

/// One workgroup of kBlock lanes. LDS = true: the trailing window of the factorisation and of the recurrence lives in dynamic LDS
/// (ncb x ncb doubles; 6 bw <= kCovLdsMaxCols), followed by kBlock doubles of reduction scratch and the factor row of the current step of
/// the recurrence (ncb doubles); LDS = false: only the scratch and the row. cov_band_lds_doubles() gives the size.
template <bool LDS>
__global__ void __launch_bounds__(kBlock) k_cov_band(CovBand B) {
  HS_DYNAMIC_LDS(smem);
  double* win = smem;
  double* red = LDS ? smem + size_t(B.ncb) * B.ncb : smem;
  double* urow = red + kBlock;
  const int tid = threadIdx.x, np = B.np, ncb = B.ncb, nb = B.nb;
  auto is_const = [&](int r) { return B.col_const[r] != 0; };
  // ---- border rows enter masked: constant rows / columns are decoupled ----
  for (int e = tid; e < np * nb; e += kBlock) {
    const int r = e / nb, b = e % nb;
    B.Zb[e] = (is_const(r) || is_const(np + b)) ? 0.0 : B.Spb[e];
  }
  // ---- band Cholesky S~ = U'U, right-looking, one row per step; Z = U^-T S~_pb alongside ----
  int loaded = 0;
  for (int i = 0; i < np; ++i) {
    const int c0 = 6 * (i / 6), e = min(np, c0 + ncb), L = e - i - 1;
    if (e > loaded) {  // rows [loaded, e) enter the window (masked): slot of row r = r % ncb, free since row r - ncb < i is done
      if (LDS) __syncthreads();  // (... once every lane has left the previous step's update, which reads the row of that slot)
      const int n_new = e - loaded;
      for (int q = tid; q < n_new * ncb; q += kBlock) {
        const int r = loaded + q / ncb, c = q % ncb, j = 6 * (r / 6) + c;
        double v = 0.0;
        if (j < np && j >= r) v = (is_const(r) || is_const(j)) ? (j == r ? 1.0 : 0.0) : B.Sb[size_t(r) * ncb + c];
        cov_row<LDS>(B, win, B.Ub, r)[c] = v;
      }
      loaded = e;
    }
    __syncthreads();
    double* Wi = cov_row<LDS>(B, win, B.Ub, i);
    const double d = Wi[i - c0];
    if (!is_const(i)) {
      const double orig = B.Sb[size_t(i) * ncb + (i - c0)];
      if (!(orig < 1.0) || !(d > kCovPivotTol * orig)) {  // (the build writes 1.0 on the diagonal of a structurally zero column)
        if (tid == 0) *B.status = i + 1;
        return;
      }
    }
    const double u = sqrt(d), inv = 1.0 / u;
    __syncthreads();  // (every lane has read the pivot before it is overwritten)
    for (int q = tid; q < ncb; q += kBlock) {
      const int j = c0 + q;
      const double v = j == i ? u : (j > i && j < e ? Wi[q] * inv : 0.0);
      Wi[q] = v;
      if (LDS) B.Ub[size_t(i) * ncb + q] = v;
    }
    for (int b = tid; b < nb; b += kBlock) B.Zb[size_t(i) * nb + b] *= inv;
    __syncthreads();
    for (int q = tid; q < L * L; q += kBlock) {  // trailing update W(k, j) -= U(i, k) U(i, j), i < k <= j < e
      const int a = q / L, bb = q % L;
      if (bb < a) continue;
      const int k = i + 1 + a, j = i + 1 + bb;
      double* Wk = cov_row<LDS>(B, win, B.Ub, k);
      Wk[j - 6 * (k / 6)] -= Wi[k - c0] * Wi[j - c0];
    }
    for (int q = tid; q < L * nb; q += kBlock) {
      const int a = q / nb, b = q % nb, k = i + 1 + a;
      B.Zb[size_t(k) * nb + b] -= Wi[k - c0] * B.Zb[size_t(i) * nb + b];
    }
  }
  __syncthreads();
  // ---- selected inverse, backward; X = U^-1 Z alongside ----
  for (int i = np - 1; i >= 0; --i) {
    const int c0 = 6 * (i / 6), e = min(np, c0 + ncb), L = e - i - 1;
    for (int q = tid; q < ncb; q += kBlock) urow[q] = B.Ub[size_t(i) * ncb + q];  // (the previous step ended with a barrier)
    __syncthreads();
    const double* Ui = urow;
    double* Si = cov_row<LDS>(B, win, B.Sig, i);
    const bool cst = is_const(i);
    const double inv = 1.0 / Ui[i - c0];
    const int P = L > 0 ? max(1, kBlock / L) : 1;
    if (!cst && tid < P * L) {
      const int jj = tid % L, part = tid / L, j = i + 1 + jj;
      double s = 0.0;
      for (int kk = part; kk < L; kk += P) {
        const int k = i + 1 + kk;
        const double skj = k <= j ? cov_row<LDS>(B, win, B.Sig, k)[j - 6 * (k / 6)] : cov_row<LDS>(B, win, B.Sig, j)[k - 6 * (j / 6)];
        s = fma(Ui[k - c0], skj, s);
      }
      red[tid] = s;
    }
    for (int b = tid; b < nb; b += kBlock) {
      double x = 0.0;
      if (!cst) {  // (four partial sums: independent loads in flight)
        double s[4] = {B.Zb[size_t(i) * nb + b], 0.0, 0.0, 0.0};
        for (int kk = 0; kk < L; ++kk) s[kk & 3] -= Ui[i + 1 + kk - c0] * B.Xb[size_t(i + 1 + kk) * nb + b];
        x = ((s[0] + s[1]) + (s[2] + s[3])) * inv;
      }
      B.Xb[size_t(i) * nb + b] = x;
    }
    __syncthreads();
    if (tid < L) {
      double s = 0.0;
      for (int p = 0; p < P; ++p) s += red[p * L + tid];
      const double v = cst ? 0.0 : -inv * s;
      Si[i + 1 + tid - c0] = v;
      if (LDS) B.Sig[size_t(i) * ncb + (i + 1 + tid - c0)] = v;
    }
    if (tid >= L + 1 && tid < ncb - (i - c0)) {  // columns past the matrix
      Si[i - c0 + tid] = 0.0;
      if (LDS) B.Sig[size_t(i) * ncb + (i - c0 + tid)] = 0.0;
    }
    __syncthreads();
    if (tid < 64) {
      double s = 0.0;
      for (int kk = tid; kk < L; kk += 64) s = fma(Ui[i + 1 + kk - c0], Si[i + 1 + kk - c0], s);
      s = wave_sum(s);
      if (tid == 0) {
        const double v = cst ? 0.0 : inv * (inv - s);
        Si[i - c0] = v;
        if (LDS) B.Sig[size_t(i) * ncb + (i - c0)] = v;
      }
    }
    __syncthreads();
  }
  // ---- lower triangles of the diagonal blocks, by symmetry ----
  for (int q = tid; q < np * 6; q += kBlock) {
    const int r = q / 6, c = q % 6, c0 = 6 * (r / 6);
    if (c0 + c < r) B.Sig[size_t(r) * ncb + c] = B.Sig[size_t(c0 + c) * ncb + (r - c0)];
  }
  if (nb == 0) return;
  // ---- border: C = (S~_bb - Z'Z)^-1 by a dense Cholesky (lower, in Cb) and the inverse of its factor ----
  for (int q = tid; q < nb * nb; q += kBlock) {
    const int a = q / nb, b = q % nb;
    double v;
    if (is_const(np + a) || is_const(np + b)) {
      v = a == b ? 1.0 : 0.0;
    } else {
      double z[4] = {0.0, 0.0, 0.0, 0.0};
      for (int r = 0; r < np; ++r) z[r & 3] = fma(B.Zb[size_t(r) * nb + a], B.Zb[size_t(r) * nb + b], z[r & 3]);
      v = B.Sbb[q] - ((z[0] + z[1]) + (z[2] + z[3]));
    }
    B.Cb[q] = v;
  }
  __syncthreads();
  for (int a = 0; a < nb; ++a) {
    const double d = B.Cb[size_t(a) * nb + a];
    if (!is_const(np + a)) {
      const double orig = B.Sbb[size_t(a) * nb + a];
      if (!(orig < 1.0) || !(d > kCovPivotTol * orig)) {
        if (tid == 0) *B.status = np + a + 1;
        return;
      }
    }
    const double l = sqrt(d), inv = 1.0 / l;
    __syncthreads();
    for (int b = a + tid; b < nb; b += kBlock) B.Cb[size_t(b) * nb + a] = b == a ? l : B.Cb[size_t(b) * nb + a] * inv;
    __syncthreads();
    const int m = nb - a - 1;
    for (int q = tid; q < m * m; q += kBlock) {
      const int b = a + 1 + q / m, c = a + 1 + q % m;
      if (c <= b) B.Cb[size_t(b) * nb + c] -= B.Cb[size_t(b) * nb + a] * B.Cb[size_t(c) * nb + a];
    }
    __syncthreads();
  }
  for (int a = tid; a < nb; a += kBlock) {  // column a of the inverse factor: forward substitution of e_a
    for (int b = 0; b < nb; ++b) {
      double v = 0.0;
      if (b >= a) {
        v = b == a ? 1.0 : 0.0;
        for (int c = a; c < b; ++c) v -= B.Cb[size_t(b) * nb + c] * B.Lb[size_t(c) * nb + a];
        v /= B.Cb[size_t(b) * nb + b];
      }
      B.Lb[size_t(b) * nb + a] = v;
    }
  }
  __syncthreads();
  for (int q = tid; q < nb * nb; q += kBlock) {  // C = L^-T L^-1
    const int a = q / nb, b = q % nb;
    double v = 0.0;
    if (!is_const(np + a) && !is_const(np + b))
      for (int c = max(a, b); c < nb; ++c) v = fma(B.Lb[size_t(c) * nb + a], B.Lb[size_t(c) * nb + b], v);
    B.Cb[q] = v;
  }
}

/// One workgroup per block row i (grid n_cp): Sigma_pp = D_p (Sig + X C X') D_p on the band rows 6i .. 6i+5, Sigma_pb = -D_p X C D_b,
/// workgroup 0 also Sigma_bb = D_b C D_b. Dynamic LDS: 6 nb doubles (the rows of X C).
__global__ void __launch_bounds__(kBlock) k_cov_finish(CovBand B) {
  HS_DYNAMIC_LDS(smem);
  const int i = blockIdx.x, tid = threadIdx.x, np = B.np, ncb = B.ncb, nb = B.nb;
  double* Y = smem;  // 6 x nb: rows of X C
  for (int q = tid; q < 6 * nb; q += kBlock) {
    const int a = q / nb, b = q % nb, rho = 6 * i + a;
    double v = 0.0;
    for (int c = 0; c < nb; ++c) v = fma(B.Xb[size_t(rho) * nb + c], B.Cb[size_t(c) * nb + b], v);
    Y[q] = v;
    B.cov_pb[size_t(rho) * nb + b] = -B.scale_p[rho] * v * B.scale_b[b];
  }
  __syncthreads();
  for (int q = tid; q < 6 * ncb; q += kBlock) {
    const int a = q / ncb, c = q % ncb, rho = 6 * i + a, col = 6 * i + c;
    double v = 0.0;
    if (col < np) {
      v = B.Sig[size_t(rho) * ncb + c];
      for (int b = 0; b < nb; ++b) v = fma(Y[a * nb + b], B.Xb[size_t(col) * nb + b], v);
      v *= B.scale_p[rho] * B.scale_p[col];
    }
    B.cov[size_t(rho) * ncb + c] = v;
  }
  if (i == 0)
    for (int q = tid; q < nb * nb; q += kBlock) B.cov_bb[q] = B.scale_b[q / nb] * B.Cb[q] * B.scale_b[q % nb];
}

/// Entry (r, c) of Sigma_pp from the band rows (both within the band).
HSD double cov_band_at(const double* cov, int ncb, int r, int c) {
  return r <= c ? cov[size_t(r) * ncb + (c - 6 * (r / 6))] : cov[size_t(c) * ncb + (r - 6 * (c / 6))];
}

/// One wave per device landmark: Sigma_ll = S_l L^-T (I + Yh' Sigma_pp Yh) L^-1 S_l (Sigma_pp unscaled, Yh unscaled on the pose side as
/// k_update_visual reads it). Constant landmarks: zero; landmarks without residual rows: NaN (not in the problem); status[dl] = 1: the
/// landmark's 3 x 3 system is rank deficient.
__global__ void __launch_bounds__(kBlock) k_cov_landmarks(Tables T, const double* cov, double* out, int* status) {
  const int lane = threadIdx.x & 63, dl = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (dl >= T.n_lm) return;
  const int ncb = 6 * T.bw;
  const bool observed = T.lm_ptr[dl + 1] > T.lm_ptr[dl];
  if (!observed || T.lm_const[dl]) {
    if (lane < 9) out[9 * size_t(dl) + lane] = observed ? 0.0 : __builtin_nan("");
    if (lane == 0) status[dl] = 0;
    return;
  }
  const int rows = 6 * T.lm_ncp[dl], r0 = 6 * T.lm_cfirst[dl];
  const double* Y = T.Y + T.lm_yoff[dl];
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = lane; r < rows; r += 64) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (int c = 0; c < rows; ++c) {
      const double s = cov_band_at(cov, ncb, r0 + r, r0 + c);
      t0 = fma(s, Y[3 * c], t0), t1 = fma(s, Y[3 * c + 1], t1), t2 = fma(s, Y[3 * c + 2], t2);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double y = Y[3 * r + a];
      m[3 * a] = fma(y, t0, m[3 * a]), m[3 * a + 1] = fma(y, t1, m[3 * a + 1]), m[3 * a + 2] = fma(y, t2, m[3 * a + 2]);
    }
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) m[e] = wave_sum(m[e]);
  if (lane != 0) return;
  const double* Lf = T.lm_L + 6 * size_t(dl);
  const double l00 = Lf[0], l10 = Lf[1], l11 = Lf[2], l20 = Lf[3], l21 = Lf[4], l22 = Lf[5];
  const bool ok = l00 > 0.0 && l11 > 0.0 && l22 > 0.0 && l11 * l11 > kCovPivotTol * (l10 * l10 + l11 * l11) &&
                  l22 * l22 > kCovPivotTol * (l20 * l20 + l21 * l21 + l22 * l22) && isfinite(l00 + l10 + l11 + l20 + l21 + l22);
  status[dl] = ok ? 0 : 1;
  // N = L^-1 (lower): columns of the inverse by forward substitution
  const double n00 = 1.0 / l00, n11 = 1.0 / l11, n22 = 1.0 / l22;
  const double n10 = -l10 * n00 * n11, n21 = -l21 * n11 * n22, n20 = -(l20 * n00 + l21 * n10) * n22;
  const double N[9] = {n00, 0.0, 0.0, n10, n11, 0.0, n20, n21, n22};
  double A[9];
#pragma unroll
  for (int e = 0; e < 9; ++e) A[e] = m[e] + (e % 4 == 0 ? 1.0 : 0.0);
  double AN[9];  // A N
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) AN[3 * a + b] = A[3 * a] * N[b] + A[3 * a + 1] * N[3 + b] + A[3 * a + 2] * N[6 + b];
  const double* sl = T.lm_scale + 3 * size_t(dl);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double v = N[a] * AN[b] + N[3 + a] * AN[3 + b] + N[6 + a] * AN[6 + b];  // (N' A N)(a, b)
      out[9 * size_t(dl) + 3 * a + b] = ok ? sl[a] * v * sl[b] : __builtin_nan("");
    }
}

/// Dynamic LDS of k_cov_landmarks_cam, in doubles: per wave the rows of G of the widest landmark (6 bw pose rows) and the nc camera rows.
inline size_t cov_landmarks_cam_lds_doubles(int bw, int nc) { return size_t(kBlock / 64) * 3 * (6 * bw + nc); }

/// Handles with free camera coordinates (T.nc > 0, the last nc border columns; kernels_calib.hpp). One wave per device landmark. The camera
/// moves with the landmark, delta_l = -S_l L^-T (yh - Yh' delta_p - Y_c delta_c), so with G = [Yh ; Y_c'] over [p_l ; c] — the
/// 6 n_l pose rows the landmark touches, then the nc camera coordinates —
///   Sigma_ll = S_l L^-T (I + G' Sigma_[p_l,c] G) L^-1 S_l,
/// Sigma_[p_l,c] read in place from the band (cov), the camera columns of Sigma_pb (cov_pb) and the trailing nc x nc block of Sigma_bb
/// (cov_bb), all unscaled. A lane owns the rows r = lane, lane + 64, ... of Sigma G (up to 6 * 42 + 64 = 316 rows); G is staged in the wave's
/// slice of dynamic LDS (cov_landmarks_cam_lds_doubles). Constant / unobserved landmarks and the rank test: as in k_cov_landmarks, which
/// handles without free camera coordinates keep launching. Fixed order in every sum: two computations are bit-identical.
__global__ void __launch_bounds__(kBlock) k_cov_landmarks_cam(Tables T, const double* cov, const double* cov_pb, const double* cov_bb, double* out, int* status) {
  HS_DYNAMIC_LDS(smem);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, dl = blockIdx.x * (kBlock / 64) + w;
  if (dl >= T.n_lm) return;
  const int ncb = 6 * T.bw, nc = T.nc, nb = T.nb, nbi = T.nb - T.nc;
  const bool observed = T.lm_ptr[dl + 1] > T.lm_ptr[dl];
  if (!observed || T.lm_const[dl]) {
    if (lane < 9) out[9 * size_t(dl) + lane] = observed ? 0.0 : __builtin_nan("");
    if (lane == 0) status[dl] = 0;
    return;
  }
  const int rows = 6 * T.lm_ncp[dl], r0 = 6 * T.lm_cfirst[dl], nr = rows + nc;
  const double* Y = T.Y + T.lm_yoff[dl];
  const double* Yc = T.calib_Yc + size_t(dl) * 3 * nc;  // 3 x nc
  double* G = smem + size_t(w) * 3 * (ncb + nc);         // nr x 3
  for (int e = lane; e < 3 * rows; e += 64) G[e] = Y[e];
  for (int e = lane; e < 3 * nc; e += 64) G[3 * (rows + e % nc) + e / nc] = Yc[e];
  wait_lds();  // (hand-over between the lanes of one wave)
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int r = lane; r < nr; r += 64) {
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    const double* Gc = G + 3 * rows;
    if (r < rows) {  // a pose row: [band | camera columns of Sigma_pb]
      for (int c = 0; c < rows; ++c) {
        const double s = cov_band_at(cov, ncb, r0 + r, r0 + c);
        t0 = fma(s, G[3 * c], t0), t1 = fma(s, G[3 * c + 1], t1), t2 = fma(s, G[3 * c + 2], t2);
      }
      const double* pb = cov_pb + size_t(r0 + r) * nb + nbi;
      for (int c = 0; c < nc; ++c) {
        const double s = pb[c];
        t0 = fma(s, Gc[3 * c], t0), t1 = fma(s, Gc[3 * c + 1], t1), t2 = fma(s, Gc[3 * c + 2], t2);
      }
    } else {  // a camera row: [camera column of Sigma_pb, transposed | trailing block of Sigma_bb]
      const int a = nbi + (r - rows);
      for (int c = 0; c < rows; ++c) {
        const double s = cov_pb[size_t(r0 + c) * nb + a];
        t0 = fma(s, G[3 * c], t0), t1 = fma(s, G[3 * c + 1], t1), t2 = fma(s, G[3 * c + 2], t2);
      }
      const double* bb = cov_bb + size_t(a) * nb + nbi;
      for (int c = 0; c < nc; ++c) {
        const double s = bb[c];
        t0 = fma(s, Gc[3 * c], t0), t1 = fma(s, Gc[3 * c + 1], t1), t2 = fma(s, Gc[3 * c + 2], t2);
      }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double y = G[3 * r + a];
      m[3 * a] = fma(y, t0, m[3 * a]), m[3 * a + 1] = fma(y, t1, m[3 * a + 1]), m[3 * a + 2] = fma(y, t2, m[3 * a + 2]);
    }
  }
#pragma unroll
  for (int e = 0; e < 9; ++e) m[e] = wave_sum(m[e]);
  if (lane != 0) return;
  // (from here on the tail of k_cov_landmarks, restated: that kernel is left exactly as it is)
  const double* Lf = T.lm_L + 6 * size_t(dl);
  const double l00 = Lf[0], l10 = Lf[1], l11 = Lf[2], l20 = Lf[3], l21 = Lf[4], l22 = Lf[5];
  const bool ok = l00 > 0.0 && l11 > 0.0 && l22 > 0.0 && l11 * l11 > kCovPivotTol * (l10 * l10 + l11 * l11) &&
                  l22 * l22 > kCovPivotTol * (l20 * l20 + l21 * l21 + l22 * l22) && isfinite(l00 + l10 + l11 + l20 + l21 + l22);
  status[dl] = ok ? 0 : 1;
  const double n00 = 1.0 / l00, n11 = 1.0 / l11, n22 = 1.0 / l22;
  const double n10 = -l10 * n00 * n11, n21 = -l21 * n11 * n22, n20 = -(l20 * n00 + l21 * n10) * n22;
  const double N[9] = {n00, 0.0, 0.0, n10, n11, 0.0, n20, n21, n22};  // N = L^-1 (lower)
  double AN[9];  // (I + G' Sigma G) N
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double a0 = m[3 * a] + (a == 0 ? 1.0 : 0.0), a1 = m[3 * a + 1] + (a == 1 ? 1.0 : 0.0), a2 = m[3 * a + 2] + (a == 2 ? 1.0 : 0.0);
      AN[3 * a + b] = a0 * N[b] + a1 * N[3 + b] + a2 * N[6 + b];
    }
  const double* sl = T.lm_scale + 3 * size_t(dl);
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const double v = N[a] * AN[b] + N[3 + a] * AN[3 + b] + N[6 + a] * AN[6 + b];  // (N' A N)(a, b)
      out[9 * size_t(dl) + 3 * a + b] = ok ? sl[a] * v * sl[b] : __builtin_nan("");
    }
}

/// One wave per stamp: J(t) Sigma_cp J(t)' with J(t) the state Jacobian of the pose prior (prior_linearize, identity sensor) whose measurement is
/// the pose at t — [Log(R_m' R) ; p - p_m] at zero residual. The pose depends on the control points only: no border term.
template <int K>
__global__ void __launch_bounds__(kBlock) k_cov_sample(Tables T, const double* cov, int n, const double* stamps, double* out) {
  __shared__ double Js[kBlock / 64][6 * 6 * K];
  __shared__ double JS[kBlock / 64][6 * 6 * K];
  __shared__ int first_s[kBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * (kBlock / 64) + w;
  const bool active = i < n;
  double* J = Js[w];
  if (active && lane == 0) {
    double u;
    const int first = segment_of(stamps[i], T.sp.t0, T.sp.dt, K, &u);
    double lam[K], dl[1], ddl[1];
    basis_weights<K>(T.basis, u, T.sp.inv_dt, lam, dl, ddl, 0);
    Quat qw;
    V3 pw;
    M3 G[K];
    spline_pose_jac<K>(T.cp + 8 * first, lam, &qw, &pw, G);
    const double id_sensor[7] = {0, 0, 0, 1, 0, 0, 0}, meas[7] = {qw.x, qw.y, qw.z, qw.w, pw.x, pw.y, pw.z};
    double r[6];
    V3 rot, Rt;
    M3 R_ws;
    prior_residual(qw, pw, id_sensor, meas, r, &rot, &R_ws, &Rt);
    const So3Coef sc = so3_coef(dot(rot, rot), true);
    const M3 Arot = mul_nt(rodrigues_poly(rot, 0.5, sc.D), R_ws);
    const M3 Apos = scale(-1.0, hat(Rt));
    for (int j = 0; j < K; ++j) {
      const double Bj = lam[j] - (j + 1 < K ? lam[j + 1] : 0.0);
      const M3 Jr = scale(2.0, mul(Arot, G[j])), Jp = scale(2.0, mul(Apos, G[j]));
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
          J[a * 6 * K + 6 * j + c] = Jr.m[3 * a + c];
          J[a * 6 * K + 6 * j + 3 + c] = 0.0;
          J[(3 + a) * 6 * K + 6 * j + c] = Jp.m[3 * a + c];
          J[(3 + a) * 6 * K + 6 * j + 3 + c] = a == c ? Bj : 0.0;
        }
    }
    first_s[w] = first;
  }
  __syncthreads();
  const int ncb = 6 * T.bw;
  if (active && lane < 6 * K) {  // column `lane` of J Sigma_cp
    const int f6 = 6 * first_s[w];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    for (int m = 0; m < 6 * K; ++m) {
      const double s = cov_band_at(cov, ncb, f6 + m, f6 + lane);
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[a] = fma(J[a * 6 * K + m], s, acc[a]);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) JS[w][a * 6 * K + lane] = acc[a];
  }
  __syncthreads();
  if (active && lane < 36) {
    const int a = lane / 6, b = lane % 6;
    double v = 0.0;
    for (int c = 0; c < 6 * K; ++c) v = fma(JS[w][a * 6 * K + c], J[b * 6 * K + c], v);
    out[36 * size_t(i) + lane] = v;
  }
}

/// v, as a value the optimiser cannot trace back to the expression it came from (through the scalar registers; for a single active lane).
HSD double cov_opaque(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

/// One wave per stamp: the covariance of the SENSOR pose T_ws(t) = T_wb(t) o T_bs (manifold.cpp:54), in the residual coordinates of the pose
/// prior with its measurement at that pose. With J_s (6 x 6K) the state Jacobian of prior_linearize for the sensor and J_e (6 x 6) its
/// Jacobian in the Ceres-local coordinates of T_bs (prior_sensor_jacobians: [2 J_r^-1 R_sb, 0 ; 0, R_wb]), J = [J_s | J_e] and
///   out = J Sigma_aug J',   Sigma_aug = [Sigma_pp, Sigma_pe ; Sigma_pe', Sigma_ee]
/// over the K control points of the segment and the six T_bs coordinates: Sigma_pp from the band (cov), Sigma_pe the columns ecol .. ecol + 5
/// of Sigma_pb (cov_pb, np x nb), Sigma_ee that 6 x 6 block of Sigma_bb (cov_bb, nb x nb), all unscaled. ecol < 0: T_bs is not an unknown of
/// the computed covariance — J = J_s, and for an identity T_bs every operation is k_cov_sample's, in its order. T_bs: seven doubles in device
/// memory (a row of T.cam or T.sensor, T.imu->T_bs). Lane 0 evaluates the spline and J, the lanes below 6K + 6 own one column of J Sigma_aug
/// each, the lanes below 36 one entry of the result; one fixed order in every sum, no atomics: two calls are bit-identical.
template <int K>
__global__ void __launch_bounds__(kBlock) k_cov_sample_sensor(Tables T, const double* cov, const double* cov_pb, const double* cov_bb, int nb,
                                                              const double* T_bs, int ecol, int n, const double* stamps, double* out) {
  constexpr int M = 6 * K + 6;  // row stride of J and of J Sigma_aug
  __shared__ double Js[kBlock / 64][6 * M];
  __shared__ double JS[kBlock / 64][6 * M];
  __shared__ int first_s[kBlock / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, i = blockIdx.x * (kBlock / 64) + w;
  const bool active = i < n;
  const int cols = ecol < 0 ? 6 * K : M;
  double* J = Js[w];
  if (active && lane == 0) {
    double u;
    const int first = segment_of(stamps[i], T.sp.t0, T.sp.dt, K, &u);
    double lam[K], dl[1], ddl[1];
    basis_weights<K>(T.basis, u, T.sp.inv_dt, lam, dl, ddl, 0);
    Quat qw;
    V3 pw;
    M3 G[K];
    spline_pose_jac<K>(T.cp + 8 * first, lam, &qw, &pw, G);
    const double sensor[7] = {T_bs[0], T_bs[1], T_bs[2], T_bs[3], T_bs[4], T_bs[5], T_bs[6]};
    const Quat q_bs{sensor[0], sensor[1], sensor[2], sensor[3]}, q_ws = qmul(qw, q_bs);
    const M3 R_wb = qmat(qw);
    const V3 lever = mul(R_wb, V3{sensor[4], sensor[5], sensor[6]});
    // (the measurement is handed over as a value of its own: prior_residual forms conj(q_m) (x) q_ws, and a compiler that knew q_m to BE q_ws
    //  would contract that product differently from k_cov_sample, where the two are different values — the last bits of an identity sensor)
    const double meas[7] = {cov_opaque(q_ws.x), cov_opaque(q_ws.y), cov_opaque(q_ws.z), cov_opaque(q_ws.w), lever.x + pw.x, lever.y + pw.y, lever.z + pw.z};
    double r[6];
    V3 rot, Rt;
    M3 R_ws;
    prior_residual(qw, pw, sensor, meas, r, &rot, &R_ws, &Rt);
    const So3Coef sc = so3_coef(dot(rot, rot), true);
    const M3 Jri = rodrigues_poly(rot, 0.5, sc.D);
    const M3 Arot = mul_nt(Jri, R_ws);
    const M3 Apos = scale(-1.0, hat(Rt));
    for (int j = 0; j < K; ++j) {
      const double Bj = lam[j] - (j + 1 < K ? lam[j + 1] : 0.0);
      const M3 Jr = scale(2.0, mul(Arot, G[j])), Jp = scale(2.0, mul(Apos, G[j]));
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
          J[a * M + 6 * j + c] = Jr.m[3 * a + c];
          J[a * M + 6 * j + 3 + c] = 0.0;
          J[(3 + a) * M + 6 * j + c] = Jp.m[3 * a + c];
          J[(3 + a) * M + 6 * j + 3 + c] = a == c ? Bj : 0.0;
        }
    }
    if (ecol >= 0) {
      const M3 Erot = scale(2.0, mul_nt(Jri, qmat(q_bs)));  // 2 J_r^-1 R_bs^T
      for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
          J[a * M + 6 * K + c] = Erot.m[3 * a + c];
          J[a * M + 6 * K + 3 + c] = 0.0;
          J[(3 + a) * M + 6 * K + c] = 0.0;
          J[(3 + a) * M + 6 * K + 3 + c] = R_wb.m[3 * a + c];
        }
    }
    first_s[w] = first;
  }
  __syncthreads();
  const int ncb = 6 * T.bw;
  if (active && lane < cols) {  // column `lane` of J Sigma_aug
    const int f6 = 6 * first_s[w];
    double acc[6] = {0, 0, 0, 0, 0, 0};
    if (lane < 6 * K) {
      for (int m = 0; m < 6 * K; ++m) {
        const double s = cov_band_at(cov, ncb, f6 + m, f6 + lane);
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = fma(J[a * M + m], s, acc[a]);
      }
      if (ecol >= 0) {
        const double* pe = cov_pb + size_t(f6 + lane) * nb + ecol;  // (row of Sigma_pe: the column of its transpose)
        for (int m = 0; m < 6; ++m) {
          const double s = pe[m];
#pragma unroll
          for (int a = 0; a < 6; ++a) acc[a] = fma(J[a * M + 6 * K + m], s, acc[a]);
        }
      }
    } else {
      const int e = ecol + lane - 6 * K;
      for (int m = 0; m < 6 * K; ++m) {
        const double s = cov_pb[size_t(f6 + m) * nb + e];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = fma(J[a * M + m], s, acc[a]);
      }
      for (int m = 0; m < 6; ++m) {
        const double s = cov_bb[size_t(ecol + m) * nb + e];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = fma(J[a * M + 6 * K + m], s, acc[a]);
      }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) JS[w][a * M + lane] = acc[a];
  }
  __syncthreads();
  if (active && lane < 36) {
    const int a = lane / 6, b = lane % 6;
    double v = 0.0;
    for (int c = 0; c < cols; ++c) v = fma(JS[w][a * M + c], J[b * M + c], v);
    out[36 * size_t(i) + lane] = v;
  }
}

}  // namespace hs
