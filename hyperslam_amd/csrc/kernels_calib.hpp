// kernels_calib.hpp — free camera blocks (T_bs, intrinsics, distortion) as border unknowns of the reduced system (part of kernels.hpp;
// included once by capi.hip through it). DESIGN §13.
//
// A free camera coordinate is a border column behind the bias / gravity columns (Tables::nc of them, from column T.nb - T.nc on). Visual
// residuals couple it with the control points AND the landmarks, so the landmark elimination gains cross terms. Per landmark l, with the
// robustified rows A = J_pose, B = J_landmark, C = J_camera and the factors the build left behind (V = S_l H_ll S_l + D_l^2 = L L' in
// T.lm_L, Yh = H_pl S_l L^-T in T.Y, yh = L^-1 S_l b_l in T.lm_yhat):
//   H_lc = sum B'C,  Y_c = L^-1 S_l H_lc                          (k_calib_landmark, stored per landmark)
//   H_pc = sum A'C - sum_l Yh_l Y_c,l                             (k_calib_pc: one workgroup per block row, owner computes)
//   H_cc = sum C'C - sum_l Y_c,l' Y_c,l,  g_c = sum C'r - sum_l Y_c,l' yh_l,  diag(J'J)_c = sum diag(C'C)
//                                                                 (k_calib_cc: per-chunk partials; k_calib_finish: fixed-order sum)
// Pose and camera sides are unscaled here; finalize_border_body scales and damps them like every other border column (Jacobi scale from
// the undamped diag(J'J)_c, which the Schur complement does not touch). Constant landmarks carry no Y_c (their rows still add A'C, C'C, C'r).
// Every sum has one owner and a fixed order: two builds of a window are bit-identical.
#pragma once
#include "kernels_common.hpp"

namespace hs {

constexpr int kCalibMaxCols = 64;    // free camera coordinates per window (one lane per column in k_calib_landmark)
constexpr int kCalibRowChunk = 256;  // visual records per partial of k_calib_cc
constexpr int kCalibLmChunk = 64;    // landmarks per partial of k_calib_cc

/// Record of one visual residual block for the camera columns, at its segment-major slot (T.v_pos): [r(2) | J_landmark 2 x 3 |
/// J_camera 2 x 14 ([T_bs 6 | intrinsics 4 | distortion 4] per row) | camera | first control point | J_pose 2 x 6K], robustified.
template <int K>
constexpr int calib_record() { return 40 + 12 * K; }

template <int K>
__global__ void __launch_bounds__(kBlock) k_calib_rows(Tables T) {
  if (T.st->done) return;
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= T.n_vis) return;
  VisualOut<K> o;
  visual_linearize<K>(T, T.cp, q, true, &o);
  double sj[kSensorRecVisual];
  visual_sensor_jacobians<K>(T, T.cp, q, true, sj);
  double* rec = T.calib_rec + size_t(T.v_pos[q]) * calib_record<K>();
  rec[0] = o.r[0], rec[1] = o.r[1];
#pragma unroll
  for (int c = 0; c < 6; ++c) rec[2 + c] = o.Jl[c];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
#pragma unroll
    for (int c = 0; c < 6; ++c) rec[8 + 14 * i + c] = sj[6 * i + c];
#pragma unroll
    for (int c = 0; c < 4; ++c) rec[8 + 14 * i + 6 + c] = sj[12 + 4 * i + c], rec[8 + 14 * i + 10 + c] = sj[20 + 4 * i + c];
  }
  rec[36] = double(T.v_info[q] & 0xffff), rec[37] = double(T.v_first[q]);
  rec[38] = rec[39] = 0.0;
#pragma unroll
  for (int c = 0; c < 12 * K; ++c) rec[40 + c] = o.Jp[c];
}

/// Column c of the camera border in row `row` of a record: the record's camera owns it (T.calib_map[c] = camera << 8 | local column) or 0.
HSD double calib_jc(const Tables& T, const double* rec, int row, int c) {
  const int m = T.calib_map[c];
  return int(rec[36]) == (m >> 8) ? rec[8 + 14 * row + (m & 0xff)] : 0.0;
}

/// One wave per landmark, one lane per camera column: H_lc = sum B'C over the landmark's records, Y_c = L^-1 S_l H_lc -> T.calib_Yc
/// (3 x nc per landmark). Constant and unobserved landmarks are not eliminated: zero.
__global__ void __launch_bounds__(kBlock) k_calib_landmark(Tables T) {
  if (T.st->done) return;
  const int dl = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), c = threadIdx.x & 63;
  if (dl >= T.n_lm || c >= T.nc) return;
  double* out = T.calib_Yc + size_t(dl) * 3 * T.nc;
  const int q0 = T.lm_ptr[dl], q1 = T.lm_ptr[dl + 1];
  if (q0 == q1 || T.lm_const[dl]) {
    out[c] = out[T.nc + c] = out[2 * T.nc + c] = 0.0;
    return;
  }
  const int stride = 40 + 12 * T.sp.k;  // (calib_record<K>: the landmark / camera part does not depend on K, only the stride does)
  double h0 = 0.0, h1 = 0.0, h2 = 0.0;
  for (int q = q0; q < q1; ++q) {
    const double* rec = T.calib_rec + size_t(T.v_pos[q]) * stride;
#pragma unroll
    for (int row = 0; row < 2; ++row) {
      const double jc = calib_jc(T, rec, row, c);
      h0 = fma(rec[2 + 3 * row], jc, h0), h1 = fma(rec[2 + 3 * row + 1], jc, h1), h2 = fma(rec[2 + 3 * row + 2], jc, h2);
    }
  }
  const double* sl = T.lm_scale + 3 * size_t(dl);
  const double* L = T.lm_L + 6 * size_t(dl);
  const double w0 = sl[0] * h0, w1 = sl[1] * h1, w2 = sl[2] * h2;
  const double y0 = w0 / L[0], y1 = (w1 - L[1] * y0) / L[2], y2 = (w2 - L[3] * y0 - L[4] * y1) / L[5];
  out[c] = y0, out[T.nc + c] = y1, out[2 * T.nc + c] = y2;
}

/// One workgroup per control point i: rows 6 i .. 6 i + 5 of H_pc into the camera columns of the H_pb partials (split 0; the other splits of
/// those columns are zero), in segment order over the records of the <= K segments that reach i, then in landmark order over the Y-hat term.
template <int K>
__global__ void __launch_bounds__(kBlock) k_calib_pc(Tables T, int n_splits) {
  if (T.st->done) return;
  const int i = blockIdx.x, nc = T.nc, nb = T.nb, nbi = T.nb - T.nc;
  const int f0 = max(0, i - K + 1), f1 = min(i, T.n_seg - 1);
  const int l0 = T.cf_ptr[max(0, i - T.bw + 1)], l1 = T.cf_ptr[i + 1];
  for (int e = threadIdx.x; e < 6 * nc; e += blockDim.x) {
    const int r = e / nc, c = e % nc;
    double acc = 0.0;
    for (int f = f0; f <= f1; ++f) {
      const int col = 6 * (i - f) + r;
      for (int pos = T.v_seg_ptr[f]; pos < T.v_seg_ptr[f + 1]; ++pos) {
        const double* rec = T.calib_rec + size_t(pos) * calib_record<K>();
#pragma unroll
        for (int row = 0; row < 2; ++row) acc = fma(rec[40 + 6 * K * row + col], calib_jc(T, rec, row, c), acc);
      }
    }
    for (int dl = l0; dl < l1; ++dl) {
      const int cf = T.lm_cfirst[dl];
      if (T.lm_ptr[dl + 1] == T.lm_ptr[dl] || T.lm_const[dl] || i >= cf + T.lm_ncp[dl]) continue;
      const double* Y = T.Y + T.lm_yoff[dl] + 3 * (6 * (i - cf) + r);
      const double* Yc = T.calib_Yc + size_t(dl) * 3 * nc + c;
      acc -= Y[0] * Yc[0] + Y[1] * Yc[nc] + Y[2] * Yc[2 * nc];
    }
    const size_t at = T.xo_pb + size_t(6 * i + r) * nb + nbi + c;
    for (int sp = 0; sp < n_splits; ++sp) T.xpart[size_t(sp) * T.x_count1 + at] = sp == 0 ? acc : 0.0;
  }
}

/// Partials of H_cc, g_c and diag(J'J)_c ([nc x nc | nc | nc] per workgroup): workgroups 0 .. n_row_chunks - 1 sum C'C, C'r over
/// kCalibRowChunk records each (segment-major slots), the others subtract Y_c' Y_c and Y_c' yh over kCalibLmChunk landmarks each.
__global__ void __launch_bounds__(kBlock) k_calib_cc(Tables T, int n_row_chunks) {
  if (T.st->done) return;
  const int nc = T.nc, E = nc * nc + 2 * nc, w = blockIdx.x;
  const int stride = 40 + 12 * T.sp.k;
  double* part = T.calib_part + size_t(w) * E;
  for (int e = threadIdx.x; e < E; e += blockDim.x) {
    const int a = e < nc * nc ? e / nc : (e - nc * nc) % nc, b = e < nc * nc ? e % nc : -1;
    const int kind = e < nc * nc ? 0 : e < nc * nc + nc ? 1 : 2;  // H_cc | g_c | diag
    double acc = 0.0;
    if (w < n_row_chunks) {
      const int p1 = min(T.n_vis, (w + 1) * kCalibRowChunk);
      for (int pos = w * kCalibRowChunk; pos < p1; ++pos) {
        const double* rec = T.calib_rec + size_t(pos) * stride;
#pragma unroll
        for (int row = 0; row < 2; ++row) {
          const double ja = calib_jc(T, rec, row, a);
          const double other = kind == 0 ? calib_jc(T, rec, row, b) : kind == 1 ? rec[row] : ja;
          acc = fma(ja, other, acc);
        }
      }
    } else if (kind != 2) {
      const int lw = w - n_row_chunks, d1 = min(T.n_lm, (lw + 1) * kCalibLmChunk);
      for (int dl = lw * kCalibLmChunk; dl < d1; ++dl) {
        const double* Yc = T.calib_Yc + size_t(dl) * 3 * nc;
        const double* yh = T.lm_yhat + 3 * size_t(dl);
        const bool elim = T.lm_ptr[dl + 1] > T.lm_ptr[dl] && !T.lm_const[dl];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const double o = kind == 0 ? Yc[u * nc + b] : yh[u];
          acc -= elim ? Yc[u * nc + a] * o : 0.0;
        }
      }
    }
    part[e] = acc;
  }
}

/// One thread per entry: the partials of k_calib_cc in workgroup order into the camera block of the exchange buffer (H_bb, g_b) and
/// diag(J'J)_c (Tables::xo_cdj). The cross block bias / gravity x camera is zero (k_border_pb's zero fill, or no IMU).
/// n_row_chunks >= 0: the sum of the row partials alone, C'r — the FULL gradient of the camera columns, which the gradient tolerance test and the
/// model cost change take (g_b holds the reduced one) — goes behind the diagonal, T.xbuf[T.xo_cdj + nc ..].
__global__ void __launch_bounds__(kBlock) k_calib_finish(Tables T, int n_parts, int n_row_chunks = -1) {
  if (T.st->done) return;
  const int nc = T.nc, E = nc * nc + 2 * nc, nb = T.nb, nbi = T.nb - T.nc;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double s = 0.0, rows = 0.0;
  for (int w = 0; w < n_parts; ++w) {
    s += T.calib_part[size_t(w) * E + e];
    if (w + 1 == n_row_chunks) rows = s;
  }
  if (e < nc * nc)
    T.xbuf[T.xo_bb + size_t(nbi + e / nc) * nb + nbi + e % nc] = s;
  else if (e < nc * nc + nc) {
    T.xbuf[T.xo_gb + nbi + e - nc * nc] = s;
    if (n_row_chunks >= 0) T.xbuf[T.xo_cdj + nc + e - nc * nc] = rows;
  } else
    T.xbuf[T.xo_cdj + e - nc * nc - nc] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Solve side (hs_set_camera_estimation): the candidate camera table and the commit of an accepted step. Both are one-workgroup launches
// of their own on handles with free camera coordinates; handles without launch neither.
// ---------------------------------------------------------------------------------------------------------------------

/// Candidate cameras from the unscaled border step dc = T.delta_b[nb - nc ..]: cam_cand (n_cam x 16, a table next to T.cam that only the
/// launches of a handle with free camera coordinates know: Tables keeps the layout every other kernel was compiled for) = T.cam with every free block retracted — T_bs on
/// Product(EigenQuaternion, R3) (q <- dq(d_rot) (x) q, p <- p + d_trans), intrinsics and distortion Euclidean. One lane per camera column
/// (nc <= kCalibMaxCols); the lane of a T_bs block's first column retracts the block. Also the camera blocks' share of the decision:
///   T.norm_part[2 norm_slot ..] = (|x|^2, |x+ - x|^2) over the ambient coordinates of the free blocks (Ceres' x_norm / step_norm), and
///   DevState::g_dot_step_far    = (g_c - g_c,reduced) . dc: the step outputs of the border sweeps form g . step with T.gb_s, which holds the
///                                 REDUCED gradient on the camera columns; the model cost change takes the full one (C'r, k_calib_finish).
///                                 One-ended solves leave this slot zero, and a handle with free cameras is always solved one-ended.
__global__ void __launch_bounds__(kBlock) k_calib_candidate(Tables T, double* cam_cand, int norm_slot) {
  if (T.st->done) return;
  __shared__ double red[3 * (kBlock / 64)];
  const int tid = threadIdx.x, nc = T.nc, nbi = T.nb - T.nc;
  for (int e = tid; e < kCamStride * T.n_cam; e += kBlock) cam_cand[e] = T.cam[e];
  __syncthreads();
  double v[3] = {0.0, 0.0, 0.0};  // |x|^2, |x+ - x|^2, (g - g_reduced) . step
  if (tid < nc) {
    const int m = T.calib_map[tid], col = m & 0xff;
    const double* x = T.cam + kCamStride * (m >> 8);
    double* y = cam_cand + kCamStride * (m >> 8);
    const double* d = T.delta_b + nbi + tid;
    if (col == 0) {  // T_bs: its six columns are consecutive
      const Quat q = quat_plus(Quat{x[0], x[1], x[2], x[3]}, V3{d[0], d[1], d[2]});
      y[0] = q.x, y[1] = q.y, y[2] = q.z, y[3] = q.w, y[4] = x[4] + d[3], y[5] = x[5] + d[4], y[6] = x[6] + d[5];
#pragma unroll
      for (int c = 0; c < 7; ++c) v[0] = fma(x[c], x[c], v[0]), v[1] = fma(y[c] - x[c], y[c] - x[c], v[1]);
    } else if (col >= 6) {  // intrinsics [cx cy fx fy] at 7 .., distortion [k1 k2 p1 p2] at 11 ..
      const double xv = x[1 + col], yv = xv + d[0];
      y[1 + col] = yv;
      v[0] = xv * xv, v[1] = (yv - xv) * (yv - xv);
    }
    v[2] = (T.xbuf[T.xo_cdj + nc + tid] - T.xbuf[T.xo_gb + nbi + tid]) * d[0];
  }
  block_sum_n<3>(v, red);
  if (tid == 0) {
    T.norm_part[2 * norm_slot] = v[0], T.norm_part[2 * norm_slot + 1] = v[1];
    T.st->g_dot_step_far = v[2];
  }
}

/// cam <- candidate when the step was accepted (k_commit's rule: `accepted` is read even when a convergence test just ended the solve).
__global__ void __launch_bounds__(kBlock) k_calib_commit(Tables T, double* cam, const double* cam_cand) {
  if (!T.st->accepted) return;
  for (int e = threadIdx.x; e < kCamStride * T.n_cam; e += kBlock) cam[e] = cam_cand[e];
}

}  // namespace hs
