// kernels_imucal.hpp — free IMU blocks (T_bs, i_g, i_a, S_g, X_a) as border unknowns of the reduced system (part of kernels.hpp; included
// once by capi.hip through it). DESIGN §14.
//
// A free IMU coordinate is a border column behind gravity and in front of the free camera coordinates:
//   [bias_g 3 n_bias | bias_a 3 n_bias | gravity 2 | IMU ni | camera nc],   IMU group: the free blocks of [T_bs 6 | i_g 6 | i_a 6 | S_g 9 | X_a 9].
// Only inertial residuals touch it, no landmark does: nothing is eliminated, its block of H_bb is plain J'J and finalize_border_body takes
// diag(J'J) and the gradient from H_bb / g_b like for a bias column. Per inertial record, with the robustified rows A = J_state (6 x 6K), the bias
// weights wg, wa, Jg = J_gravity (6 x 2), r and C = J_imu (6 x ni, the free columns of the record's sensor Jacobian):
//   H_pi = sum A'C                                                          (k_imucal_pi: owner = control point, lanes take records)
//   H_{b_g,j ; i} = sum wg[j] C[0:3, :],  H_{b_a,j ; i} = sum wa[j] C[3:6, :]   (k_imucal_bb: per bias control point, lanes take records, in slices)
//   H_ii = sum C'C,  g_i = sum C'r,  H_gi = sum Jg'C                        (k_imucal_ii: per-chunk partials; k_imucal_finish: fixed-order sum)
// The block against the camera columns is exactly zero (the zero fill of k_border_pb). A constant bias spline / constant gravity reach the
// records as zero weights / a zero J_gravity (inertial_linearize_col): their cross terms are sums of exact zeros.
// Every sum has one owner and a fixed order, nothing is accumulated atomically: two builds of a window are bit-identical, and every entry of H_bb
// is written together with its mirror from one value.
#pragma once
#include "kernels_common.hpp"
#include "kernels_sensor.hpp"
#include "kernels_border.hpp"

namespace hs {

constexpr int kImuCalGroup = 6;     // IMU columns per lane group: 6 x 6 accumulators per lane
constexpr int kImuCalChunk = kBlock;  // inertial records per partial of k_imucal_ii (one record per lane)
constexpr int kImuCalBbSlices = 8;   // at most: workgroups a bias point's records are dealt to in k_imucal_bb (a bias point owns ~kb / n_bias of a window's records, and there are few bias points)

/// What the kernels of this file get next to Tables (which keeps the layout every other kernel was compiled for): the table of sensor
/// Jacobians, the column map and the partials. Allocated on handles with a free IMU block only.
struct ImuCal {
  double* rec;     // n_ine x kSensorRecInertial: inertial_sensor_jacobians of every record, at the slot of T.i_rec (segment-major)
  const int* map;  // ni: entry of row 0 of the column inside a record | row stride << 16
  double* part;    // n_chunks x n_jobs x 36: partials of k_imucal_ii
  double* bb_part; // n_bias x n_groups x n_slices x 36: partials of k_imucal_bb
  int ni;          // free IMU coordinates in the system (<= 36: T_bs 6 + i_g 6 + i_a 6 + S_g 9 + X_a 9)
  int col0;        // first IMU column of the border: 6 n_bias + 2
};

/// Groups of kImuCalGroup consecutive IMU columns, and the jobs of k_imucal_ii: job g < n_groups is group g against [r | Jg(:, 0) | Jg(:, 1)],
/// the others are the pairs (ga <= gb) of groups in row-major order.
__host__ __device__ inline int imucal_groups(int ni) { return (ni + kImuCalGroup - 1) / kImuCalGroup; }
/// Slices of k_imucal_bb (its gridDim.z): one per 256 records of the window, at most kImuCalBbSlices.
__host__ __device__ inline int imucal_slices(int n_ine) { return max(1, min(kImuCalBbSlices, (n_ine + kBlock - 1) / kBlock)); }
__host__ __device__ inline int imucal_jobs(int ni) {
  const int g = imucal_groups(ni);
  return g + g * (g + 1) / 2;
}
HSD void imucal_pair(int n_groups, int job, int* ga, int* gb) {
  int a = 0, rest = job - n_groups;
  while (rest >= n_groups - a) rest -= n_groups - a, ++a;
  *ga = a, *gb = a + rest;
}

/// The map entries of group `grp`; columns past ni repeat the last one (read, never written out).
HSD void imucal_group_map(const ImuCal& A, int grp, int (&off)[kImuCalGroup], int (&str)[kImuCalGroup]) {
#pragma unroll
  for (int c = 0; c < kImuCalGroup; ++c) {
    const int m = A.map[min(kImuCalGroup * grp + c, A.ni - 1)];
    off[c] = m & 0xffff, str[c] = m >> 16;
  }
}

/// One lane per inertial record: its 6 x 36 sensor Jacobian (Ceres-local coordinates, robustified, in the Jacobian mode of
/// hs_set_inertial_jacobian) straight into the table.
template <int K>
__global__ void __launch_bounds__(kBlock) k_imucal_rows(Tables T, ImuCal A) {
  if (T.st->done) return;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T.n_ine) return;
  inertial_sensor_jacobians<K, 4>(T, T.cp, i, true, A.rec + size_t(i) * kSensorRecInertial);
}

/// H_pi. Workgroup (i, g): control point i against column group g. The lanes walk the records of the <= K segments that reach i (contiguous
/// in the segment-major table) with stride 256, 6 x 6 sums in registers, then one butterfly per sum (the gravity wave of k_border_pb) and the
/// waves in index order. Rows 6 i .. 6 i + 5 of the IMU columns of the H_pb partials: split 0 carries the value, the other splits are zero.
template <int K>
__global__ void __launch_bounds__(kBlock) k_imucal_pi(Tables T, ImuCal A, int n_splits) {
  __shared__ double red[kBlock / 64][6 * kImuCalGroup];
  if (T.st->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x, grp = blockIdx.y, c0 = kImuCalGroup * grp, nb = T.nb;
  const int IREC = 18 + 36 * K + 2 * T.kb;
  int off[kImuCalGroup], str[kImuCalGroup];
  imucal_group_map(A, grp, off, str);
  const int f0 = max(0, i - K + 1), f1 = min(i, T.n_seg - 1);
  const int p0 = T.i_seg_ptr[f0], p1 = T.i_seg_ptr[f1 + 1];
  int seg_end[K];  // (k_border_pb: first control point of record pos = f0 + #{j : pos >= seg_end[j]})
#pragma unroll
  for (int j = 0; j < K; ++j) seg_end[j] = T.i_seg_ptr[min(f0 + j + 1, T.n_seg)];
  double acc[6][kImuCalGroup];
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < kImuCalGroup; ++c) acc[a][c] = 0.0;
  for (int pos = p0 + tid; pos < p1; pos += kBlock) {
    int f = f0;
#pragma unroll
    for (int j = 0; j < K - 1; ++j) f += pos >= seg_end[j] ? 1 : 0;
    f = min(f, f1);
    const double* jp = T.i_rec + size_t(pos) * IREC + 6 + 6 * (i - f);
    const double* sj = A.rec + size_t(pos) * kSensorRecInertial;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double cv[kImuCalGroup];
#pragma unroll
      for (int c = 0; c < kImuCalGroup; ++c) cv[c] = sj[off[c] + r * str[c]];
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double v = jp[r * 6 * K + a];
#pragma unroll
        for (int c = 0; c < kImuCalGroup; ++c) acc[a][c] = fma(v, cv[c], acc[a][c]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int c = 0; c < kImuCalGroup; ++c) {
      const double v = wave_sum_fast(acc[a][c]);
      if (lane == 0) red[wave][kImuCalGroup * a + c] = v;
    }
  __syncthreads();
  const int nv = min(kImuCalGroup, A.ni - c0);
  double* out = T.xpart + T.xo_pb + size_t(6 * i) * nb + A.col0 + c0;
  if (tid < 6 * kImuCalGroup && tid % kImuCalGroup < nv) {
    double t = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) t += red[w][tid];
    out[size_t(tid / kImuCalGroup) * nb + tid % kImuCalGroup] = t;
  }
  for (int e = tid; e < 6 * nv * (n_splits - 1); e += kBlock) {
    const int sp = 1 + e / (6 * nv), a = (e % (6 * nv)) / nv, c = e % nv;
    out[size_t(sp) * T.x_count1 + size_t(a) * nb + c] = 0.0;
  }
}

/// Bias cross block, partials. Workgroup (b, g, z): bias control point b (gyro and accel parts) against column group g, over slice z of the
/// records whose bias window covers b (T.i_bias_ptr, as k_border_bb: rounds z, z + gridDim.z, .. of 256 records), one record per lane
/// and round; wave sums, then the waves in index order -> A.bb_part. k_imucal_finish adds the slices in index order and is the single writer
/// of each entry of H_bb and its mirror. (A bias point owns ~kb / n_bias of a window's records and there are few bias points: one workgroup per
/// (b, g) would leave most of the chip idle.)
template <int K>
__global__ void __launch_bounds__(kBlock) k_imucal_bb(Tables T, ImuCal A) {
  __shared__ double red[kBlock / 64][6 * kImuCalGroup];
  if (T.st->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x, grp = blockIdx.y, z = blockIdx.z, n_slices = gridDim.z;
  const int kb = T.kb;
  const int IREC = 18 + 36 * K + 2 * kb;
  int off[kImuCalGroup], str[kImuCalGroup];
  imucal_group_map(A, grp, off, str);
  const int p0 = T.i_bias_ptr[max(0, b - kb + 1)], p1 = T.i_bias_ptr[b + 1];
  double acc[6][kImuCalGroup];  // rows 0 - 2: gyro bias of b, rows 3 - 5: accel bias of b
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < kImuCalGroup; ++c) acc[r][c] = 0.0;
  for (int pos = p0 + z * kBlock + tid; pos < p1; pos += n_slices * kBlock) {
    const double* rec = T.i_rec + size_t(pos) * IREC;
    const double* sj = A.rec + size_t(pos) * kSensorRecInertial;
    const int j = b - T.i_first_bias[pos];
    const double* wgp = rec + 6 + 36 * K;
    const double* wap = wgp + kb;
    double wgb, wab;
    if (kb == 4) {  // (wave uniform; sel4: no load depends on j)
      const double wg4[4] = {wgp[0], wgp[1], wgp[2], wgp[3]}, wa4[4] = {wap[0], wap[1], wap[2], wap[3]};
      wgb = sel4(wg4, j), wab = sel4(wa4, j);
    } else {
      wgb = wgp[j], wab = wap[j];  // (0 <= j < kb inside the range of b)
    }
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const double w = r < 3 ? wgb : wab;
#pragma unroll
      for (int c = 0; c < kImuCalGroup; ++c) acc[r][c] = fma(w, sj[off[c] + r * str[c]], acc[r][c]);
    }
  }
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = 0; c < kImuCalGroup; ++c) {
      const double v = wave_sum_fast(acc[r][c]);
      if (lane == 0) red[wave][kImuCalGroup * r + c] = v;
    }
  __syncthreads();
  if (tid >= 6 * kImuCalGroup) return;
  double t = 0.0;
  for (int w = 0; w < kBlock / 64; ++w) t += red[w][tid];
  A.bb_part[((size_t(b) * gridDim.y + grp) * n_slices + z) * (6 * kImuCalGroup) + tid] = t;
}

/// Partials of H_ii, g_i and H_gi. Workgroup (w, job): records w kImuCalChunk .. of the table, one per lane; job: imucal_jobs. 36 sums per
/// lane, wave sums, then the waves in index order -> A.part[(w n_jobs + job) 36 ..].
template <int K>
__global__ void __launch_bounds__(kBlock) k_imucal_ii(Tables T, ImuCal A) {
  __shared__ double red[kBlock / 64][kImuCalGroup * kImuCalGroup];
  if (T.st->done) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int w = blockIdx.x, job = blockIdx.y, n_groups = imucal_groups(A.ni), n_jobs = imucal_jobs(A.ni);
  const int IREC = 18 + 36 * K + 2 * T.kb;
  const bool extras = job < n_groups;
  int ga = job, gb = job;
  if (!extras) imucal_pair(n_groups, job, &ga, &gb);
  int offa[kImuCalGroup], stra[kImuCalGroup], offb[kImuCalGroup], strb[kImuCalGroup];
  imucal_group_map(A, ga, offa, stra);
  imucal_group_map(A, gb, offb, strb);
  double acc[kImuCalGroup][kImuCalGroup];
#pragma unroll
  for (int a = 0; a < kImuCalGroup; ++a)
#pragma unroll
    for (int c = 0; c < kImuCalGroup; ++c) acc[a][c] = 0.0;
  const int pos = w * kImuCalChunk + tid;
  if (pos < T.n_ine) {
    const double* rec = T.i_rec + size_t(pos) * IREC;
    const double* jg = rec + 6 + 36 * K + 2 * T.kb;
    const double* sj = A.rec + size_t(pos) * kSensorRecInertial;
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      double ca[kImuCalGroup], cb[kImuCalGroup];
#pragma unroll
      for (int c = 0; c < kImuCalGroup; ++c) ca[c] = sj[offa[c] + r * stra[c]];
      if (extras) {  // (workgroup uniform)
        cb[0] = rec[r], cb[1] = jg[2 * r], cb[2] = jg[2 * r + 1];
#pragma unroll
        for (int c = 3; c < kImuCalGroup; ++c) cb[c] = 0.0;
      } else {
#pragma unroll
        for (int c = 0; c < kImuCalGroup; ++c) cb[c] = sj[offb[c] + r * strb[c]];
      }
#pragma unroll
      for (int a = 0; a < kImuCalGroup; ++a)
#pragma unroll
        for (int c = 0; c < kImuCalGroup; ++c) acc[a][c] = fma(ca[a], cb[c], acc[a][c]);
    }
  }
#pragma unroll
  for (int a = 0; a < kImuCalGroup; ++a)
#pragma unroll
    for (int c = 0; c < kImuCalGroup; ++c) {
      const double v = wave_sum_fast(acc[a][c]);
      if (lane == 0) red[wave][kImuCalGroup * a + c] = v;
    }
  __syncthreads();
  if (tid >= kImuCalGroup * kImuCalGroup) return;
  double t = 0.0;
  for (int v = 0; v < kBlock / 64; ++v) t += red[v][tid];
  A.part[(size_t(w) * n_jobs + job) * (kImuCalGroup * kImuCalGroup) + tid] = t;
}

/// One thread per entry of a job: the partials of k_imucal_ii in workgroup order into the IMU block of the exchange buffer (H_bb with the
/// gravity cross block, g_b). Diagonal pairs write their upper triangle; every entry goes out together with its mirror. Behind the jobs, one
/// thread per entry of the bias cross block: the slices of k_imucal_bb in index order.
__global__ void __launch_bounds__(kBlock) k_imucal_finish(Tables T, ImuCal A, int n_chunks, int n_slices) {
  if (T.st->done) return;
  constexpr int E = kImuCalGroup * kImuCalGroup;
  const int n_groups = imucal_groups(A.ni), n_jobs = imucal_jobs(A.ni), nb = T.nb;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  double* Hbb = T.xbuf + T.xo_bb;
  if (e >= n_jobs * E) {
    const int e2 = e - n_jobs * E, bg = e2 / E, t = e2 % E;
    if (bg >= T.n_bias * n_groups) return;
    const int b = bg / n_groups, r = t / kImuCalGroup, ci = kImuCalGroup * (bg % n_groups) + t % kImuCalGroup;
    double v[kImuCalBbSlices], sum = 0.0;
#pragma unroll
    for (int z = 0; z < kImuCalBbSlices; ++z) v[z] = z < n_slices ? A.bb_part[(size_t(bg) * n_slices + z) * E + t] : 0.0;
#pragma unroll
    for (int z = 0; z < kImuCalBbSlices; ++z) sum += v[z];
    if (ci >= A.ni) return;
    const int row = (r < 3 ? 0 : 3 * T.n_bias) + 3 * b + r % 3, col = A.col0 + ci;
    Hbb[size_t(row) * nb + col] = sum, Hbb[size_t(col) * nb + row] = sum;
    return;
  }
  const int job = e / E, a = (e % E) / kImuCalGroup, c = e % kImuCalGroup;
  double s = 0.0;
  for (int w0 = 0; w0 < n_chunks; w0 += 8) {  // (eight partials in flight, added in workgroup order)
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = w0 + u < n_chunks ? A.part[(size_t(w0 + u) * n_jobs + job) * E + e % E] : 0.0;
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  if (job < n_groups) {
    const int ca = kImuCalGroup * job + a;
    if (ca >= A.ni || c > 2) return;
    if (c == 0) {
      T.xbuf[T.xo_gb + A.col0 + ca] = s;
    } else {
      const int row = A.col0 - 2 + (c - 1);  // gravity columns
      Hbb[size_t(row) * nb + A.col0 + ca] = s, Hbb[size_t(A.col0 + ca) * nb + row] = s;
    }
    return;
  }
  int ga, gb;
  imucal_pair(n_groups, job, &ga, &gb);
  const int ca = kImuCalGroup * ga + a, cb = kImuCalGroup * gb + c;
  if (ca >= A.ni || cb >= A.ni || (ga == gb && a > c)) return;
  Hbb[size_t(A.col0 + ca) * nb + A.col0 + cb] = s, Hbb[size_t(A.col0 + cb) * nb + A.col0 + ca] = s;
}

// ---------------------------------------------------------------------------------------------------------------------
// Solve side (hs_set_imu_estimation): the candidate IMU parameters and the commit of an accepted step. Both are one-workgroup launches of
// their own on handles that estimate IMU blocks; handles without launch neither.
// ---------------------------------------------------------------------------------------------------------------------

constexpr int kImuParamDoubles = int(sizeof(ImuParams) / sizeof(double));  // [T_bs 7 | i_g 6 | i_a 6 | S_g 9 | X_a 9]
static_assert(kImuParamDoubles == 37 && kImuParamDoubles <= kBlock, "ImuParams is 37 doubles, copied one per lane");

/// Candidate IMU parameters from the unscaled border step di = T.delta_b[A.col0 ..]: *cand (a buffer next to *T.imu that only the launches of a
/// handle that estimates IMU blocks know: Tables keeps the layout every other kernel was compiled for) = *T.imu with every free block
/// retracted — T_bs on Product(EigenQuaternion, R3) (q <- dq(d_rot) (x) q, p <- p + d_trans), i_g, i_a, S_g, X_a Euclidean in the parameter
/// layout. One lane per IMU column (ni <= 36) through the column map (entry of row 0 inside a record of sensor Jacobians: T_bs from 0, i_g 36,
/// i_a 72, S_g 108, X_a 162); the lane of the T_bs block's first column retracts the block. Also the IMU blocks' share of the decision:
/// T.norm_part[2 norm_slot ..] = (|x|^2, |x+ - x|^2) over the ambient coordinates of the free blocks, summed in lane order per wave, waves in
/// index order. No gradient term: the IMU block is not a Schur complement, T.gb_s holds the full gradient on these columns.
__global__ void __launch_bounds__(kBlock) k_imucal_candidate(Tables T, ImuCal A, ImuParams* cand, int norm_slot) {
  if (T.st->done) return;
  __shared__ double red[2 * (kBlock / 64)];
  const int tid = threadIdx.x;
  const double* x = reinterpret_cast<const double*>(T.imu);
  double* y = reinterpret_cast<double*>(cand);
  if (tid < kImuParamDoubles) y[tid] = x[tid];
  __syncthreads();
  double v[2] = {0.0, 0.0};  // |x|^2, |x+ - x|^2
  if (tid < A.ni) {
    const int o = A.map[tid] & 0xffff;
    const double* d = T.delta_b + A.col0 + tid;
    if (o == 0) {  // T_bs: its six columns are consecutive
      const Quat q = quat_plus(Quat{x[0], x[1], x[2], x[3]}, V3{d[0], d[1], d[2]});
      y[0] = q.x, y[1] = q.y, y[2] = q.z, y[3] = q.w, y[4] = x[4] + d[3], y[5] = x[5] + d[4], y[6] = x[6] + d[5];
#pragma unroll
      for (int c = 0; c < 7; ++c) v[0] = fma(x[c], x[c], v[0]), v[1] = fma(y[c] - x[c], y[c] - x[c], v[1]);
    } else if (o >= 36) {  // i_g at 7 .., i_a at 13 .., S_g at 19 .., X_a at 28 .. of the parameter layout
      const int at = o < 72 ? 7 + (o - 36) : o < 108 ? 13 + (o - 72) : o < 162 ? 19 + (o - 108) : 28 + (o - 162);
      const double xv = x[at], yv = xv + d[0];
      y[at] = yv;
      v[0] = xv * xv, v[1] = (yv - xv) * (yv - xv);
    }
  }
  block_sum_n<2>(v, red);
  if (tid == 0) T.norm_part[2 * norm_slot] = v[0], T.norm_part[2 * norm_slot + 1] = v[1];
}

/// *imu <- candidate when the step was accepted (k_commit's rule: `accepted` is read even when a convergence test just ended the solve).
__global__ void __launch_bounds__(kBlock) k_imucal_commit(Tables T, ImuParams* imu, const ImuParams* cand) {
  if (!T.st->accepted) return;
  if (threadIdx.x < kImuParamDoubles) reinterpret_cast<double*>(imu)[threadIdx.x] = reinterpret_cast<const double*>(cand)[threadIdx.x];
}

}  // namespace hs
