// backward_pm_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_backward_pm.py): the backward sweep with one phase per super-step on
// premultiplied blocks (k_band_backward_pm, hyperslam_amd/csrc/kernels_backward_sb.hpp) next to the two-phase sweep it replaces
// (k_band_backward_sb), both compiled FROM THE PRODUCT'S KERNEL SOURCE for the host (tests/emul/hip/hip_runtime.h: one std::thread per
// lane) and run on the factor the product's factorisation kernels leave of a band system a Python test hands over:
//   two-ended: k_band_factor_mx from both ends, one-ended: k_band_factor_la behind k_factor_decoupled_rows — launch_factor's jobs and shapes.
// Output: the factor rows of both jobs, the stacked blocks [Winv_J ; U[above, J] Winv_J] of both jobs, and per sweep the solution, the
// step, the scaled step and the two sums of the model cost change.
// Usage: backward_pm_harness <system.bin> <out.bin>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hip/hip_runtime.h"

thread_local dim3 threadIdx;
thread_local unsigned hs_emul::exchange_count = 0;
dim3 blockIdx, blockDim, gridDim;

#include "../../hyperslam_amd/csrc/kernels_common.hpp"
#include "../../hyperslam_amd/csrc/kernels_linearize.hpp"
#include "../../hyperslam_amd/csrc/kernels_sensor.hpp"
#include "../../hyperslam_amd/csrc/kernels_schur.hpp"
#include "../../hyperslam_amd/csrc/kernels_border.hpp"
#include "../../hyperslam_amd/csrc/kernels_factor.hpp"
#include "../../hyperslam_amd/csrc/kernels_factor_mx.hpp"
#include "../../hyperslam_amd/csrc/kernels_backward_sb.hpp"

namespace hs {
HSD void begin_iteration(const Tables&, double, double, bool) {}  // (Tables::bookkeep = 0 in the harness: never reached)
}  // namespace hs

using namespace hs;

template <class T>
static std::vector<T> read_vec(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}
static void write_vec(FILE* f, const std::vector<double>& v) { fwrite(v.data(), sizeof(double), v.size(), f); }

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const std::vector<int> hdr = read_vec<int>(in, 4);  // np, bw, two-ended | f0 << 8, 0
  const int np = hdr[0], bw = hdr[1], two_ended = hdr[2] & 1, f0 = hdr[2] >> 8, ncb = 6 * bw, n_blk = np / 6, w_mid = bw - 1;
  const std::vector<double> Sb = read_vec<double>(in, size_t(np) * ncb), g = read_vec<double>(in, np);
  const std::vector<double> Sb2 = read_vec<double>(in, size_t(np) * ncb), g2 = read_vec<double>(in, np);  // the reversed system
  const std::vector<double> scale_p = read_vec<double>(in, np), g_full = read_vec<double>(in, np), D2p = read_vec<double>(in, np);
  fclose(in);
  if (6 * (bw - 1) > 96 || la_compute_waves(bw) == 0 || (two_ended && (!mx_fits(bw) || n_blk < 4 * bw || f0 > 0)) || f0 >= n_blk) {
    fprintf(stderr, "system outside the kernels' range\n");
    return 3;
  }
  std::vector<double> Ub(size_t(np) * ncb, 0.0), Ubk(size_t(24) * n_blk, 0.0), yb(np, 0.0), Ub2 = Ub, Ubk2 = Ubk, yb2 = yb;
  std::vector<double> win(size_t(6 * w_mid) * (ncb + 1), 0.0), xpart(8 * 1024, 0.0);
  DevState st{};
  std::vector<unsigned> join_flag(kBfFlagBase + 512 + 4 * kProgressStride, 0u);
  Tables T{};
  T.np = np, T.bw = bw, T.st = &st, T.join_flag = join_flag.data(), T.join_epoch = 1, T.xpart = xpart.data();
  T.Sb = const_cast<double*>(Sb.data()), T.g_s = const_cast<double*>(g.data()), T.Ub = Ub.data(), T.Ubk = Ubk.data(), T.ybuf = yb.data();
  static const double zero = 0.0;
  int m = -1, mB = 0;
  // ---- the factorisation (launch_factor) ----
  if (two_ended) {
    m = std::min((n_blk - w_mid) / 2 + two_ended_lead(true), n_blk - w_mid - w_mid), mB = n_blk - w_mid - m;
    T.mj[0] = MfmaJob{Sb2.data(), g.data(), Ub.data(), Ubk.data(), yb.data(), win.data(), m + w_mid, m, m + w_mid, INT_MAX, 0, &zero};
    T.mj[1] = MfmaJob{Sb.data(), g2.data(), Ub2.data(), Ubk2.data(), yb2.data(), win.data(), mB, -1, mB + w_mid, mB, 1, &zero};
    hs_emul::launch(dim3(2), dim3(kMxThreads), size_t(kMxLds) * sizeof(double), [&] { mx_wide(bw) ? k_band_factor_mx<true>(T) : k_band_factor_mx<false>(T); },
                    std::vector<unsigned>{1, 0});  // (workgroup 0 waits at the junction for workgroup 1's window)
  } else {
    const Tables Tfull = T;
    if (f0 > 0) {  // the decoupled rows one wave each, the kernel on the trailing sub-matrix (the band storage is row relative)
      hs_emul::launch(dim3(f0), dim3(64), 0, [&] { k_factor_decoupled_rows(Tfull, f0); });
      T.Sb += size_t(6 * f0) * ncb, T.g_s += 6 * f0, T.Ub += size_t(6 * f0) * ncb, T.Ubk += size_t(24) * f0, T.ybuf += 6 * f0, T.np -= 6 * f0;
    }
    T.fj[0] = FactorJob{T.Sb, T.g_s, T.Ub, T.Ubk, T.ybuf, nullptr, T.np / 6, -1};
    const size_t la_lds = (size_t(42) * (ncb + 2) + size_t(np) + 48) * sizeof(double);
    if (la_compute_waves(bw) == 3)
      hs_emul::launch(dim3(1), dim3(la_threads(3)), la_lds, [&] { k_band_factor_la<1, 3>(T); });
    else
      hs_emul::launch(dim3(1), dim3(la_threads(4)), la_lds, [&] { k_band_factor_la<1, 4>(T); });
    T = Tfull;  // (the sweeps run on the whole factor and stop above block row f0)
  }
  // ---- the sweeps: the two-phase one, then the one-phase one, each with builders of its own launch and outputs of its own ----
  const size_t n_sb_all = size_t(sb_count(n_blk) + 1);
  std::vector<double> Vb(n_sb_all * kSbN * kSbN, 0.0), Vb2 = Vb, Mb(n_sb_all * sb_stack_doubles(bw), 7.0), Mb2 = Mb;  // (7: what a builder does not write is never read)
  T.scale_p = const_cast<double*>(scale_p.data()), T.g_full = const_cast<double*>(g_full.data()), T.D2p = const_cast<double*>(D2p.data());
  const int n0 = two_ended ? m + w_mid : n_blk;
  const BackJob j0{Ub.data(), Ubk.data(), yb.data(), Vb.data(), nullptr, n0, 0, 0, Mb.data()};
  const BackJob j1 = two_ended ? BackJob{Ub2.data(), Ubk2.data(), yb2.data(), Vb2.data(), nullptr, mB, w_mid, 1, Mb2.data()} : j0;
  const int n_jobs = two_ended ? 2 : 1;
  const size_t g_lds = size_t(6 * (bw - 1)) * (6 * (bw - 1) | 1) * sizeof(double);
  const size_t lds = std::max((2 * size_t(np) + 32) * sizeof(double) + (two_ended ? g_lds + sb_phase_a_doubles(bw) * sizeof(double) : 0),
                              size_t(3 * kSbN * (kSbN + 1)) * sizeof(double));
  const unsigned n_wg = n_jobs + sb_count(n0) + (two_ended ? sb_count(mB) : 0);
  std::vector<unsigned> order;  // builders, then the near sweep, then the far sweep
  for (unsigned w = n_jobs; w < n_wg; ++w) order.push_back(w);
  for (int j = 0; j < n_jobs; ++j) order.push_back(j);
  std::vector<double> out[2][4];
  for (int pm = 0; pm < 2; ++pm) {
    std::vector<double> xsol(np, 0.0), step_p(np, 0.0), delta_p(np, 0.0);
    st.g_dot_step_pose = st.d2_step2_pose = st.g_dot_step_far = st.d2_step2_far = 0.0;
    T.join_epoch = 2 + pm;
    T.xsol = xsol.data(), T.step_p = step_p.data(), T.delta_p = delta_p.data();
    if (pm)
      hs_emul::launch(dim3(n_wg), dim3(kCholThreads), lds, [&] { k_band_backward_pm(T, j0, j1, m, n_jobs, f0); }, order);
    else
      hs_emul::launch(dim3(n_wg), dim3(kCholThreads), lds, [&] { k_band_backward_sb(T, j0, j1, m, n_jobs, f0); }, order);
    if (!two_ended)
      for (int i = 0; i < np; ++i) xsol[i] = -step_p[i];  // (a one-ended sweep does not write xsol)
    out[pm][0] = xsol, out[pm][1] = step_p, out[pm][2] = delta_p;
    out[pm][3] = {st.g_dot_step_pose, st.d2_step2_pose, st.g_dot_step_far, st.d2_step2_far};
  }
  FILE* o = fopen(argv[2], "wb");
  // (super-blocks the middle rows span less one: the far sweep redoes them — phase A — while that is below kSbPrefetch)
  const int res[4] = {m, mB, st.chol_failed, two_ended ? sb_count(m + w_mid) - 1 - m / kSb : -1};
  fwrite(res, sizeof(int), 4, o);
  write_vec(o, Ub), write_vec(o, Ub2), write_vec(o, Mb), write_vec(o, Mb2);
  for (int pm = 0; pm < 2; ++pm)
    for (int k = 0; k < 4; ++k) write_vec(o, out[pm][k]);
  fclose(o);
  return 0;
}
