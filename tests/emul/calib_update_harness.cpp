// calib_update_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_calib_update.py): the update kernels of a window with free camera
// coordinates (Tables::nc > 0), compiled FROM THE PRODUCT'S KERNEL SOURCES for the host (tests/emul/hip/hip_runtime.h) and run on landmark
// factors a Python test fabricates:
//   k_backsub_retract<true>     per landmark:  y_l = L^-T (yh - Yh' (Sp o y_p) - Y_c y_c), candidate landmarks, decision terms
//   k_update_visual<K, true>    the same per chunk (chunks without residual blocks: the candidate cost is not what is checked here)
//   k_calib_candidate           candidate camera table, the camera blocks' norms, (g_c - g_c,reduced) . dc
//   k_calib_commit              cam <- candidate on an accepted step
// Usage: calib_update_harness <in.bin> <out.bin>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hip/hip_runtime.h"

thread_local dim3 threadIdx;
thread_local unsigned hs_emul::exchange_count = 0;
dim3 blockIdx, blockDim, gridDim;

#include "../../hyperslam_amd/csrc/host_structure.hpp"
#include "../../hyperslam_amd/csrc/kernels_common.hpp"
#include "../../hyperslam_amd/csrc/kernels_linearize.hpp"
#include "../../hyperslam_amd/csrc/kernels_sensor.hpp"
#include "../../hyperslam_amd/csrc/kernels_schur.hpp"
#include "../../hyperslam_amd/csrc/kernels_build.hpp"
#include "../../hyperslam_amd/csrc/kernels_update.hpp"
#include "../../hyperslam_amd/csrc/kernels_calib.hpp"

namespace hs {
HSD void finalize_border_body(const Tables&, int, int, int) {}  // (k_finalize_reduced's border workgroups: never launched here)
}  // namespace hs

using namespace hs;

struct Reader {
  FILE* f;
  template <class T>
  std::vector<T> vec(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
      fprintf(stderr, "short read\n");
      exit(2);
    }
    return v;
  }
};

template <int K>
static void run_fused(const Tables& B, int nb_vis, int Lmax) {
  const int R = 64;
  hs_emul::launch(dim3(nb_vis + B.n_norm_part), dim3(kBlock), size_t(update_lds_doubles(B.bw, R, Lmax)) * 8, [&] { k_update_visual<K, true>(B, R, Lmax, nb_vis); });
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  Reader rd{fopen(argv[1], "rb")};
  if (!rd.f) return 1;
  const std::vector<int> hdr = rd.vec<int>(8);
  const int k = hdr[0], n_cp = hdr[1], n_lm = hdr[2], bw = hdr[3], nc = hdr[4], nbi = hdr[5], n_chunk = hdr[6], n_cam = hdr[7];
  const int np = 6 * n_cp, nb = nbi + nc;
  std::vector<double> cp = rd.vec<double>(size_t(8) * n_cp), cam = rd.vec<double>(size_t(16) * n_cam), lm = rd.vec<double>(size_t(3) * n_lm);
  const std::vector<int> lmc_i = rd.vec<int>(n_lm), lm_ptr = rd.vec<int>(n_lm + 1), lm_cfirst = rd.vec<int>(n_lm), lm_ncp = rd.vec<int>(n_lm), lm_yoff = rd.vec<int>(n_lm + 1);
  std::vector<double> Y = rd.vec<double>(size_t(lm_yoff[n_lm]) + 1), lm_L = rd.vec<double>(size_t(6) * n_lm), lm_yhat = rd.vec<double>(size_t(3) * n_lm);
  std::vector<double> lm_scale = rd.vec<double>(size_t(3) * n_lm), lm_sb = rd.vec<double>(size_t(3) * n_lm), lm_D2 = rd.vec<double>(size_t(3) * n_lm);
  std::vector<double> step_p = rd.vec<double>(np), scale_p = rd.vec<double>(np), D2p = rd.vec<double>(np), delta_b = rd.vec<double>(nb), D2b = rd.vec<double>(nb);
  std::vector<double> Yc = rd.vec<double>(size_t(3) * n_lm * nc), g_full = rd.vec<double>(nc), g_red = rd.vec<double>(nc);
  const std::vector<int> calib_map = rd.vec<int>(nc);
  std::vector<int> ch_desc = rd.vec<int>(size_t(8) * n_chunk);
  fclose(rd.f);
  std::vector<uint8_t> lmc(n_lm);
  for (int i = 0; i < n_lm; ++i) lmc[i] = uint8_t(lmc_i[i]);
  std::vector<double> delta_p(np);
  for (int i = 0; i < np; ++i) delta_p[i] = scale_p[i] * step_p[i];
  int Lmax = 1, n_obs = n_lm;
  for (int w = 0; w < n_chunk; ++w) Lmax = std::max(Lmax, ch_desc[8 * w + 1]);
  while (n_obs > 0 && lm_ptr[n_obs] == lm_ptr[n_obs - 1]) --n_obs;
  // exchange buffer: [g_b nb | diag(J'J)_c nc | full camera gradient nc | decision 5]
  std::vector<double> xbuf(size_t(nb) + 2 * nc + 8, 0.0);
  for (int c = 0; c < nc; ++c) xbuf[nbi + c] = g_red[c], xbuf[nb + nc + c] = g_full[c];
  DevState st;
  std::memset(&st, 0, sizeof(st));
  st.radius = 1e4, st.decrease_factor = 2.0, st.max_iterations = 4, st.scaling_ready = 1, st.iteration = 1;

  Tables T;
  std::memset(&T, 0, sizeof(T));
  T.sp = Spline{k, n_cp, 0.0, 0.1, 10.0, 0, 0};
  T.basis = make_basis_coef(k);
  T.cp = cp.data(), T.cam = cam.data(), T.n_cam = n_cam;
  T.n_lm = n_lm, T.lm = lm.data(), T.lm_const = lmc.data(), T.lm_ptr = lm_ptr.data(), T.lm_cfirst = lm_cfirst.data(), T.lm_ncp = lm_ncp.data(), T.lm_yoff = lm_yoff.data();
  T.lm_scale = lm_scale.data(), T.lm_L = lm_L.data(), T.lm_yhat = lm_yhat.data(), T.lm_sb = lm_sb.data(), T.lm_D2 = lm_D2.data(), T.Y = Y.data(), T.n_obs_lm = n_obs;
  T.bw = bw, T.np = np, T.scale_p = scale_p.data(), T.D2p = D2p.data(), T.step_p = step_p.data(), T.delta_p = delta_p.data();
  T.nb = nb, T.nc = nc, T.calib_map = calib_map.data(), T.calib_Yc = Yc.data(), T.delta_b = delta_b.data(), T.D2b = D2b.data();
  T.xbuf = xbuf.data(), T.xo_gb = 0, T.xo_cdj = nb, T.x_count1 = nb + 2 * nc, T.xo_dec = nb + 2 * nc;
  T.fused = 1, T.n_chunk = n_chunk, T.ch_desc = ch_desc.data();
  T.n_norm_part = std::max((n_cp + kBlock - 1) / kBlock, 1);
  T.rank = 0, T.world = 1, T.st = &st;

  // records path
  const int n_lm_part_a = (n_lm + 3) / 4;
  std::vector<double> lm_cand_a(size_t(3) * n_lm, -7.0), cp_cand_a(size_t(8) * n_cp), norm_a(2 * size_t(T.n_norm_part) + 2, 0.0), lm_part_a(4 * size_t(n_lm_part_a) + 4);
  Tables A = T;
  A.lm_cand = lm_cand_a.data(), A.cp_cand = cp_cand_a.data(), A.norm_part = norm_a.data(), A.lm_part = lm_part_a.data(), A.n_lm_part = n_lm_part_a;
  hs_emul::launch(dim3(A.n_lm_part + A.n_norm_part), dim3(kBlock), 0, [&] { k_backsub_retract<true>(A); });
  // fused path
  const int nb_vis = n_chunk;
  std::vector<double> lm_cand_b(size_t(3) * n_lm, -7.0), cp_cand_b(size_t(8) * n_cp), norm_b(2 * size_t(T.n_norm_part) + 2, 0.0), lm_part_b(4 * size_t(nb_vis) + 4), cand_b(nb_vis + 1);
  Tables B = T;
  B.lm_cand = lm_cand_b.data(), B.cp_cand = cp_cand_b.data(), B.norm_part = norm_b.data(), B.lm_part = lm_part_b.data(), B.n_lm_part = nb_vis, B.cand_part = cand_b.data();
  if (k == 4)
    run_fused<4>(B, nb_vis, Lmax);
  else if (k == 5)
    run_fused<5>(B, nb_vis, Lmax);
  else
    run_fused<6>(B, nb_vis, Lmax);
  // candidate cameras, their norms, the gradient correction; commit of an accepted / a rejected step
  std::vector<double> cam_cand(size_t(16) * n_cam, -7.0), cam_acc = cam, cam_rej = cam;
  Tables C = A;
  hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_calib_candidate(C, cam_cand.data(), C.n_norm_part); });
  st.accepted = 1;
  hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_calib_commit(C, cam_acc.data(), cam_cand.data()); });
  st.accepted = 0;
  hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_calib_commit(C, cam_rej.data(), cam_cand.data()); });

  FILE* out = fopen(argv[2], "wb");
  auto put = [&](const std::vector<double>& v, size_t n) { fwrite(v.data(), 8, n, out); };
  put(lm_cand_a, size_t(3) * n_lm), put(lm_cand_b, size_t(3) * n_lm);
  double sums[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < n_lm_part_a; ++i)
    for (int e = 0; e < 4; ++e) sums[e] += lm_part_a[4 * i + e];
  for (int i = 0; i < nb_vis; ++i)
    for (int e = 0; e < 4; ++e) sums[4 + e] += lm_part_b[4 * i + e];
  fwrite(sums, 8, 8, out);
  put(cam_cand, cam_cand.size()), put(cam_acc, cam_acc.size()), put(cam_rej, cam_rej.size());
  const double tail[3] = {norm_a[2 * T.n_norm_part], norm_a[2 * T.n_norm_part + 1], st.g_dot_step_far};
  fwrite(tail, 8, 3, out);
  fclose(out);
  return 0;
}
