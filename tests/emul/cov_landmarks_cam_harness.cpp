// cov_landmarks_cam_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_cov_landmarks_cam.py): the landmark blocks of the covariance
// with free camera coordinates (hyperslam_amd/csrc/kernels_covariance.hpp: k_cov_landmarks_cam), compiled FROM THE PRODUCT'S KERNEL SOURCE
// for the host (tests/emul/hip/hip_runtime.h: one std::thread per lane) and run on landmark factors and covariance blocks a Python test
// fabricates.
// Usage: cov_landmarks_cam_harness <in.bin> <out.bin>
//   in:  int32 [n_lm, bw, nc, nbi, np, 0, 0, 0], int32 lm_const (n_lm), lm_ptr (n_lm + 1), lm_cfirst (n_lm), lm_ncp (n_lm), lm_yoff (n_lm + 1),
//        Y (lm_yoff[n_lm]), Y_c (n_lm x 3 x nc), lm_L (n_lm x 6), lm_scale (n_lm x 3), Sigma_pp band rows (np x 6bw), Sigma_pb (np x nb),
//        Sigma_bb (nb x nb), nb = nbi + nc
//   out: int32 status (n_lm), Sigma_ll (n_lm x 9)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip/hip_runtime.h"

thread_local dim3 threadIdx;
thread_local unsigned hs_emul::exchange_count = 0;
dim3 blockIdx, blockDim, gridDim;

#include "../../hyperslam_amd/csrc/kernels_common.hpp"
#include "../../hyperslam_amd/csrc/kernels_covariance.hpp"

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

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const std::vector<int> hdr = read_vec<int>(in, 8);
  const int n_lm = hdr[0], bw = hdr[1], nc = hdr[2], nbi = hdr[3], np = hdr[4], nb = nbi + nc, ncb = 6 * bw;
  const std::vector<int> lmc_i = read_vec<int>(in, n_lm), lm_ptr = read_vec<int>(in, n_lm + 1), lm_cfirst = read_vec<int>(in, n_lm);
  const std::vector<int> lm_ncp = read_vec<int>(in, n_lm), lm_yoff = read_vec<int>(in, n_lm + 1);
  std::vector<double> Y = read_vec<double>(in, lm_yoff[n_lm]), Yc = read_vec<double>(in, size_t(3) * n_lm * nc);
  std::vector<double> lm_L = read_vec<double>(in, size_t(6) * n_lm), lm_scale = read_vec<double>(in, size_t(3) * n_lm);
  const std::vector<double> cov = read_vec<double>(in, size_t(np) * ncb), cov_pb = read_vec<double>(in, size_t(np) * nb);
  const std::vector<double> cov_bb = read_vec<double>(in, size_t(nb) * nb);
  fclose(in);
  for (int l = 0; l < n_lm; ++l)  // (what the host guarantees the kernel: a landmark's control points lie inside the window and the band)
    if (lm_ncp[l] > bw || 6 * (lm_cfirst[l] + lm_ncp[l]) > np) {
      fprintf(stderr, "landmark %d outside the band\n", l);
      return 3;
    }
  std::vector<uint8_t> lmc(lmc_i.begin(), lmc_i.end());
  Tables T;
  std::memset(&T, 0, sizeof(T));
  T.n_lm = n_lm, T.bw = bw, T.np = np, T.nb = nb, T.nc = nc;
  T.lm_const = lmc.data(), T.lm_ptr = lm_ptr.data(), T.lm_cfirst = lm_cfirst.data(), T.lm_ncp = lm_ncp.data(), T.lm_yoff = lm_yoff.data();
  T.Y = Y.data(), T.calib_Yc = Yc.data(), T.lm_L = lm_L.data(), T.lm_scale = lm_scale.data();
  std::vector<double> out(size_t(9) * n_lm, 7.0);
  std::vector<int> status(n_lm, -1);
  const int waves = kBlock / 64;
  hs_emul::launch(dim3((n_lm + waves - 1) / waves), dim3(kBlock), cov_landmarks_cam_lds_doubles(bw, nc) * sizeof(double),
                  [&] { k_cov_landmarks_cam(T, cov.data(), cov_pb.data(), cov_bb.data(), out.data(), status.data()); });
  FILE* o = fopen(argv[2], "wb");
  fwrite(status.data(), sizeof(int), status.size(), o);
  fwrite(out.data(), sizeof(double), out.size(), o);
  fclose(o);
  return 0;
}
