// cov_sample_sensor_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_cov_sample_sensor.py): the covariance of a sensor pose
// (hyperslam_amd/csrc/kernels_covariance.hpp: k_cov_sample_sensor, and k_cov_sample next to it), compiled FROM THE PRODUCT'S KERNEL SOURCE
// for the host (tests/emul/hip/hip_runtime.h: one std::thread per lane) and run on a spline and covariance blocks a Python test fabricates.
// Usage: cov_sample_sensor_harness <in.bin> <out.bin>
//   in:  int32 [K, n_cp, bw, nb, ecol, n, 0, 0], double [t0, dt], cp (n_cp x 8), T_bs (7), Sigma_pp band rows (6 n_cp x 6 bw),
//        Sigma_pb (6 n_cp x nb), Sigma_bb (nb x nb), stamps (n)
//   out: double: the output buffer of a first run of k_cov_sample_sensor with kGuard sentinels (kSentinel) in front and behind
//        (kGuard + 36 n + kGuard), the same of a second run, then the 36 n values of k_cov_sample
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "hip/hip_runtime.h"

thread_local dim3 threadIdx;
thread_local unsigned hs_emul::exchange_count = 0;
dim3 blockIdx, blockDim, gridDim;

#include "../../hyperslam_amd/csrc/host_structure.hpp"
#include "../../hyperslam_amd/csrc/kernels_common.hpp"
#include "../../hyperslam_amd/csrc/kernels_covariance.hpp"

using namespace hs;

constexpr int kGuard = 64;
constexpr double kSentinel = -7.25;

template <class T>
static std::vector<T> read_vec(FILE* f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) {
    fprintf(stderr, "short read\n");
    exit(2);
  }
  return v;
}

template <int K>
static void run(const Tables& T, const double* cov, const double* pb, const double* bb, int nb, const double* T_bs, int ecol, int n, const double* stamps,
                double* out_sensor, double* out_body) {
  const int waves = kBlock / 64, grid = (n + waves - 1) / waves;
  if (out_sensor) hs_emul::launch(dim3(grid), dim3(kBlock), 0, [&] { k_cov_sample_sensor<K>(T, cov, pb, bb, nb, T_bs, ecol, n, stamps, out_sensor); });
  if (out_body) hs_emul::launch(dim3(grid), dim3(kBlock), 0, [&] { k_cov_sample<K>(T, cov, n, stamps, out_body); });
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const std::vector<int> hdr = read_vec<int>(in, 8);
  const int K = hdr[0], n_cp = hdr[1], bw = hdr[2], nb = hdr[3], ecol = hdr[4], n = hdr[5], np = 6 * n_cp, ncb = 6 * bw;
  const std::vector<double> knots = read_vec<double>(in, 2);
  std::vector<double> cp = read_vec<double>(in, size_t(8) * n_cp);
  const std::vector<double> T_bs = read_vec<double>(in, 7), cov = read_vec<double>(in, size_t(np) * ncb), pb = read_vec<double>(in, size_t(np) * nb);
  const std::vector<double> bb = read_vec<double>(in, size_t(nb) * nb), stamps = read_vec<double>(in, n);
  fclose(in);
  // what the host guarantees the kernel: the K control points of every stamp inside the window and the band, the T_bs columns inside the border
  if (K < 4 || K > 6 || bw < K || n_cp < K || (ecol >= 0 && ecol + 6 > nb)) {
    fprintf(stderr, "bad shape\n");
    return 3;
  }
  for (int i = 0; i < n; ++i) {
    const int f = h_segment_first(stamps[i], knots[0], knots[1], K);
    if (f < 0 || f > n_cp - K) {
      fprintf(stderr, "stamp %d outside the spline\n", i);
      return 3;
    }
  }
  Tables T;
  std::memset(&T, 0, sizeof(T));
  T.sp = Spline{K, n_cp, knots[0], knots[1], 1.0 / knots[1], 0, 0};
  T.basis = make_basis_coef(K);
  T.cp = cp.data(), T.bw = bw, T.np = np, T.nb = nb;
  const size_t len = size_t(kGuard) + size_t(36) * n + kGuard;
  std::vector<double> a(len, kSentinel), b(len, kSentinel), body(size_t(36) * n, kSentinel);
  for (int pass = 0; pass < 2; ++pass) {
    double* o = (pass ? b : a).data() + kGuard;
    double* ob = pass ? nullptr : body.data();
    if (K == 4) run<4>(T, cov.data(), pb.data(), bb.data(), nb, T_bs.data(), ecol, n, stamps.data(), o, ob);
    if (K == 5) run<5>(T, cov.data(), pb.data(), bb.data(), nb, T_bs.data(), ecol, n, stamps.data(), o, ob);
    if (K == 6) run<6>(T, cov.data(), pb.data(), bb.data(), nb, T_bs.data(), ecol, n, stamps.data(), o, ob);
  }
  FILE* out = fopen(argv[2], "wb");
  fwrite(a.data(), sizeof(double), a.size(), out);
  fwrite(b.data(), sizeof(double), b.size(), out);
  fwrite(body.data(), sizeof(double), body.size(), out);
  fclose(out);
  return 0;
}
