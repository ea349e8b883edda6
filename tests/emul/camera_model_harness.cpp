// camera_model_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_camera_model.py): the three places of the product that project or
// un-project a pixel, compiled FROM THE PRODUCT'S SOURCES for the host (tests/emul/hip/hip_runtime.h) and run point by point:
//   visual_measure            (hyperslam_amd/csrc/factors.hpp)         residual rows and d r / d p_s
//   visual_sensor_jacobians   (hyperslam_amd/csrc/kernels_sensor.hpp)  the intrinsics and distortion blocks
//   pixel_to_bearing          (hyperslam_amd/csrc/kernels_aux.hpp)     the inverse of hs_process_tracks
// with unit intrinsics [0, 0, 1, 1] and a zero measurement, so that the residual is the distorted plane point itself. The sensor Jacobians
// run on a one-residual window whose control points and extrinsics are the identity pose and whose landmark is (x, y, 1): p_s = (x, y, 1).
// Input (text): n, then n lines "model x y k1 k2 k3 k4"; m, then m lines "model u v k1 k2 k3 k4".
// Output (text, %.17g): per point r(2) Jps(6) J_intrinsics(8) J_distortion(8); per pixel the bearing(3).
// Usage: camera_model_harness <in.txt> <out.txt>
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
#include "../../hyperslam_amd/csrc/kernels_sensor.hpp"
#include "../../hyperslam_amd/csrc/kernels_aux.hpp"

using namespace hs;

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "r");
  FILE* out = fopen(argv[2], "w");
  if (!in || !out) return 1;
  constexpr int K = 4;
  std::vector<double> cp(size_t(8) * K, 0.0);
  for (int j = 0; j < K; ++j) cp[8 * j + 3] = 1.0, cp[8 * j + 7] = 0.1 * (j - 1);
  double cam[16], lm[3], stamp = 0.05, meas[3] = {0.0, 0.0, 0.0};
  int info = 0, first = 0, lm_id = 0;
  Tables T;
  std::memset(&T, 0, sizeof(T));
  T.sp = Spline{K, K, -0.1, 0.1, 10.0, 0, 0};
  T.basis = make_basis_coef(K);
  T.cp = cp.data(), T.cam = cam, T.n_cam = 1, T.lm = lm, T.n_lm = 1;
  T.n_vis = 1, T.v_stamp = &stamp, T.v_meas = meas, T.v_lm = &lm_id, T.v_info = &info, T.v_first = &first;
  auto camera = [&](int model, const double* k) {
    const double c[16] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 1, k[0], k[1], k[2], k[3], double(model)};
    std::memcpy(cam, c, sizeof(c));
  };
  int n = 0, m = 0;
  if (fscanf(in, "%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int model;
    double x, y, k[4];
    if (fscanf(in, "%d %lf %lf %lf %lf %lf %lf", &model, &x, &y, &k[0], &k[1], &k[2], &k[3]) != 7) return 2;
    camera(model, k);
    double r[2], Jps[6], rec[kSensorRecVisual];
    visual_measure(0, V3{x, y, 1.0}, cam, meas, true, r, Jps);
    lm[0] = x, lm[1] = y, lm[2] = 1.0;
    visual_sensor_jacobians<K>(T, T.cp, 0, false, rec);
    fprintf(out, "%.17g %.17g", r[0], r[1]);
    for (int c = 0; c < 6; ++c) fprintf(out, " %.17g", Jps[c]);
    for (int c = 12; c < kSensorRecVisual; ++c) fprintf(out, " %.17g", rec[c]);
    fprintf(out, "\n");
  }
  if (fscanf(in, "%d", &m) != 1) return 2;
  for (int i = 0; i < m; ++i) {
    int model;
    double u, v, k[4];
    if (fscanf(in, "%d %lf %lf %lf %lf %lf %lf", &model, &u, &v, &k[0], &k[1], &k[2], &k[3]) != 7) return 2;
    camera(model, k);
    const V3 b = pixel_to_bearing(cam, u, v);
    fprintf(out, "%.17g %.17g %.17g\n", b.x, b.y, b.z);
  }
  fclose(in), fclose(out);
  return 0;
}
