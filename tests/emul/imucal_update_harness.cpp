// imucal_update_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_imucal_update.py): the solve-side kernels of a handle that estimates
// IMU blocks (hyperslam_amd/csrc/kernels_imucal.hpp: k_imucal_candidate, k_imucal_commit), compiled FROM THE PRODUCT'S KERNEL SOURCE for the
// host (tests/emul/hip/hip_runtime.h) and run on parameters and a border step a Python test fabricates.
// Usage: imucal_update_harness <in.bin> <out.bin>
//   in:  int32 [ni, col0, nc, norm_slot], int32 map (ni), IMU parameters (37), border step delta_b (col0 + ni + nc)
//   out: candidate buffer (37 + 8 doubles, prefilled with -7), norm_part (2 norm_slot + 6, prefilled with -7), the parameters and delta_b as
//        the candidate kernel left them (37, nb), the parameters behind a commit of an accepted and of a rejected step (37, 37; the rejected
//        one into a table prefilled with the parameters), and the candidate buffer / norm_part of a launch on a finished solve (st.done)
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
#include "../../hyperslam_amd/csrc/kernels_imucal.hpp"

namespace hs {
HSD void begin_iteration(const Tables&, double, double, bool) {}  // (the bookkeeping of k_pack_exchange: never launched here)
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

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const std::vector<int> hdr = read_vec<int>(in, 4);
  const int ni = hdr[0], col0 = hdr[1], nc = hdr[2], norm_slot = hdr[3], nb = col0 + ni + nc;
  const std::vector<int> map = read_vec<int>(in, ni);
  std::vector<double> imu = read_vec<double>(in, kImuParamDoubles), delta_b = read_vec<double>(in, nb);
  fclose(in);
  static_assert(sizeof(ImuParams) == kImuParamDoubles * sizeof(double), "ImuParams is a plain array of doubles");
  DevState st;
  std::memset(&st, 0, sizeof(st));
  Tables T;
  std::memset(&T, 0, sizeof(T));
  T.nb = nb, T.nc = nc, T.n_bias = (col0 - 2) / 6, T.delta_b = delta_b.data(), T.imu = reinterpret_cast<const ImuParams*>(imu.data());
  T.n_norm_part = norm_slot, T.st = &st;
  const ImuCal A{nullptr, map.data(), nullptr, nullptr, ni, col0};
  const size_t n_norm = 2 * size_t(norm_slot) + 6;
  std::vector<double> cand(kImuParamDoubles + 8, -7.0), norm(n_norm, -7.0), acc(kImuParamDoubles, -7.0), rej = imu;
  T.norm_part = norm.data();
  hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_imucal_candidate(T, A, reinterpret_cast<ImuParams*>(cand.data()), norm_slot); });
  st.accepted = 1;
  hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_imucal_commit(T, reinterpret_cast<ImuParams*>(acc.data()), reinterpret_cast<const ImuParams*>(cand.data())); });
  st.accepted = 0;
  hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_imucal_commit(T, reinterpret_cast<ImuParams*>(rej.data()), reinterpret_cast<const ImuParams*>(cand.data())); });
  std::vector<double> cand_done(kImuParamDoubles + 8, -7.0), norm_done(n_norm, -7.0);
  st.done = 1;
  T.norm_part = norm_done.data();
  hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_imucal_candidate(T, A, reinterpret_cast<ImuParams*>(cand_done.data()), norm_slot); });
  FILE* out = fopen(argv[2], "wb");
  for (const std::vector<double>* v : {&cand, &norm, &imu, &delta_b, &acc, &rej, &cand_done, &norm_done}) fwrite(v->data(), 8, v->size(), out);
  fclose(out);
  return 0;
}
