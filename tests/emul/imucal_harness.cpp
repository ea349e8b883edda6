// imucal_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_imucal.py): the gathers of the free IMU columns (hyperslam_amd/csrc/
// kernels_imucal.hpp: k_imucal_pi, k_imucal_bb, k_imucal_ii, k_imucal_finish), compiled FROM THE PRODUCT'S KERNEL SOURCE for the host
// (tests/emul/hip/hip_runtime.h) and run on inertial records and sensor Jacobians a Python test fabricates. The whole sequence runs twice
// into separate buffers: the test compares the two bit for bit.
// Usage: imucal_harness <in.bin> <out.bin>
//   in:  int32 [K, kb, n_cp, n_bias, n_ine, ni, n_splits, nc, n_slices], int32 map (ni), i_seg_ptr (n_seg + 1), i_first_bias (n_ine), i_bias_ptr (n_bias + 2),
//        i_rec (n_ine x (18 + 36 K + 2 kb)), sensor Jacobians (n_ine x 216)
//   out: per run: the H_pb partials (n_splits x 6 n_cp x nb, prefilled with 7), H_bb (nb x nb, prefilled with 0), g_b (nb, prefilled with 0)
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

template <int K>
static void run(const Tables& T, const ImuCal& A, int n_splits, int n_slices) {
  const int n_groups = imucal_groups(A.ni), n_jobs = imucal_jobs(A.ni), n_chunks = (T.n_ine + kImuCalChunk - 1) / kImuCalChunk;
  hs_emul::launch(dim3(T.sp.n_cp, n_groups), dim3(kBlock), 0, [&] { k_imucal_pi<K>(T, A, n_splits); });
  hs_emul::launch(dim3(T.n_bias, n_groups, n_slices), dim3(kBlock), 0, [&] { k_imucal_bb<K>(T, A); });
  hs_emul::launch(dim3(n_chunks, n_jobs), dim3(kBlock), 0, [&] { k_imucal_ii<K>(T, A); });
  hs_emul::launch(dim3(((n_jobs + T.n_bias * n_groups) * kImuCalGroup * kImuCalGroup + kBlock - 1) / kBlock), dim3(kBlock), 0, [&] { k_imucal_finish(T, A, n_chunks, n_slices); });
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  const std::vector<int> hdr = read_vec<int>(in, 9);
  const int k = hdr[0], kb = hdr[1], n_cp = hdr[2], n_bias = hdr[3], n_ine = hdr[4], ni = hdr[5], n_splits = hdr[6], nc = hdr[7], n_slices = hdr[8];
  const int n_seg = n_cp - k + 1, np = 6 * n_cp, nb = 6 * n_bias + 2 + ni + nc, irec = 18 + 36 * k + 2 * kb;
  const std::vector<int> map = read_vec<int>(in, ni), seg_ptr = read_vec<int>(in, n_seg + 1), first_bias = read_vec<int>(in, n_ine),
                         bias_ptr = read_vec<int>(in, n_bias + 2);
  std::vector<double> i_rec = read_vec<double>(in, size_t(n_ine) * irec), sj = read_vec<double>(in, size_t(n_ine) * kSensorRecInertial);
  fclose(in);
  DevState st;
  std::memset(&st, 0, sizeof(st));
  Tables T;
  std::memset(&T, 0, sizeof(T));
  T.sp = Spline{k, n_cp, 0.0, 0.1, 10.0, 0, 0};
  T.n_seg = n_seg, T.np = np, T.nb = nb, T.nc = nc, T.kb = kb, T.n_bias = n_bias, T.n_ine = n_ine;
  T.i_rec = i_rec.data(), T.i_seg_ptr = seg_ptr.data(), T.i_first_bias = first_bias.data(), T.i_bias_ptr = bias_ptr.data();
  T.xo_pb = 0, T.xo_bb = np * nb, T.xo_gb = T.xo_bb + nb * nb, T.x_count1 = T.xo_gb + nb;
  T.st = &st;
  const int n_chunks = (n_ine + kImuCalChunk - 1) / kImuCalChunk;
  FILE* out = fopen(argv[2], "wb");
  for (int pass = 0; pass < 2; ++pass) {
    std::vector<double> xbuf(T.x_count1, 0.0), xpart(size_t(n_splits) * T.x_count1, 7.0);
    const size_t n_ii = size_t(n_chunks) * imucal_jobs(ni) * kImuCalGroup * kImuCalGroup;
    std::vector<double> part(n_ii + size_t(n_bias) * imucal_groups(ni) * kImuCalBbSlices * kImuCalGroup * kImuCalGroup, -3.0);
    T.xbuf = xbuf.data(), T.xpart = xpart.data();
    const ImuCal A{sj.data(), map.data(), part.data(), part.data() + n_ii, ni, 6 * n_bias + 2};
    if (k == 4)
      run<4>(T, A, n_splits, n_slices);
    else if (k == 5)
      run<5>(T, A, n_splits, n_slices);
    else
      run<6>(T, A, n_splits, n_slices);
    for (int sp = 0; sp < n_splits; ++sp) fwrite(xpart.data() + size_t(sp) * T.x_count1 + T.xo_pb, 8, size_t(np) * nb, out);
    fwrite(xbuf.data() + T.xo_bb, 8, size_t(nb) * nb, out);
    fwrite(xbuf.data() + T.xo_gb, 8, nb, out);
  }
  fclose(out);
  return 0;
}
