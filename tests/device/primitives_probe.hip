// primitives_probe.hip — TEST INFRASTRUCTURE (tests/test_gpu_primitives.py): primitives_probe.hpp for gfx950 behind one C entry point.
// Built by __graft_entry__.build() into tests/device/libhs_probe.so with the product's flags; nothing in the product links it.
#include "primitives_probe.hpp"

/// Runs family `which` on one workgroup of `threads` lanes: allocates, copies `in` up, launches, synchronises, copies `out` back.
/// Returns the HIP status (0 = hipSuccess), or -1 when the sizes do not belong to the family (nothing is launched then).
extern "C" int hs_probe_run(int which, const double* in, int n_in, double* out, int n_out, int threads) {
  if (!hs_probe::sizes_ok(which, n_in, n_out, threads) || (n_in > 0 && !in) || (n_out > 0 && !out)) return -1;
  double *d_in = nullptr, *d_out = nullptr;
  hipError_t e = hipMalloc(&d_in, sizeof(double) * size_t(n_in > 0 ? n_in : 1));
  if (e == hipSuccess) e = hipMalloc(&d_out, sizeof(double) * size_t(n_out > 0 ? n_out : 1));
  if (e == hipSuccess) e = hipMemcpy(d_in, in, sizeof(double) * size_t(n_in), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0xff, sizeof(double) * size_t(n_out));  // (NaN: a value no probe leaves is seen as such)
  if (e == hipSuccess) {
    k_primitives_probe<<<dim3(1), dim3(threads), 0, 0>>>(which, d_in, n_in, d_out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out, d_out, sizeof(double) * size_t(n_out), hipMemcpyDeviceToHost);
  (void)hipFree(d_in), (void)hipFree(d_out);
  return int(e);
}
