// primitives_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulator_primitives.py): tests/device/primitives_probe.hpp, the kernel that calls
// the product's spelling of every wave primitive, compiled for the host against tests/emul/hip/hip_runtime.h (one std::thread per lane) — the
// same text tests/device/primitives_probe.hip compiles for gfx950. What it writes must equal tests/primitive_models.py bit for bit.
// Usage: primitives_harness <family> <threads> <in.bin> <out.bin>     (raw little-endian doubles; the output size follows from the family)
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "hip/hip_runtime.h"

thread_local dim3 threadIdx;
thread_local unsigned hs_emul::exchange_count = 0;
dim3 blockIdx, blockDim, gridDim;

#include "../device/primitives_probe.hpp"

int main(int argc, char** argv) {
  if (argc < 5) return 1;
  const int which = atoi(argv[1]), threads = atoi(argv[2]);
  FILE* f = fopen(argv[3], "rb");
  if (!f) return 1;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> in(size_t(bytes) / sizeof(double));
  if (!in.empty() && fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
  fclose(f);
  const int n_in = int(in.size());
  const int n_out = which == hs_probe::kRsq ? 2 * n_in : (which >= 0 && which < hs_probe::kFamilies ? hs_probe::kOutPerLane[which] * threads : 0);
  if (!hs_probe::sizes_ok(which, n_in, n_out, threads)) {
    fprintf(stderr, "sizes do not belong to family %d\n", which);
    return 3;
  }
  std::vector<double> out(size_t(n_out), std::numeric_limits<double>::quiet_NaN());
  hs_emul::launch(dim3(1), dim3(threads), 0, [&] { k_primitives_probe(which, in.data(), n_in, out.data()); });
  FILE* o = fopen(argv[4], "wb");
  if (!o) return 1;
  fwrite(out.data(), sizeof(double), out.size(), o);
  fclose(o);
  return 0;
}
