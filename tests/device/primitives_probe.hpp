// primitives_probe.hpp — TEST INFRASTRUCTURE: one kernel that calls the product's own spelling of every wave primitive its kernels rest on
// (hyperslam_amd/csrc/kernels_common.hpp, dpp_f64.hpp, kernels_backward_sb.hpp's pair_sum, and the builtins the kernels call directly) and
// writes every lane's result out. It is compiled twice from this one text: for gfx950 (primitives_probe.hip -> libhs_probe.so, run by
// tests/test_gpu_primitives.py) and for the host against tests/emul/hip/hip_runtime.h (tests/emul/primitives_harness.cpp, run by
// tests/test_emulator_primitives.py). Both must equal tests/primitive_models.py bit for bit: that is what ties the emulator, on which every
// `-m "not gpu"` test of a kernel rests, to the hardware.
//
// One workgroup. Inputs and outputs are arrays of doubles, lane-minor: value e of lane t is at [e * blockDim.x + t]. `which` selects the
// family (wave-uniform: every wave primitive below sits in uniform control flow, as in the kernels).
#pragma once
#include "../../hyperslam_amd/csrc/kernels_common.hpp"
#include "../../hyperslam_amd/csrc/dpp_f64.hpp"
#include "../../hyperslam_amd/csrc/kernels_backward_sb.hpp"

namespace hs {
HSD void begin_iteration(const Tables&, double, double, bool) {}  // (declared by the factorisation kernels kernels_backward_sb.hpp brings along; defined by kernels_update.hpp in the product: never reached here)
}  // namespace hs

namespace hs_probe {

enum Family { kDpp = 0, kSums = 1, kShfl = 2, kReadlane = 3, kBallot = 4, kBcast = 5, kArith = 6, kMfma = 7, kRsq = 8, kFamilies = 9 };
// values per lane a family reads / writes (kRsq: n values in, 2 n out, whatever the lane count)
constexpr int kInPerLane[kFamilies] = {1, 5, 2, 1, 1, 3, 3, 8, 0};
constexpr int kOutPerLane[kFamilies] = {9, 7, 18, 64, 4, 48, 6, 8, 0};
constexpr int kMaxThreads = 256;

/// Sizes the entry points check before anything is launched: a probe never reads or writes outside what it was handed.
inline bool sizes_ok(int which, int n_in, int n_out, int threads) {
  if (which < 0 || which >= kFamilies || threads < 1 || threads > kMaxThreads || n_in < 0 || n_out < 0) return false;
  if (which == kRsq) return n_in <= (1 << 20) && n_out == 2 * n_in;
  if (which == kMfma && threads != 64) return false;
  return n_in == kInPerLane[which] * threads && n_out == kOutPerLane[which] * threads;
}

/// The multiply-adds with a DPP operand carry no wait states of their own (dpp_f64.hpp: the caller keeps two instructions between the write
/// of the broadcast operand and its use); here every use gets them from a statement of its own.
HSD void settle() {
#if !defined(HS_EMULATED_DEVICE)
  asm volatile("s_nop 4");
#endif
}

template <int R>
HSD void bcast_one(double u, double m, double acc, double* out, int nt, int t) {
  settle();
  out[(3 * R) * nt + t] = hs::dx_row_bcast<R>(u);
  double a = acc, b = acc;
  hs::dx_pin(a), hs::dx_pin(b);
  settle();
  hs::dx_fmac_bcast<R>(a, u, m);
  settle();
  hs::dx_fnma_bcast<R>(b, u, m);
  settle();
  out[(3 * R + 1) * nt + t] = a, out[(3 * R + 2) * nt + t] = b;
  if constexpr (R + 1 < 16) bcast_one<R + 1>(u, m, acc, out, nt, t);
}

}  // namespace hs_probe

#if defined(HS_EMULATED_DEVICE)
typedef hs_emul_f64x4 hs_probe_f64x4;
#else
typedef double hs_probe_f64x4 __attribute__((ext_vector_type(4)));
#endif

__global__ void __launch_bounds__(256) k_primitives_probe(int which, const double* __restrict__ in, int n, double* __restrict__ out) {
  using namespace hs;
  using namespace hs_probe;
  const int t = threadIdx.x, nt = blockDim.x;
  __shared__ double lds[5 * (kMaxThreads / 64)];
  if (which == kDpp) {
    const double v = in[t];
    out[0 * nt + t] = dpp_move<0xB1>(v);
    out[1 * nt + t] = dpp_move<0x4E>(v);
    out[2 * nt + t] = dpp_move<0x104>(v);
    out[3 * nt + t] = dpp_move<0x114>(v);
    out[4 * nt + t] = dpp_move<0x128>(v);
    out[5 * nt + t] = lane_xor1(v);
    out[6 * nt + t] = lane_xor2(v);
    out[7 * nt + t] = lane_xor4(v);
    out[8 * nt + t] = pair_sum(v);  // (kernels_backward_sb.hpp's own spelling of the 0xB1 move: v + the partner's v)
  } else if (which == kSums) {
    double v[5];
    for (int e = 0; e < 5; ++e) v[e] = in[e * nt + t];
    out[0 * nt + t] = wave_sum(v[0]);
    out[1 * nt + t] = block_sum(v[0], lds);  // (valid on thread 0)
    block_sum_n<5>(v, lds);
    for (int e = 0; e < 5; ++e) out[(2 + e) * nt + t] = v[e];  // (valid on thread 0)
  } else if (which == kShfl) {
    const double v = in[t];
    const int iv = int(in[nt + t]);
#pragma unroll
    for (int b = 0; b < 6; ++b) {
      out[b * nt + t] = __shfl_xor(v, 1 << b);
      out[(6 + b) * nt + t] = double(__shfl_xor(iv, 1 << b));
      out[(12 + b) * nt + t] = double(__shfl_up(iv, 1 << b));  // (the deltas of kernels_build.hpp's scan: 1, 2, .. 32)
    }
  } else if (which == kReadlane) {
    const double v = in[t];
#pragma unroll
    for (int s = 0; s < 64; ++s)  // (the hi / lo pair form of the panels: kernels_factor.hpp, kernels_factor_mx.hpp, kernels_border.hpp)
      out[s * nt + t] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), s), __builtin_amdgcn_readlane(__double2loint(v), s));
  } else if (which == kBallot) {
    const int lane = t & 63;
    const unsigned long long m = __ballot(in[t] > 0.0);
    out[0 * nt + t] = double(unsigned(m & 0xffffffffull));
    out[1 * nt + t] = double(unsigned(m >> 32));
    out[2 * nt + t] = double(__popcll(m));
    out[3 * nt + t] = double(__popcll(m & ((1ull << lane) - 1ull)));  // (the rank inside the wave: kernels_build.hpp, kernels_klt.hpp)
  } else if (which == kBcast) {
    bcast_one<0>(in[t], in[nt + t], in[2 * nt + t], out, nt, t);
  } else if (which == kArith) {
    const double a = in[t], b = in[nt + t], c = in[2 * nt + t];
    out[0 * nt + t] = dx_mul(a, b);
    out[1 * nt + t] = dx_fma(a, b, c);
    out[2 * nt + t] = dx_one_minus(a, b);
    out[3 * nt + t] = dx_half_plus(a, b);
    double p = a, q = b;
    dx_pin(p), dx_pin(q);
    dx_scale2(p, q, c);
    out[4 * nt + t] = p, out[5 * nt + t] = q;
  } else if (which == kMfma) {
    const double a = in[t], b = in[nt + t], a2 = in[6 * nt + t], b2 = in[7 * nt + t];
    hs_probe_f64x4 c = {in[2 * nt + t], in[3 * nt + t], in[4 * nt + t], in[5 * nt + t]};
    hs_probe_f64x4 one = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    hs_probe_f64x4 two = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b2, one, 0, 0, 0);  // (chained through the accumulator: kernels_factor_mx.hpp)
    for (int r = 0; r < 4; ++r) out[r * nt + t] = one[r], out[(4 + r) * nt + t] = two[r];
  } else if (which == kRsq) {
    for (int i = t; i < n; i += nt) {
      const double d = in[i];
      out[i] = __builtin_amdgcn_rsq(d);
      out[n + i] = dx_rsq(d);
    }
  }
}
