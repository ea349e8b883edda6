// kernels_common.hpp — shared device helpers: wave / workgroup reductions, batched strided loads, control-point staging (part of kernels.hpp; included once by capi.hip through it).
#pragma once
#include <type_traits>
#include "factors.hpp"
#include "device_primitives.hpp"
#include "switches.hpp"

namespace hs {

constexpr int kBlock = 256;

/// Phase-timestamp hooks (wall_clock64 writes behind the stamp_* switches of switches.hpp, read by tools/*_phase_timing.py) exist only in
/// profiling builds: with the default HS_PROFILE_HOOKS = 0 every `prof` predicate below is a compile-time false and the product
/// kernels carry no timing code.
#ifndef HS_PROFILE_HOOKS
#define HS_PROFILE_HOOKS 0
#endif
constexpr int kDenseLd = 256;  // leading dimension of the dense copy of a small reduced system (Tables::dense, kernels_dense_mx.hpp)
template <unsigned long long Mask>
HSD bool prof_enabled(int debug_flags, Switch<Mask> s) { return HS_PROFILE_HOOKS && (debug_flags & s.low()); }

constexpr int kGatherFlag = 4 + 2 * 512 + 512 + 4 * kProgressStride;  // word of T.join_flag behind every other use (kBfFlagBase + 512 + 4 kProgressStride)

/// A bounded wait gave up: the solve ends here (every later kernel exits on `done`, hs_solve reports the reason) — nothing downstream may
/// consume what the workgroup that did not arrive has left half written. chol_failed = 2 is never cleared within a solve.
HSD void give_up(DevState* st) {
  st->chol_failed = 2;
  st->termination = HS_FAILURE;
  st->done = 1;
}

/// The verdict of the factorisation kernels (DevState::chol_failed = 1): raised iff a pivot is not a positive FINITE number. `d > 0` alone
/// lets +inf through (1 / sqrt of it is 0, the entries behind it NaN), and a NaN pivot is caught by it only where every pivot is tested
/// on its own: the kernels that keep the test off their chain take the minimum of a block's pivots, and fmin drops a NaN operand.
HSD bool pivot_ok(double d) { return d > 0.0 && d < __builtin_huge_val(); }
/// The same verdict for the six pivots of a diagonal block from what the panel has in registers anyway, with nothing on its chain waiting:
/// dmin, their fmin, catches a pivot <= 0 wherever it stands (a NaN beside it is the operand fmin drops). inv[a] = 1 / sqrt(d_a) by the rsq
/// estimate + one correction step is NaN when d_a is NaN or +inf (rsq = 0, the correction multiplies it with inf), and a NaN inv[a] makes
/// row a of the block NaN (entry * inv[a], whatever the entry), hence the next pivot, and so on down to inv[5]: one comparison of the last
/// inverse sees a non-finite pivot anywhere in the block, the last block row of the system included, where no later pivot would.
HSD bool block_pivots_ok(double dmin, const double (&inv)[6]) { return dmin > 0.0 && inv[5] < __builtin_huge_val(); }


/// The value of lane ^ 1 / ^ 2 / ^ 4 through the DPP cross bar (vector moves; a general __shfl_xor is an LDS permute: ~80 cycles of issue per
/// 32-bit half where these are 4). xor 4 = row_shl:4 for the lanes with bit 2 clear, row_shr:4 for the others.
/// A lane whose source lies outside its row (the shifts) gets 0, through bound_ctrl: with the zero as the instruction's `old` operand every
/// move was preceded by a v_mov that wrote it — half of the instructions of an exchange.
template <int CTRL>
HSD double dpp_move(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
  return __hiloint2double(hi, lo);
}
HSD double lane_xor1(double v) { return dpp_move<0xB1>(v); }  // quad_perm [1 0 3 2]
HSD double lane_xor2(double v) { return dpp_move<0x4E>(v); }  // quad_perm [2 3 0 1]
HSD double lane_xor4(double v) {
#if !defined(HS_EMULATED_DEVICE)
  // row_shl:4 into every lane, then row_shr:4 on top of it into the banks of four lanes with bit 2 set (bank_mask 0b1010): no select behind them
  const int lo = __builtin_amdgcn_update_dpp(__builtin_amdgcn_update_dpp(0, __double2loint(v), 0x104, 0xF, 0xF, true), __double2loint(v), 0x114, 0xF, 0xA, false);
  const int hi = __builtin_amdgcn_update_dpp(__builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x104, 0xF, 0xF, true), __double2hiint(v), 0x114, 0xF, 0xA, false);
  return __hiloint2double(hi, lo);
#else
  const double up = dpp_move<0x104>(v), down = dpp_move<0x114>(v);
  return (threadIdx.x & 4) ? down : up;
#endif
}
/// a <-> b in the lanes that execute the statement (v_swap_b32 per half: as selects a conditional exchange of two doubles is four v_cndmask).
HSD void lane_swap(double& a, double& b) {
#if !defined(HS_EMULATED_DEVICE)
  int al = __double2loint(a), ah = __double2hiint(a), bl = __double2loint(b), bh = __double2hiint(b);
  asm volatile("v_swap_b32 %0, %1" : "+v"(al), "+v"(bl));
  asm volatile("v_swap_b32 %0, %1" : "+v"(ah), "+v"(bh));
  a = __hiloint2double(ah, al), b = __hiloint2double(bh, bl);
#else
  const double t = a;
  a = b, b = t;
#endif
}

/// Sum over the wave, in every lane: a butterfly over lane ^ 32, 16, 8, 4, 2, 1 — the four lower levels on the DPP cross bar (xor 8 = row_ror:8
/// inside a row of 16 lanes), the two upper ones as LDS permutes. (Up to round 6 wave_sum was six __shfl_xor — twelve LDS permutes, ~0.25 us —
/// and this form, same pairs in the same order, i.e. bit-identical sums, was kept for the decision's five sums only: the 39 sums of
/// k_border_bb were 8 - 13 us of that kernel.)
HSD double wave_sum(double v) {
  v += __shfl_xor(v, 32);
  v += __shfl_xor(v, 16);
  v += dpp_move<0x128>(v);
  v += lane_xor4(v);
  v += lane_xor2(v);
  v += lane_xor1(v);
  return v;
}
HSD double wave_sum_fast(double v) { return wave_sum(v); }


/// Deterministic block sum (fixed butterfly inside each wave, waves combined in index order). Result valid on thread 0.
HSD double block_sum(double v, double* lds /* >= blockDim/64 */) {
  v = wave_sum(v);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) lds[w] = v;
  __syncthreads();
  double s = 0;
  if (threadIdx.x == 0)
    for (int i = 0; i < int(blockDim.x >> 6); ++i) s += lds[i];
  __syncthreads();
  return s;
}

/// N block sums at once (same order of additions as N calls of block_sum, two barriers instead of 2 N). Results valid on thread 0.
template <int N>
HSD void block_sum_n(double (&v)[N], double* lds /* >= N * blockDim / 64 */) {
  const int w = threadIdx.x >> 6, nw = int(blockDim.x >> 6);
#pragma unroll
  for (int e = 0; e < N; ++e) {
    v[e] = wave_sum_fast(v[e]);
    if ((threadIdx.x & 63) == 0) lds[e * nw + w] = v[e];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
      double s = 0;
      for (int i = 0; i < nw; ++i) s += lds[e * nw + i];
      v[e] = s;
    }
  }
  __syncthreads();
}

/// Per-lane partial sum / max of a strided array with eight independent loads in flight (a plain `s += p[i]` loop keeps one
/// load in flight per lane and pays the full memory latency per element). Fixed order: bit-reproducible.
HSD double strided_sum(const double* __restrict__ p, int n, int stride = 1, int offset = 0) {
  double s = 0.0;
  for (int i0 = threadIdx.x; i0 < n; i0 += 8 * blockDim.x) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * blockDim.x;
      v[u] = i < n ? p[size_t(i) * stride + offset] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  return s;
}
template <int U = 8>
HSD double strided_max(const double* __restrict__ p, int n) {  // entries >= 0; U independent loads in flight per lane
  double m = 0.0;
  for (int i0 = threadIdx.x; i0 < n; i0 += U * blockDim.x) {
    double v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = i0 + u * blockDim.x;
      v[u] = i < n ? p[i] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) m = fmax(m, v[u]);
  }
  return m;
}

HSD void stage_cps(const double* __restrict__ src, double* dst, int n_doubles) {
  // control points are n x 8 doubles: 16-byte pieces, four loads in flight per lane (one round trip for up to 128 control points
  // per 256 lanes instead of one per piece)
  const double2* s2 = reinterpret_cast<const double2*>(src);
  double2* d2 = reinterpret_cast<double2*>(dst);
  const int n2 = n_doubles / 2;
  for (int i0 = threadIdx.x; i0 < n2; i0 += 4 * blockDim.x) {
    double2 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * blockDim.x;
      v[u] = i < n2 ? s2[i] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = i0 + u * blockDim.x;
      if (i < n2) d2[i] = v[u];
    }
  }
  __syncthreads();
}

/// Free camera coordinates (kernels_calib.hpp; T.nc > 0, the update kernels' CALIB instantiations). The camera term of the landmark back-substitution for camera column c of landmark dl: Y_c[u][c] * y_c, u = 0 .. 2, with y_c = -dc (the
/// solution of the normal equations, as y_p = -step_p):  L' y_l = yh - Yh' (Sp o y_p) - Y_c y_c.
HSD void calib_backsub_term(const Tables& T, int dl, int c, double* t0, double* t1, double* t2) {
  const double* Yc = T.calib_Yc + size_t(dl) * 3 * T.nc + c;
  const double yc = -T.delta_b[T.nb - T.nc + c];
  *t0 = fma(Yc[0], yc, *t0), *t1 = fma(Yc[T.nc], yc, *t1), *t2 = fma(Yc[2 * T.nc], yc, *t2);
}

}  // namespace hs
