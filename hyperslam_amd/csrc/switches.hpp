// switches.hpp — the measurement switches of HS_DEBUG_FLAGS: the one table (plain C++: device code, host code, the emulator builds under
// tests/emul/ and — read as text — hyperslam_amd/switches.py all take it from here).
//
// HS_DEBUG_FLAGS is ONE decimal number in the environment, read by prepare(); a switch is one bit of it, its value 2^bit. None is ever
// needed for correct operation: each selects an alternative kept to be measured against (or a set of timestamps). The values are frozen —
// bench.py, profiles/ and the documents quote them.
//   HS_SWITCH(name, bit, "meaning"): the name says which alternative the switch SELECTS.
//   "profiling": compiled into profiling builds only (HS_PROFILE_HOOKS = 1, tools/build_profiling_lib.sh); through HS_AB / prof_enabled
//   a compile-time false in the product library. Every other switch works in the product library too.
// Bit 13 has two names (border_solve_reg, backward2_one_ended): two unrelated meanings that never meet — one needs a border, the other
// needs none. It is the only shared bit.
// (Not a switch of this table: the sign of Tables::debug_flags — HS_DEBUG_FLAGS 2147483648, profiling builds, the fixed stream rule of
//  k_build_visual.)
#pragma once

// clang-format off
#define HS_SWITCH_TABLE \
  HS_SWITCH(skip_backward,        0, "skip the backward sweep, k_band_backward (timing only: results are garbage)") \
  HS_SWITCH(skip_rank6,           1, "skip the rank-6 updates: the panel chain alone (timing only: results are garbage)") \
  HS_SWITCH(factor_legacy,        2, "one-ended pre-look-ahead factorisation kernel, k_band_factor") \
  HS_SWITCH(no_dense_mx,          3, "small systems: one-ended band kernels + border chain + k_band_backward, no k_dense_solve_mx") \
  HS_SWITCH(stamp_factor,         4, "profiling: phase stamps of the factorisation and the sweeps -> hs_debug_read") \
  HS_SWITCH(stamp_build,          5, "profiling: per-workgroup stamps of the linearise / gram / build kernels") \
  HS_SWITCH(factor_la,            6, "two-ended factorisation on the VALU look-ahead kernel k_band_factor_la, not k_band_factor_mx") \
  HS_SWITCH(sweep_behind,         7, "border forward sweep behind the two-ended factorisation, not alongside it") \
  HS_SWITCH(stamp_assemble,       8, "profiling: phase stamps of k_assemble") \
  HS_SWITCH(stamp_update,         9, "profiling: phase stamps of k_update_visual") \
  HS_SWITCH(no_gram_pair,        10, "k_seg_gram on a side stream next to k_landmark -> k_group_gram, no k_gram_pair") \
  HS_SWITCH(one_ended,           11, "one-ended factorisation (no second workgroup)") \
  HS_SWITCH(finalize_always,     12, "k_finalize_reduced in every iteration (no direct mode of k_assemble)") \
  HS_SWITCH(border_solve_reg,    13, "with a border: k_border_solve_reg, not k_dense_solve_mx, on the border Schur complement of a two-ended system") \
  HS_SWITCH(backward2_one_ended, 13, "profiling, no border (shares bit 13): the generalised sweep k_band_backward2 on a one-ended factor") \
  HS_SWITCH(join_events,         14, "border gathers / pipelined border sweep joined by events, not device flags (Tables::gather_epoch, sweep_epoch)") \
  HS_SWITCH(decide_always,       15, "k_pack_decision behind every update (no decision folded into the next k_build_visual)") \
  HS_SWITCH(backward_w,          16, "profiling: single-wave register backward sweep k_band_backward_w") \
  HS_SWITCH(factor_mfma,         17, "profiling: k_band_factor_mfma instead of the VALU factorisation kernels") \
  HS_SWITCH(no_decouple,         18, "eliminate the block rows of leading constant control points like any other") \
  HS_SWITCH(border_lds,          19, "border Cholesky in LDS, k_border_solve, not k_border_solve_reg") \
  HS_SWITCH(imu_main_stream,     20, "inertial branch on the main stream (no side stream)") \
  HS_SWITCH(no_dense_factor,     21, "banded kernels instead of k_dense_factor") \
  HS_SWITCH(landmark_wave,       22, "k_landmark<K,4,1> (one wave per landmark, four passes) instead of k_landmark_rows") \
  HS_SWITCH(finalize_five,       23, "five finalisation launches for a bordered single shard") \
  HS_SWITCH(commit_launch,       24, "k_commit launch for small windows (no commit inside the decision kernel)") \
  HS_SWITCH(cost_per_type,       25, "one candidate cost launch per factor type, no k_cost_all") \
  HS_SWITCH(commit_always,       26, "k_commit in every iteration (no deferred commit)") \
  HS_SWITCH(cost_own_launches,   27, "prior / inertial candidate costs as launches of their own behind k_update_visual") \
  HS_SWITCH(backward_rows,       28, "backward sweeps one block row per step (two-ended: profiling, k_band_backward2)") \
  HS_SWITCH(border_one_ended,    29, "bordered systems one-ended") \
  HS_SWITCH(no_speculation,      30, "no speculative linearisation at the candidate") \
  HS_SWITCH(backward_sb,         32, "backward sweep in two phases per super-step: k_band_backward_sb, not k_band_backward_pm")
// clang-format on

namespace hs {

/// A switch is a type of its own, so that every test of one is a constant mask where it is compiled.
template <unsigned long long Mask>
struct Switch {
  static constexpr unsigned long long mask = Mask;  // its value in HS_DEBUG_FLAGS
  /// As a mask of the first word, Tables::debug_flags. Device code, which only has switches of that word, tests `T.debug_flags & sw::name.low()`.
  __attribute__((always_inline)) static constexpr int low() {
    static_assert((Mask >> 32) == 0, "a switch of the second word: switch_on(T, ..)");
    return int(Mask);
  }
};

namespace sw {
#define HS_SWITCH(name, bit, meaning) constexpr Switch<(1ull << (bit))> name{};
HS_SWITCH_TABLE
#undef HS_SWITCH
}  // namespace sw

/// Is the switch set? Host code: hides that `Tables` keeps the number in two ints (kernel argument layout), debug_flags = bits 0 .. 31 and
/// debug_flags2 = bits 32 .. (TablesT: this header knows no project type; it is called with a `Tables`).
template <class TablesT, unsigned long long Mask>
constexpr bool switch_on(const TablesT& T, Switch<Mask> s) {
  if constexpr ((Mask >> 32) != 0)
    return (T.debug_flags2 & int(Mask >> 32)) != 0;
  else
    return (T.debug_flags & s.low()) != 0;
}

}  // namespace hs
