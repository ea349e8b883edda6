// build_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_build.py): the fused build of the visual factors, compiled FROM THE PRODUCT'S
// KERNEL SOURCES for the host (tests/emul/hip/hip_runtime.h: one std::thread per lane) and run on a window a Python test hands over.
//   k_build_visual<K> -> k_assemble<K> -> k_finalize_reduced     (hyperslam_amd/csrc/kernels_build.hpp, kernels_schur.hpp)
// with the tables laid out the way prepare() of capi.hip lays them out (host_structure.hpp is shared). Output: the scaled, damped band
// system, its right-hand side, the cost and the Y-hat rows — compared by the test with the oracle's reduced system of the same window.
// Usage: build_harness <window.bin> <out.bin>
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
#include "../../hyperslam_amd/csrc/kernels_linearize.hpp"
#include "../../hyperslam_amd/csrc/kernels_schur.hpp"
#include "../../hyperslam_amd/csrc/kernels_build.hpp"
#include "../../hyperslam_amd/csrc/kernels_factor.hpp"
#include "../../hyperslam_amd/csrc/kernels_backward_sb.hpp"
#include "../../hyperslam_amd/csrc/kernels_update.hpp"

namespace hs {
HSD void finalize_border_body(const Tables&, int, int, int) {}  // (no border unknowns in the harness: never reached)
}  // namespace hs

using namespace hs;

struct Reader {
  FILE* f;
  template <class T>
  std::vector<T> vec(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) {
      fprintf(stderr, "short read\n");
      exit(2);
    }
    return v;
  }
};

template <int K>
static void run(Tables& T, int nb_vis, int R, int L, size_t lds) {
  hs_emul::launch(dim3(nb_vis), dim3(kBlock), lds, [&] { k_build_visual<K>(T, R, L, 1); });
  if (T.wide_q) hs_emul::launch(dim3(landmark_gram_wide_grid(T.sp.n_cp, T.bw)), dim3(kGramWideThreads), 0, [&] { k_landmark_gram_wide(T); });
  if (T.bw * (T.bw + 1) / 2 > kBlock)  // (launch_build's rule: window-wide bands take the instance with the pipelined source loop)
    hs_emul::launch(dim3(T.sp.n_cp, 6), dim3(kAsmWideThreads), 0, [&] { k_assemble_wide<K>(T, 0); });
  else
    hs_emul::launch(dim3(T.sp.n_cp, 6), dim3(kAsmThreads), 0, [&] { k_assemble<K>(T, 0); });
  hs_emul::launch(dim3(T.sp.n_cp + 1), dim3(kBlock), 0, [&] { k_finalize_reduced(T, 1); });
  // Direct mode of k_assemble (scaling fixed: every linearisation of a solve but the first): the same partials scaled, damped and written in
  // the factorisation's layout by k_assemble itself must reproduce k_finalize_reduced's output BIT FOR BIT (same operations on the same sums).
  // (not for window-wide bands: k_assemble_wide deals a row's sources to more slices — another, equally fixed, summation order — and the
  //  product never runs those windows in direct mode: launch_build)
  if (T.st->scaling_ready == 0 && T.bw * (T.bw + 1) / 2 <= kBlock) {  // (first pass of this process: the scaling was just fixed by the finalisation above)
    const size_t nS = size_t(T.np) * 6 * T.bw;
    std::vector<double> Sb(nS), g_s(T.np), g_full(T.np), D2p(T.np), gabs(T.np + 8);
    Tables D = T;
    D.Sb = Sb.data(), D.g_s = g_s.data(), D.g_full = g_full.data(), D.D2p = D2p.data(), D.gabs = gabs.data(), D.Sb2 = nullptr, D.g2 = nullptr;
    hs_emul::launch(dim3(T.sp.n_cp, 6), dim3(kAsmThreads), 0, [&] { k_assemble<K>(D, 1); });
    bool same = true;
    auto eq = [](double a, double b) { return a == b || (a != a && b != b); };  // (a window with a NaN in it — the failure path — builds NaN both ways)
    for (size_t e = 0; e < nS; ++e) same &= eq(Sb[e], T.Sb[e]);
    for (int e = 0; e < T.np; ++e) same &= eq(g_s[e], T.g_s[e]) && eq(g_full[e], T.g_full[e]) && eq(D2p[e], T.D2p[e]) && eq(gabs[e], T.gabs[e]);
    if (!same) {
      fprintf(stderr, "k_assemble direct mode differs from k_finalize_reduced\n");
      exit(7);
    }
  }
}

struct Sizes {
  size_t grpQ, cost_part, Y, nl;
};

/// The decision of an iteration inside the NEXT iteration's build (Tables::fold_decision: workgroup 0 of k_build_visual decides, the chunk
/// workgroups wait for its flag) against k_pack_decision(3) followed by the plain build: solver state, control points and every output of
/// the build must agree BIT FOR BIT — for an accepted step (the chunks then read the point from cp_cand / lm_cand while workgroup 0 copies
/// it) and for a rejected one. U: the tables behind k_update_visual (candidate point and the partials the decision sums).
template <int K>
static void check_fold(const Tables& U, int nb_vis, int R, int L, size_t lds, const Sizes& z, bool accept) {
  double cand = 0.0, d3 = 0.0, d4 = 0.0;
  for (int i = 0; i < nb_vis; ++i) cand += U.cand_part[i];
  for (int i = 0; i < U.n_lm_part; ++i) d3 += U.lm_part[4 * i + 2], d4 += U.lm_part[4 * i + 3];
  DevState st0 = *U.st;
  st0.spec = 4, st0.iteration = 1, st0.max_iterations = 8, st0.scaling_ready = 1;
  st0.cost = accept ? 1.5 * cand : 0.5 * cand;
  const double mcc = 2.0 * std::fabs(st0.cost - cand);  // relative decrease +-0.5
  st0.g_dot_step_pose = -2.0 * mcc - d3 + d4, st0.d2_step2_pose = 0.0, st0.g_dot_step_far = 0.0, st0.d2_step2_far = 0.0;
  struct Run {
    DevState st;
    std::vector<double> cp, grpQ, cost_part, ch_gmax, Y, lm_L, lm_yhat, lm_sb, lm_D2, lm_gmax, xbuf;
  } run[2];
  std::vector<unsigned> flags(8, 0u);
  for (int v = 0; v < 2; ++v) {
    Run& r = run[v];
    r.st = st0;
    r.cp.assign(U.cp, U.cp + 8 * size_t(U.sp.n_cp));
    r.grpQ.assign(z.grpQ, 1e300), r.cost_part.assign(z.cost_part, -1.0), r.ch_gmax.assign(z.cost_part, -1.0), r.Y.assign(z.Y, 0.0);
    r.lm_L.assign(6 * z.nl, 0.0), r.lm_yhat.assign(3 * z.nl, 0.0), r.lm_sb.assign(3 * z.nl, 0.0), r.lm_D2.assign(3 * z.nl, 0.0), r.lm_gmax.assign(z.nl, 0.0);
    r.xbuf.assign(size_t(U.x_count1) + 8, 1e300);
    Tables V = U;
    V.st = &r.st, V.cp = r.cp.data(), V.grpQ = r.grpQ.data(), V.cost_part = r.cost_part.data(), V.ch_gmax = r.ch_gmax.data(), V.Y = r.Y.data();
    V.lm_L = r.lm_L.data(), V.lm_yhat = r.lm_yhat.data(), V.lm_sb = r.lm_sb.data(), V.lm_D2 = r.lm_D2.data(), V.lm_gmax = r.lm_gmax.data(), V.xbuf = r.xbuf.data();
    V.join_flag = flags.data();
    if (v == 0) {
      hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_pack_decision(V, 3); });
      hs_emul::launch(dim3(nb_vis), dim3(kBlock), lds, [&] { k_build_visual<K>(V, R, L, 1); });
    } else {
      V.fold_decision = 1, V.fold_epoch = 5;
      hs_emul::launch(dim3(nb_vis + 1), dim3(kBlock), lds, [&] { k_build_visual<K>(V, R, L, 1); });
    }
  }
  bool same = std::memcmp(&run[0].st, &run[1].st, sizeof(DevState)) == 0 && run[0].st.accepted == (accept ? 1 : 0) && !run[0].st.done;
  auto eq = [&](const std::vector<double>& a, const std::vector<double>& b) { same &= std::memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0; };
  eq(run[0].cp, run[1].cp), eq(run[0].grpQ, run[1].grpQ), eq(run[0].cost_part, run[1].cost_part), eq(run[0].ch_gmax, run[1].ch_gmax), eq(run[0].Y, run[1].Y);
  eq(run[0].lm_L, run[1].lm_L), eq(run[0].lm_yhat, run[1].lm_yhat), eq(run[0].lm_sb, run[1].lm_sb), eq(run[0].lm_D2, run[1].lm_D2), eq(run[0].lm_gmax, run[1].lm_gmax);
  if (accept) same &= std::memcmp(run[1].cp.data(), U.cp_cand, 8 * size_t(U.sp.n_cp) * sizeof(double)) == 0;  // the accepted point was committed
  if (!same) {
    fprintf(stderr, "decision folded into k_build_visual differs from k_pack_decision + k_build_visual (%s step)\n", accept ? "accepted" : "rejected");
    exit(8);
  }
}

/// The candidate point two ways: k_update_visual (per chunk) against k_backsub_retract + k_cost_visual (per landmark / per residual).
template <int K>
static void run_update(Tables& T, int nb_vis, int R, int L, std::vector<double>* out, size_t build_lds, const Sizes& z, bool fold_check, bool decide,
                       std::vector<double>* dec) {
  const int n_lm = T.n_lm, n_cp = T.sp.n_cp;
  std::vector<double> lm_cand_a(3 * size_t(std::max(n_lm, 1))), cp_cand_a(8 * size_t(n_cp)), cand_a(nb_vis + 1), norm_a(2 * size_t(T.n_norm_part));
  std::vector<double> lm_part_a(4 * size_t((n_lm + 3) / 4) + 4);
  Tables A = T;
  A.lm_cand = lm_cand_a.data(), A.cp_cand = cp_cand_a.data(), A.cand_part = cand_a.data(), A.norm_part = norm_a.data(), A.lm_part = lm_part_a.data();
  A.n_lm_part = (n_lm + 3) / 4;
  hs_emul::launch(dim3(A.n_lm_part + A.n_norm_part), dim3(kBlock), 0, [&] { k_backsub_retract(A); });
  hs_emul::launch(dim3(nb_vis), dim3(kBlock), size_t(8) * n_cp * 8, [&] { k_cost_visual<K>(A, A.cp_cand, A.lm_cand, A.cand_part); });
  std::vector<double> lm_cand_b(3 * size_t(std::max(n_lm, 1))), cp_cand_b(8 * size_t(n_cp)), cand_b(nb_vis + 1), norm_b(2 * size_t(T.n_norm_part));
  std::vector<double> lm_part_b(4 * size_t(nb_vis) + 4);
  Tables B = T;
  B.lm_cand = lm_cand_b.data(), B.cp_cand = cp_cand_b.data(), B.cand_part = cand_b.data(), B.norm_part = norm_b.data(), B.lm_part = lm_part_b.data();
  B.n_lm_part = nb_vis;
  hs_emul::launch(dim3(nb_vis + B.n_norm_part), dim3(kBlock), size_t(update_lds_doubles(T.bw, R, L)) * 8, [&] { k_update_visual<K>(B, R, L, nb_vis); });
  if (fold_check) check_fold<K>(B, nb_vis, R, L, build_lds, z, true), check_fold<K>(B, nb_vis, R, L, build_lds, z, false);
  auto sum = [](const std::vector<double>& v, size_t n, size_t stride = 1, size_t off = 0) {
    double s = 0;
    for (size_t i = 0; i < n; ++i) s += v[i * stride + off];
    return s;
  };
  double dlm = 0, dcp = 0;
  for (size_t i = 0; i < 3 * size_t(n_lm); ++i) dlm = std::max(dlm, std::fabs(lm_cand_a[i] - lm_cand_b[i]));
  for (size_t i = 0; i < 8 * size_t(n_cp); ++i) dcp = std::max(dcp, std::fabs(cp_cand_a[i] - cp_cand_b[i]));
  out->assign({dlm, dcp, sum(cand_a, nb_vis), sum(cand_b, nb_vis)});
  for (int e = 0; e < 4; ++e) out->push_back(sum(lm_part_a, A.n_lm_part, 4, e)), out->push_back(sum(lm_part_b, B.n_lm_part, 4, e));
  for (int e = 0; e < 2; ++e) out->push_back(sum(norm_a, T.n_norm_part, 2, e)), out->push_back(sum(norm_b, T.n_norm_part, 2, e));
  if (decide) {  // full iteration: the trust-region decision on the fused path's partials (k_pack_decision(3): decides, commits the control points)
    std::vector<double> cp_work(T.cp, T.cp + 8 * size_t(n_cp));
    B.cp = cp_work.data();
    const int verdict = B.st->chol_failed;  // as the factorisation left it: the decision consumes and clears it
    const hs_iteration& rd = B.st->records[B.st->iteration];  // the record this decision writes (records[0] is the start point's: begin_iteration)
    hs_emul::launch(dim3(1), dim3(kBlock), 0, [&] { k_pack_decision(B, 3); });
    const hs_iteration& r = B.st->records[0];
    // the state as the decision leaves it, and the point: control points (the decision's working copy) and landmarks in device order
    dec->assign({double(verdict), double(B.st->chol_failed), double(B.st->invalid_streak), B.st->radius, double(B.st->accepted), double(B.st->done),
                 double(B.st->termination), double(rd.step_is_valid), double(rd.step_is_successful)});
    dec->insert(dec->end(), cp_work.begin(), cp_work.end());
    dec->insert(dec->end(), B.lm, B.lm + 3 * size_t(n_lm));
    out->insert(out->end(), {r.cost, r.cost_change, r.gradient_max_norm, r.step_norm, r.relative_decrease, r.radius, double(r.step_is_valid), double(r.step_is_successful),
                             B.st->cost, double(B.st->accepted), double(B.st->done)});
    double dcp = 0;  // an accepted candidate was committed
    for (size_t i = 0; i < 8 * size_t(n_cp); ++i) dcp = std::max(dcp, std::fabs(cp_work[i] - (B.st->accepted ? cp_cand_b[i] : T.cp[i])));
    out->push_back(dcp);
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  Reader rd{fopen(argv[1], "rb")};
  if (!rd.f) return 1;
  const std::vector<int> hdr = rd.vec<int>(12);
  const int k = hdr[0], n_cp = hdr[1], n_lm = hdr[2], n_px = hdr[3], n_br = hdr[4], n_cam = hdr[5], rot_c = hdr[6], tr_c = hdr[7];
  int R = hdr[8], L = hdr[9];
  const int scaling_ready = hdr[10];
  const bool fold_check = (hdr[11] & 1) != 0;  // also run the decision folded into the build against k_pack_decision + build (check_fold)
  const bool full_iteration = (hdr[11] & 2) != 0;  // factor + sweeps on the built system, the update along the REAL step, the decision: one LM iteration
  const bool failure_expected = (hdr[11] & 4) != 0;  // full iteration: a factorisation that raises chol_failed is carried through the update and the decision
  const std::vector<double> par = rd.vec<double>(3);
  const double t0 = par[0], dt = par[1], radius = par[2];
  std::vector<double> cp = rd.vec<double>(size_t(8) * n_cp);
  const std::vector<int> cpc_i = rd.vec<int>(n_cp);
  std::vector<double> cam = rd.vec<double>(size_t(16) * n_cam);
  const std::vector<double> lm_tab = rd.vec<double>(size_t(3) * n_lm);
  const std::vector<int> lmc_i = rd.vec<int>(n_lm);
  const std::vector<double> px_stamp = rd.vec<double>(n_px), px_meas = rd.vec<double>(size_t(2) * n_px);
  const std::vector<int> px_lm = rd.vec<int>(n_px), px_cam = rd.vec<int>(n_px);
  const std::vector<double> br_stamp = rd.vec<double>(n_br), br_meas = rd.vec<double>(size_t(3) * n_br);
  const std::vector<int> br_lm = rd.vec<int>(n_br), br_cam = rd.vec<int>(n_br);
  const std::vector<double> lm_scale_in = rd.vec<double>(scaling_ready ? size_t(3) * n_lm : 0);  // table order
  const std::vector<double> scale_p_in = rd.vec<double>(scaling_ready ? size_t(6) * n_cp : 0);
  fclose(rd.f);

  VisualStructure vs;
  std::string err;
  VisualInput in = {k, n_cp, n_lm, t0, dt, n_px, n_br, px_stamp.data(), br_stamp.data(), px_lm.data(), br_lm.data()};
  if (!build_visual_structure(in, &vs, &err)) {
    fprintf(stderr, "%s\n", err.c_str());
    return 3;
  }
  const int n_vis = n_px + n_br, bw = vs.bw, np = 6 * n_cp, ncb = 6 * bw, ntile = bw * (bw + 1) / 2;
  {
    auto lds_bytes = [&](int r, int l) { return size_t(build_lds_layout(k, bw, r, l).total_doubles) * 8; };
    if (!choose_build_geometry(k, R ? R : (k == 4 ? 128 : k == 5 ? 112 : 96), L ? L : (k == 4 ? 12 : k == 5 ? 11 : 10), size_t(79) * 1024, size_t(156) * 1024, lds_bytes, &R, &L)) return 5;
  }
  std::vector<int> ch_ptr, gw_ptr, gw_cf, ch_desc;
  if (!build_chunks(vs, n_cp, R, L, &ch_ptr, &gw_ptr, &gw_cf, &ch_desc)) return 6;  // a landmark with more than R residuals: record path in the library
  // the dispatch order of the chunks (a permutation of the descriptors; partial slots by chunk id): "two rounds" rule of a device with 2/3 n CUs
  order_chunks_for_dispatch(vs, k, std::max(1, 2 * (int(ch_ptr.size()) - 1) / 3), &ch_desc, int(ch_ptr.size()) - 1);
  const int n_chunk = int(ch_ptr.size()) - 1;

  // device-order tables (prepare() of capi.hip)
  std::vector<double> lm_dev(size_t(3) * n_lm), lm_scale(size_t(3) * std::max(n_lm, 1), 1.0);
  std::vector<uint8_t> lmc_dev(n_lm), cpc(n_cp);
  for (int i = 0; i < n_cp; ++i) cpc[i] = uint8_t(cpc_i[i]);
  for (int d = 0; d < n_lm; ++d) {
    const int t = vs.table_of_dev[d];
    for (int c = 0; c < 3; ++c) lm_dev[3 * d + c] = lm_tab[3 * t + c];
    if (scaling_ready)
      for (int c = 0; c < 3; ++c) lm_scale[3 * d + c] = lm_scale_in[3 * t + c];
    lmc_dev[d] = uint8_t(lmc_i[t]);
  }
  std::vector<double> v_stamp(n_vis), v_meas(size_t(3) * n_vis);
  std::vector<int> v_info(n_vis);
  for (int q = 0; q < n_vis; ++q) {
    const int ti = vs.table_idx[q];
    if (vs.table_type[q] == HS_PIXEL) {
      v_stamp[q] = px_stamp[ti], v_meas[3 * q] = px_meas[2 * ti], v_meas[3 * q + 1] = px_meas[2 * ti + 1], v_meas[3 * q + 2] = 0.0;
      v_info[q] = px_cam[ti];
    } else {
      v_stamp[q] = br_stamp[ti];
      for (int c = 0; c < 3; ++c) v_meas[3 * q + c] = br_meas[3 * ti + c];
      v_info[q] = br_cam[ti] | (1 << 16);
    }
  }
  const size_t nl = size_t(std::max(n_lm, 1));
  std::vector<double> lm_L(6 * nl), lm_yhat(3 * nl), lm_sb(3 * nl), lm_D2(3 * nl), lm_gmax(nl), Y(size_t(vs.y_total) + 1);
  const int nb_vis = std::max((n_vis + kBlock - 1) / kBlock, n_chunk);
  ch_desc.resize(size_t(8) * nb_vis, 0);
  std::vector<double> cost_part(nb_vis + 1, -1.0), grpQ(size_t(n_chunk) * (size_t(ntile) * 36 + 3 * ncb) + 1, 1e300), segP(1);
  std::vector<int> sw_ptr(n_cp - k + 2, 0), sw_seg(1, 0);
  const int x_count1 = np * (ncb + 3) + 2;
  std::vector<double> xbuf(size_t(x_count1) + 8, 1e300), scale_p(np, 1.0), Sb(size_t(np) * ncb, 0.0), g_s(np), g_full(np), D2p(np), gabs(np + 1);
  if (scaling_ready) scale_p = scale_p_in;
  DevState st;
  std::memset(&st, 0, sizeof(st));
  st.radius = radius, st.decrease_factor = 2.0, st.max_iterations = 1, st.scaling_ready = scaling_ready;

  Tables T;
  std::memset(&T, 0, sizeof(T));
  T.sp = Spline{k, n_cp, t0, dt, 1.0 / dt, rot_c, tr_c};
  T.basis = make_basis_coef(k);
  T.cp = cp.data(), T.cp_cand = cp.data(), T.cp_const = cpc.data(), T.cam = cam.data(), T.n_cam = n_cam;
  T.n_lm = n_lm, T.lm = lm_dev.data(), T.lm_cand = lm_dev.data(), T.lm_const = lmc_dev.data();
  T.lm_ptr = vs.lm_ptr.data(), T.lm_cfirst = vs.lm_cfirst.data(), T.lm_ncp = vs.lm_ncp.data(), T.lm_yoff = vs.lm_yoff.data(), T.cf_ptr = vs.cf_ptr.data();
  T.lm_scale = lm_scale.data(), T.lm_L = lm_L.data(), T.lm_yhat = lm_yhat.data(), T.lm_sb = lm_sb.data(), T.lm_D2 = lm_D2.data();
  std::vector<double> ch_gmax(size_t(nb_vis) + 1);
  T.lm_gmax = lm_gmax.data(), T.Y = Y.data(), T.ch_gmax = ch_gmax.data();
  {
    int n_obs = n_lm;
    while (n_obs > 0 && vs.lm_ptr[n_obs] == vs.lm_ptr[n_obs - 1]) --n_obs;
    T.n_obs_lm = n_obs;
  }
  T.n_vis = n_vis, T.v_stamp = v_stamp.data(), T.v_meas = v_meas.data(), T.v_lm = vs.lm_dev.data(), T.v_info = v_info.data();
  T.v_first = vs.first.data(), T.v_pos = vs.pos.data(), T.v_seg_ptr = vs.seg_ptr.data();
  T.n_seg = n_cp - k + 1, T.bw = bw, T.np = np;
  T.scale_p = scale_p.data(), T.Sb = Sb.data(), T.g_s = g_s.data(), T.g_full = g_full.data(), T.D2p = D2p.data(), T.gabs = gabs.data();
  T.cost_part = cost_part.data(), T.n_cost_part = nb_vis;
  T.xbuf = xbuf.data(), T.segP = segP.data(), T.grpQ = grpQ.data();
  T.gw_ptr = gw_ptr.data(), T.gw_cf = gw_cf.data(), T.sw_ptr = sw_ptr.data(), T.sw_seg = sw_seg.data();
  T.xo_g = np * ncb, T.xo_gs = T.xo_g + np, T.xo_dj = T.xo_gs + np, T.xo_pb = T.xo_dj + np, T.xo_bb = T.xo_pb, T.xo_gb = T.xo_bb, T.xo_cost = T.xo_gb, T.xo_gmax = T.xo_cost + 1;
  T.x_count1 = x_count1, T.xo_dec = x_count1;
  T.fused = 1, T.n_chunk = n_chunk, T.ch_ptr = ch_ptr.data(), T.ch_desc = ch_desc.data();
  T.build_stream_lg = hs::build_streams_packed(vs.bw, k);
  std::vector<double> Qw(size_t(np) * (ncb + 1) + 1, 1e300);  // (prepare()'s rule: window-wide bands form the landmark term once per window)
  const int yt_stride = (n_lm + 63) / 64 * 64;
  std::vector<double> Yt(size_t(18) * n_cp * yt_stride + 2, 1e300);
  T.Yt = Yt.data(), T.yt_stride = yt_stride;
  T.wide_q = ntile > kBlock && !(std::getenv("HS_WIDE_Q") && std::atoi(std::getenv("HS_WIDE_Q")) == 0) ? 1 : 0, T.Qw = Qw.data();
  T.rank = 0, T.world = 1, T.st = &st;

  const size_t lds = size_t(build_lds_layout(k, bw, R, L).total_doubles) * 8;
  if (k == 4)
    run<4>(T, nb_vis, R, L, lds);
  else if (k == 5)
    run<5>(T, nb_vis, R, L, lds);
  else if (k == 6)
    run<6>(T, nb_vis, R, L, lds);
  else
    return 4;

  // a step to retract along (any vector will do for the comparison of the two update paths): step_p fabricated, delta_p = s_p o step_p
  std::vector<double> step_p(np), delta_p(np), lm_sb_dummy;
  for (int i = 0; i < np; ++i) step_p[i] = 1e-2 * std::sin(0.37 * i + 0.1) * (D2p[i] != 0.0 ? 1.0 : 0.0), delta_p[i] = -step_p[i] * scale_p[i];
  // Full iteration: the REAL step instead — the band Cholesky of the system built above and the sweeps, with launch_factor's choices for a
  // short window (one-ended: fewer than 4 bw block rows; look-ahead kernel where the band fits its compute waves, k_band_factor<1> otherwise)
  const int n_blk = np / 6;
  std::vector<double> Ub(size_t(np) * ncb, 0.0), Ubk(size_t(24) * n_blk, 0.0), ybuf(np, 0.0), Vb(size_t(sb_count(n_blk) + 1) * kSbN * kSbN, 0.0), xpart(8 * 1024, 0.0);
  std::vector<unsigned> join_flag(kSbFlagBase + 2 * kSbMaxBlocks, 0u);
  if (full_iteration) {
    if (n_blk >= 4 * bw || 6 * (bw - 1) > 96) return 9;  // (two-ended / wide-band windows: tests/emul/factor_harness.cpp)
    T.Ub = Ub.data(), T.Ubk = Ubk.data(), T.ybuf = ybuf.data(), T.join_flag = join_flag.data(), T.join_epoch = 1, T.xpart = xpart.data();
    T.step_p = step_p.data(), T.delta_p = delta_p.data();
    T.fj[0] = FactorJob{T.Sb, T.g_s, T.Ub, T.Ubk, T.ybuf, nullptr, n_blk, -1};
    const size_t la_lds = (size_t(42) * (ncb + 2) + size_t(np) + 48) * sizeof(double), chol_lds = (size_t(24) * (ncb + 2) + size_t(np)) * sizeof(double);
    const int ncw = la_compute_waves(bw);
    if (ncw == 3)
      hs_emul::launch(dim3(1), dim3(la_threads(3)), la_lds, [&] { k_band_factor_la<1, 3>(T); });
    else if (ncw == 4)
      hs_emul::launch(dim3(1), dim3(la_threads(4)), la_lds, [&] { k_band_factor_la<1, 4>(T); });
    else if (bw * bw <= kCholThreads)
      hs_emul::launch(dim3(1), dim3(kCholThreads + kCholIo), chol_lds, [&] { k_band_factor<1>(T); });
    else
      return 9;
    T.join_epoch = 2;
    const BackJob j0{T.Ub, T.Ubk, T.ybuf, Vb.data(), nullptr, n_blk, 0, 0};
    const unsigned n_wg = 1 + sb_count(n_blk);
    std::vector<unsigned> order;
    for (unsigned w = 1; w < n_wg; ++w) order.push_back(w);
    order.push_back(0);  // the inverse builders, then the sweep
    hs_emul::launch(dim3(n_wg), dim3(kCholThreads), std::max((2 * size_t(np) + 32) * sizeof(double), size_t(3 * kSbN * (kSbN + 1)) * sizeof(double)),
                    [&] { k_band_backward_sb(T, j0, j0, -1, 1, 0); }, order);
    if (st.chol_failed && !failure_expected) return 10;
  }
  std::vector<double> norm_part(2), upd, dec;
  T.step_p = step_p.data(), T.delta_p = delta_p.data(), T.n_norm_part = std::max((n_cp + kBlock - 1) / kBlock, 1), T.norm_part = norm_part.data();
  const Sizes z{grpQ.size(), cost_part.size(), Y.size(), nl};
  if (k == 4)
    run_update<4>(T, nb_vis, R, L, &upd, lds, z, fold_check, full_iteration, &dec);
  else if (k == 5)
    run_update<5>(T, nb_vis, R, L, &upd, lds, z, fold_check, full_iteration, &dec);
  else
    run_update<6>(T, nb_vis, R, L, &upd, lds, z, fold_check, full_iteration, &dec);

  FILE* out = fopen(argv[2], "wb");
  const int ohdr[8] = {bw, np, n_chunk, R, L, vs.y_total, int(lds), int(upd.size())};
  fwrite(ohdr, sizeof(int), 8, out);
  const double cost = st.cost;
  fwrite(&cost, 8, 1, out);
  fwrite(Sb.data(), 8, Sb.size(), out);
  fwrite(g_s.data(), 8, g_s.size(), out);
  fwrite(Y.data(), 8, size_t(vs.y_total), out);
  // landmark scaling back in table order, pose scaling (so that a second call can run with the scaling fixed)
  std::vector<double> ls_tab(size_t(3) * n_lm);
  for (int d = 0; d < n_lm; ++d)
    for (int c = 0; c < 3; ++c) ls_tab[3 * vs.table_of_dev[d] + c] = lm_scale[3 * d + c];
  fwrite(ls_tab.data(), 8, ls_tab.size(), out);
  fwrite(scale_p.data(), 8, scale_p.size(), out);
  fwrite(upd.data(), 8, upd.size(), out);
  if (full_iteration) {  // behind everything else: what the decision left (9 words of state, 8 n_cp control points, the landmarks back in table order)
    std::vector<double> lm_tab_out(size_t(3) * n_lm);
    for (int d = 0; d < n_lm; ++d)
      for (int c = 0; c < 3; ++c) lm_tab_out[3 * vs.table_of_dev[d] + c] = dec[9 + 8 * size_t(n_cp) + 3 * d + c];
    fwrite(dec.data(), 8, 9 + 8 * size_t(n_cp), out);
    fwrite(lm_tab_out.data(), 8, lm_tab_out.size(), out);
  }
  fclose(out);
  return 0;
}
