// spline_harness.cpp — TEST INFRASTRUCTURE (tests/test_emulated_spline.py): the spline routines of hyperslam_amd/csrc/device_spline.hpp and
// basis_weights<K> / segment_of of csrc/device_math.hpp, compiled FROM THE PRODUCT'S SOURCES for the host (tests/emul/hip/hip_runtime.h) and
// run query by query:
//   spline_pose, spline_pose_pre, spline_pose_jac, spline_pose_jac_pre, spline_full<K, true>, spline_full<K, false>, spline_full_col (every m)
// Input (text): n, then per query "K stamp t0 dt" and K rows of 8 doubles (control points of the segment, t0 = the stamp of the first).
// Output (text, %.17g), per query one line per routine, "name values...":
//   lam K | pose 7 | pose_pre 7 | jac 7 + 9K | jac_pre 7 + 9K | full 19 + 27K + 3K (q p w al v a, dth, dw, dal, B Bd Bdd) | full_value 19
//   | col<m> 19 + 27 + 1 (blocks of control point m, Bdd_m)
// Usage: spline_harness <in.txt> <out.txt>
#include <cstdio>
#include <vector>

#include "hip/hip_runtime.h"

thread_local dim3 threadIdx;
thread_local unsigned hs_emul::exchange_count = 0;
dim3 blockIdx, blockDim, gridDim;

#include "../../hyperslam_amd/csrc/host_structure.hpp"
#include "../../hyperslam_amd/csrc/device_spline.hpp"

using namespace hsd;

static FILE* out;
static void put(const double* v, int n) {
  for (int i = 0; i < n; ++i) fprintf(out, " %.17g", v[i]);
}
static void put(Quat q, V3 p) { fprintf(out, " %.17g %.17g %.17g %.17g %.17g %.17g %.17g", q.x, q.y, q.z, q.w, p.x, p.y, p.z); }
static void put(V3 v) { fprintf(out, " %.17g %.17g %.17g", v.x, v.y, v.z); }
static void put(const M3& m) { put(m.m, 9); }

template <int K>
static int query(const double* cp, double stamp, double t0, double dt) {
  double u;
  if (segment_of(stamp, t0, dt, K, &u) != 0) return 3;
  const BasisCoef bc = hs::make_basis_coef(K);
  double lam[K], dlam[K], ddlam[K];
  basis_weights<K>(bc, u, 1.0 / dt, lam, dlam, ddlam, 2);
  fprintf(out, "lam"), put(lam, K), fprintf(out, "\n");
  Quat q;
  V3 p;
  M3 G[K];
  RelPre rel[K - 1];
  for (int j = 1; j < K; ++j) rel[j - 1] = rel_precompute(cp + 8 * (j - 1), cp + 8 * j);
  spline_pose<K>(cp, lam, &q, &p);
  fprintf(out, "pose"), put(q, p), fprintf(out, "\n");
  spline_pose_pre<K>(cp, rel, lam, &q, &p);
  fprintf(out, "pose_pre"), put(q, p), fprintf(out, "\n");
  spline_pose_jac<K>(cp, lam, &q, &p, G);
  fprintf(out, "jac"), put(q, p);
  for (int j = 0; j < K; ++j) put(G[j]);
  fprintf(out, "\n");
  spline_pose_jac_pre<K>(cp, rel, lam, &q, &p, G);
  fprintf(out, "jac_pre"), put(q, p);
  for (int j = 0; j < K; ++j) put(G[j]);
  fprintf(out, "\n");
  SplineFull<K> f;
  spline_full<K, true>(cp, lam, dlam, ddlam, &f);
  fprintf(out, "full"), put(f.q, f.p), put(f.w), put(f.al), put(f.v), put(f.a);
  for (int j = 0; j < K; ++j) put(f.dth[j]);
  for (int j = 0; j < K; ++j) put(f.dw[j]);
  for (int j = 0; j < K; ++j) put(f.dal[j]);
  put(f.B, K), put(f.Bd, K), put(f.Bdd, K), fprintf(out, "\n");
  SplineFull<K> v;
  spline_full<K, false>(cp, lam, dlam, ddlam, &v);
  fprintf(out, "full_value"), put(v.q, v.p), put(v.w), put(v.al), put(v.v), put(v.a), fprintf(out, "\n");
  for (int m = 0; m < K; ++m) {
    SplineCol<K> c;
    spline_full_col<K>(cp, lam, dlam, ddlam, m, &c);
    fprintf(out, "col%d", m), put(c.q, c.p), put(c.w), put(c.al), put(c.v), put(c.a), put(c.dth), put(c.dw), put(c.dal), put(&c.Bdd_m, 1), fprintf(out, "\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 1;
  FILE* in = fopen(argv[1], "r");
  out = fopen(argv[2], "w");
  if (!in || !out) return 1;
  int n = 0;
  if (fscanf(in, "%d", &n) != 1) return 2;
  for (int i = 0; i < n; ++i) {
    int K;
    double stamp, t0, dt;
    if (fscanf(in, "%d %lf %lf %lf", &K, &stamp, &t0, &dt) != 4 || K < 4 || K > 6) return 2;
    std::vector<double> cp(size_t(8) * K);
    for (double& v : cp)
      if (fscanf(in, "%lf", &v) != 1) return 2;
    const int rc = K == 4 ? query<4>(cp.data(), stamp, t0, dt) : K == 5 ? query<5>(cp.data(), stamp, t0, dt) : query<6>(cp.data(), stamp, t0, dt);
    if (rc) return rc;
  }
  fclose(in), fclose(out);
  return 0;
}
