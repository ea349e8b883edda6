// chunks_balanced_dump.cpp — test helper: runs hs::build_chunks_balanced and hs::order_chunks_by_records (hyperslam_amd/csrc/host_structure.hpp:
// the work list of the fused build and its dispatch order) on the tables of a binary input file (the format of structure_dump.cpp) and dumps
// what they produce; tests/test_host_chunks_balanced.py compares it with an independent numpy restatement of the rules. Host-only program.
// usage: chunks_balanced_dump <in> <out> <R> <L>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "host_structure.hpp"

static std::vector<int> read_ints(FILE* f, int n) {
  std::vector<int> v(n);
  if (n && fread(v.data(), sizeof(int), n, f) != size_t(n)) exit(2);
  return v;
}
static std::vector<double> read_doubles(FILE* f, int n) {
  std::vector<double> v(n);
  if (n && fread(v.data(), sizeof(double), n, f) != size_t(n)) exit(2);
  return v;
}
static void dump(FILE* f, const std::string& name, const std::vector<int>& v) {
  fprintf(f, "%s %zu", name.c_str(), v.size());
  for (int x : v) fprintf(f, " %d", x);
  fprintf(f, "\n");
}

int main(int argc, char** argv) {
  if (argc < 5) return 1;
  FILE* in = fopen(argv[1], "rb");
  if (!in) return 1;
  int hdr[5];   // k, n_cp, n_lm, n_px, n_br
  double t[2];  // t0, dt
  if (fread(hdr, sizeof(int), 5, in) != 5 || fread(t, sizeof(double), 2, in) != 2) return 2;
  const std::vector<double> px_stamp = read_doubles(in, hdr[3]), br_stamp = read_doubles(in, hdr[4]);
  const std::vector<int> px_lm = read_ints(in, hdr[3]), br_lm = read_ints(in, hdr[4]);
  fclose(in);
  hs::VisualInput vi = {hdr[0], hdr[1], hdr[2], t[0], t[1], hdr[3], hdr[4], px_stamp.data(), br_stamp.data(), px_lm.data(), br_lm.data()};
  hs::VisualStructure vs;
  std::string err;
  FILE* out = fopen(argv[2], "w");
  if (!hs::build_visual_structure(vi, &vs, &err)) {
    fprintf(out, "error %s\n", err.c_str());
    fclose(out);
    return 0;
  }
  dump(out, "lm_ptr", vs.lm_ptr), dump(out, "cf_ptr", vs.cf_ptr), dump(out, "lm_cfirst", vs.lm_cfirst), dump(out, "first", vs.first);
  fprintf(out, "bw 1 %d\n", vs.bw);
  const int R = atoi(argv[3]), L = atoi(argv[4]);
  // the even split, with its dispatch order on 8 and on 256 compute units
  {
    std::vector<int> ch_ptr, gw_ptr, gw_cf, ch_desc;
    for (int rep = 0; rep < 2; ++rep)  // twice into the same vectors: the outputs are rebuilt, not appended to
      if (!hs::build_chunks_balanced(vs, vi.n_cp, R, L, &ch_ptr, &gw_ptr, &gw_cf, &ch_desc)) {
        fprintf(out, "declined 0\n");
        fclose(out);
        return 0;
      }
    dump(out, "ch_ptr", ch_ptr), dump(out, "gw_ptr", gw_ptr), dump(out, "gw_cf", gw_cf), dump(out, "ch_desc", ch_desc);
    for (int n_cu : {8, 256}) {
      std::vector<int> d = ch_desc;
      hs::order_chunks_by_records(n_cu, &d, int(ch_ptr.size()) - 1);
      dump(out, "ch_desc_cu" + std::to_string(n_cu), d);
    }
  }
  // the pinned pair (greedy fill, pairing by records in k segments) for comparison
  std::vector<int> ch_ptr, gw_ptr, gw_cf, ch_desc;
  if (hs::build_chunks(vs, vi.n_cp, R, L, &ch_ptr, &gw_ptr, &gw_cf, &ch_desc)) {
    dump(out, "greedy_gw_ptr", gw_ptr), dump(out, "greedy_ch_desc", ch_desc);
    hs::order_chunks_for_dispatch(vs, vi.k, 256, &ch_desc, int(ch_ptr.size()) - 1);
    dump(out, "greedy_ch_desc_cu256", ch_desc);
  }
  fclose(out);
  return 0;
}
