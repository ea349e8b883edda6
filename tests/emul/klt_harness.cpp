// klt_harness.cpp — TEST INFRASTRUCTURE: the front-end kernels of hyperslam_amd/csrc/kernels_klt.hpp compiled for the host through
// tests/emul/hip/hip_runtime.h and driven on small images by tests/test_klt_emulated.py, which compares with tests/klt_numpy.py.
//   klt_harness MODE IN OUT      MODE = pyr | eig | gft | flow; IN: int32 header + arrays (see read_* below); OUT: the results, raw.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "hip/hip_runtime.h"

thread_local dim3 threadIdx;
thread_local unsigned hs_emul::exchange_count = 0;
dim3 blockIdx, blockDim, gridDim;

// wave / bit intrinsics the front-end kernels use beyond what the shared emulation header provides
template <class T>
inline T __shfl(T v, int src_lane) { return hs_emul::wave_exchange(v, src_lane); }
inline unsigned __float_as_uint(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
inline float __uint_as_float(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
inline int atomicAdd(int* p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
inline unsigned atomicMax(unsigned* p, unsigned v) {
  unsigned old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (old < v && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {
  }
  return old;
}

#include "../../hyperslam_amd/csrc/host_structure.hpp"
#include "../../hyperslam_amd/csrc/kernels_common.hpp"
#include "../../hyperslam_amd/csrc/kernels_klt.hpp"

using namespace hs;

static std::vector<char> slurp(const char* path) {
  std::vector<char> b;
  FILE* f = std::fopen(path, "rb");
  if (!f) return b;
  char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) b.insert(b.end(), buf, buf + n);
  std::fclose(f);
  return b;
}

struct Reader {
  const char* p;
  template <class T>
  T get() {
    T v;
    std::memcpy(&v, p, sizeof(T));
    p += sizeof(T);
    return v;
  }
  template <class T>
  std::vector<T> arr(size_t n) {
    std::vector<T> v(n);
    std::memcpy(v.data(), p, n * sizeof(T));
    p += n * sizeof(T);
    return v;
  }
};

static KltGeom geometry(int w, int h, int patch, int max_level, size_t* elems) {
  KltGeom g{};
  g.patch = patch, g.pad = patch + 1;
  int n = 1;
  g.w[0] = w, g.h[0] = h;
  while (n <= max_level) {
    const int w1 = (w + 1) / 2, h1 = (h + 1) / 2;
    if (w1 <= patch || h1 <= patch) break;
    g.w[n] = w = w1, g.h[n] = h = h1, ++n;
  }
  g.n_levels = n;
  long long off = 0;
  for (int l = 0; l < n; ++l) g.stride[l] = g.w[l] + 2 * g.pad, g.off[l] = off, off += (long long)g.stride[l] * (g.h[l] + 2 * g.pad);
  *elems = size_t(off);
  return g;
}

static void build(const KltGeom& g, size_t elems, const std::vector<uint8_t>& raw, int w, int h, std::vector<uint8_t>* img, std::vector<short>* der) {
  img->assign(elems, 0), der->assign(2 * elems, 0);
  for (int level = 0; level <= g.n_levels; ++level) {
    int ew = 0, eh = 0;
    for (int l : {level - 1, level})
      if (l >= 0 && l < g.n_levels) ew = std::max(ew, g.stride[l]), eh = std::max(eh, g.h[l] + 2 * g.pad);
    uint8_t* ip = img->data();
    short* dp = der->data();
    const uint8_t* rp = raw.data();
    hs_emul::launch(dim3((ew + 15) / 16, (eh + 15) / 16, 1), dim3(256), 0, [&] { k_klt_pyramid(g, level, rp, rp, ip, ip, dp, dp, w, h); });
  }
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const std::string mode = argv[1];
  std::vector<char> in = slurp(argv[2]);
  if (in.empty()) return 3;
  Reader r{in.data()};
  FILE* out = std::fopen(argv[3], "wb");
  if (!out) return 4;
  const int w = r.get<int>(), h = r.get<int>();
  if (mode == "pyr") {
    const int patch = r.get<int>(), levels = r.get<int>();
    std::vector<uint8_t> raw = r.arr<uint8_t>(size_t(w) * h), img;
    std::vector<short> der;
    size_t elems = 0;
    const KltGeom g = geometry(w, h, patch, levels, &elems);
    build(g, elems, raw, w, h, &img, &der);
    std::fwrite(&g.n_levels, 4, 1, out);
    for (int l = 0; l < g.n_levels; ++l)
      for (int y = 0; y < g.h[l]; ++y) std::fwrite(img.data() + g.off[l] + size_t(y + g.pad) * g.stride[l] + g.pad, 1, g.w[l], out);
    for (int l = 0; l < g.n_levels; ++l)
      for (int y = 0; y < g.h[l]; ++y) std::fwrite(der.data() + 2 * (g.off[l] + size_t(y + g.pad) * g.stride[l] + g.pad), 2, 2 * size_t(g.w[l]), out);
  } else if (mode == "eig" || mode == "gft") {
    std::vector<uint8_t> raw = r.arr<uint8_t>(size_t(w) * h);
    std::vector<float> eig(size_t(w) * h);
    const dim3 grid((w + 15) / 16, (h + 15) / 16);
    if (mode == "eig") {
      hs_emul::launch(grid, dim3(256), 0, [&] { k_klt_min_eigen(raw.data(), w, h, eig.data(), nullptr, KltMask{}); });
      std::fwrite(eig.data(), 4, eig.size(), out);
    } else {
      const int has_mask = r.get<int>(), max_corners = r.get<int>();
      const double quality = r.get<double>(), min_distance = r.get<double>();
      std::vector<uint8_t> mask = has_mask ? r.arr<uint8_t>(size_t(w) * h) : std::vector<uint8_t>();
      KltMask m{};
      if (has_mask) m.img = mask.data();
      unsigned max_key = 0;
      int counts[2] = {0, 0};
      std::vector<unsigned long long> keys(size_t(w) * h), sorted(size_t(w) * h);
      std::vector<float> corners(2 * size_t(w) * h);
      hs_emul::launch(grid, dim3(256), 0, [&] { k_klt_min_eigen(raw.data(), w, h, eig.data(), &max_key, m); });
      hs_emul::launch(grid, dim3(256), 0, [&] { k_klt_candidates(eig.data(), w, h, &max_key, quality, m, keys.data(), counts); });
      hs_emul::launch(dim3((counts[0] + 255) / 256), dim3(256), 0, [&] { k_klt_rank(keys.data(), counts, sorted.data()); });
      hs_emul::launch(dim3(1), dim3(1024), 0, [&] { k_klt_select(sorted.data(), counts, w, max_corners, min_distance, corners.data(), counts + 1); });
      std::fwrite(counts + 1, 4, 1, out);
      std::fwrite(corners.data(), 4, 2 * size_t(counts[1]), out);
    }
  } else if (mode == "flow") {
    const int patch = r.get<int>(), levels = r.get<int>(), n = r.get<int>(), has_init = r.get<int>();
    std::vector<uint8_t> raw0 = r.arr<uint8_t>(size_t(w) * h), raw1 = r.arr<uint8_t>(size_t(w) * h), img0, img1;
    std::vector<float> pts = r.arr<float>(2 * size_t(n)), init = has_init ? r.arr<float>(2 * size_t(n)) : std::vector<float>(), res(2 * size_t(n));
    std::vector<uint8_t> st(n);
    std::vector<short> der0, der1;
    size_t elems = 0;
    const KltGeom g = geometry(w, h, patch, levels, &elems);
    build(g, elems, raw0, w, h, &img0, &der0);
    build(g, elems, raw1, w, h, &img1, &der1);
    KltPasses ps{};
    ps.p[0] = KltPass{img0.data(), der0.data(), img1.data(), pts.data(), has_init ? init.data() : nullptr, res.data(), st.data(), n, 0};
    hs_emul::launch(dim3((n + 3) / 4, 1), dim3(256), 0, [&] { k_klt_flow(g, ps, 30, 0.01 * 0.01, 1e-4f); });
    std::fwrite(res.data(), 4, res.size(), out);
    std::fwrite(st.data(), 1, st.size(), out);
  } else {
    return 5;
  }
  std::fclose(out);
  return 0;
}
