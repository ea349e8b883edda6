// tracker.hpp — hs_tracker: the stereo KLT front-end on the device (kernels_klt.hpp) behind its own handle, stream and id generator
// (part of capi.hip: included once, by it). Replaces VisualFrontend::callback / trackForward / trackFeatures / selectFeatures /
// circularInitialization of HyperSLAM's klt.cpp and the OpenCV calls they make. The pyramid, Lucas-Kanade and corner work runs on the GPU;
// the host keeps the per-track bookkeeping of at most max_num_tracks points (statuses, the sort by length, the disc test, ids).
#pragma once

struct hs_tracker {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int w = 0, h = 0;
  hs_tracker_options o{};
  std::string err;
  KltGeom g{};
  size_t level_elems = 0;  // elements of one padded pyramid (all levels)
  // image slots: 0..3 the two stereo pairs of process() (ping-pong), 4..5 the single calls
  DBuf<uint8_t> raw[6], img[6];
  DBuf<short> der[6];
  DBuf<float> eig, disc, fpts[12];
  DBuf<uint8_t> mask, fst[12];
  DBuf<unsigned> max_key;
  DBuf<unsigned long long> keys, sorted;
  DBuf<int> counts;  // [candidate count, corner count]
  DBuf<float> corners;
  // frame state (the previous view of klt.cpp)
  int cur = 0;  // pair of the previous frame: slots 2 cur, 2 cur + 1
  bool has_prev = false;
  double prev_stamp = 0.0;
  std::vector<float> P0, P1;
  std::vector<int64_t> ids;
  std::vector<int32_t> lengths;
  int64_t next_id = 0;
};

namespace {

/// Levels 0..L while each level's width and height exceed the patch (buildOpticalFlowPyramid's reduction of maxLevel), padding patch + 1.
static void klt_geometry(hs_tracker* p) {
  KltGeom& g = p->g;
  g = KltGeom{};
  g.patch = p->o.patch_size, g.pad = p->o.patch_size + 1;
  int w = p->w, h = p->h, n = 1;
  g.w[0] = w, g.h[0] = h;
  while (n <= p->o.num_pyramid_levels) {
    const int w1 = (w + 1) / 2, h1 = (h + 1) / 2;
    if (w1 <= g.patch || h1 <= g.patch) break;
    g.w[n] = w = w1, g.h[n] = h = h1, ++n;
  }
  g.n_levels = n;
  long long off = 0;
  for (int l = 0; l < n; ++l) {
    g.stride[l] = g.w[l] + 2 * g.pad;
    g.off[l] = off;
    off += (long long)g.stride[l] * (g.h[l] + 2 * g.pad);
  }
  p->level_elems = size_t(off);
}

static int klt_alloc(hs_tracker* p) {
  const size_t px = size_t(p->w) * p->h;
  for (int s = 0; s < 6; ++s) {
    HIP_TRY(p->raw[s].reserve(px));
    HIP_TRY(p->img[s].reserve(p->level_elems));
    HIP_TRY(p->der[s].reserve(2 * p->level_elems));
  }
  HIP_TRY(p->eig.reserve(px));
  HIP_TRY(p->mask.reserve(px));
  HIP_TRY(p->keys.reserve(px));
  HIP_TRY(p->sorted.reserve(px));
  HIP_TRY(p->corners.reserve(2 * px));
  HIP_TRY(p->max_key.reserve(1));
  HIP_TRY(p->counts.reserve(2));
  return HS_OK;
}

/// Uploads the images of slots a (and b >= 0) and builds their padded pyramids and derivatives: n_levels + 1 launches.
static int klt_build(hs_tracker* p, int a, const uint8_t* ia, int b, const uint8_t* ib) {
  const size_t px = size_t(p->w) * p->h;
  HIP_TRY(hipMemcpyAsync(p->raw[a].p, ia, px, hipMemcpyHostToDevice, p->stream));
  if (b >= 0) HIP_TRY(hipMemcpyAsync(p->raw[b].p, ib, px, hipMemcpyHostToDevice, p->stream));
  const KltGeom& g = p->g;
  const int bb = b >= 0 ? b : a;
  for (int level = 0; level <= g.n_levels; ++level) {
    int ext_w = 0, ext_h = 0;
    for (int l : {level - 1, level})
      if (l >= 0 && l < g.n_levels) ext_w = std::max(ext_w, g.stride[l]), ext_h = std::max(ext_h, g.h[l] + 2 * g.pad);
    dim3 grid((ext_w + 15) / 16, (ext_h + 15) / 16, b >= 0 ? 2 : 1);
    k_klt_pyramid<<<grid, 256, 0, p->stream>>>(g, level, p->raw[a].p, p->raw[bb].p, p->img[a].p, p->img[bb].p, p->der[a].p, p->der[bb].p, p->w, p->h);
    HIP_TRY(hipGetLastError());
  }
  return HS_OK;
}

static KltPass klt_pass(hs_tracker* p, int I, int J, const float* pts, const float* init, int out, int n) {
  return KltPass{p->img[I].p, p->der[I].p, p->img[J].p, pts, init, p->fpts[out].p, p->fst[out].p, n, 0};
}

/// Up to four independent LK passes in one launch.
static int klt_flow(hs_tracker* p, std::initializer_list<KltPass> passes) {
  KltPasses ps{};
  int np = 0, nmax = 0;
  for (const KltPass& q : passes) ps.p[np++] = q, nmax = std::max(nmax, q.n);
  if (nmax == 0) return HS_OK;
  const double eps2 = p->o.epsilon * p->o.epsilon;
  k_klt_flow<<<dim3((nmax + 3) / 4, np), 256, 0, p->stream>>>(p->g, ps, p->o.max_iterations, eps2, float(p->o.min_eig_threshold));
  HIP_TRY(hipGetLastError());
  return HS_OK;
}

static int klt_reserve_points(hs_tracker* p, int n) {
  for (int i = 0; i < 12; ++i) {
    HIP_TRY(p->fpts[i].reserve(2 * size_t(std::max(n, 1))));
    HIP_TRY(p->fst[i].reserve(size_t(std::max(n, 1))));
  }
  return HS_OK;
}

/// goodFeaturesToTrack on the level-0 image of slot s: corners stay on the device (p->corners), their count is returned in *n (synchronises).
static int klt_good_features(hs_tracker* p, int s, KltMask mask, int max_corners, double quality, double min_distance, int* n) {
  const int w = p->w, h = p->h;
  HIP_TRY(hipMemsetAsync(p->max_key.p, 0, sizeof(unsigned), p->stream));
  HIP_TRY(hipMemsetAsync(p->counts.p, 0, 2 * sizeof(int), p->stream));
  const dim3 grid((w + 15) / 16, (h + 15) / 16);
  k_klt_min_eigen<<<grid, 256, 0, p->stream>>>(p->raw[s].p, w, h, p->eig.p, p->max_key.p, mask);
  HIP_TRY(hipGetLastError());
  k_klt_candidates<<<grid, 256, 0, p->stream>>>(p->eig.p, w, h, p->max_key.p, quality, mask, p->keys.p, p->counts.p);
  HIP_TRY(hipGetLastError());
  const int cap = w * h;
  k_klt_rank<<<(cap + 255) / 256, 256, 0, p->stream>>>(p->keys.p, p->counts.p, p->sorted.p);
  HIP_TRY(hipGetLastError());
  k_klt_select<<<1, 1024, 0, p->stream>>>(p->sorted.p, p->counts.p, w, max_corners, min_distance, p->corners.p, p->counts.p + 1);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(n, p->counts.p + 1, sizeof(int), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipStreamSynchronize(p->stream));
  return HS_OK;
}

static bool klt_contains(const hs_tracker* p, float x, float y) {  // klt.cpp contains(): cvRound, border 1, asymmetric bounds
  const float rx = rintf(x), ry = rintf(y);
  return rx >= 1.f && ry >= 1.f && rx <= float(p->w - 1) && ry < float(p->h - 1);
}
static bool klt_close(const float* a, const float* b, double max_err) {
#pragma clang fp contract(off)
  const float dx = a[0] - b[0], dy = a[1] - b[1];
  return double(std::sqrt(dx * dx + dy * dy)) < max_err;
}

/// trackPoints(A, B, P) per point: status of A -> B (out slot fa), back-check B -> A seeded with P (slot fb), contains, distance.
static bool klt_keep(const hs_tracker* p, const std::vector<uint8_t>& sa, const std::vector<uint8_t>& sb, const std::vector<float>& pb,
                     const std::vector<float>& pts, const std::vector<float>& back, int i) {
  return sa[i] && sb[i] && klt_contains(p, pb[2 * i], pb[2 * i + 1]) && klt_close(&pts[2 * i], &back[2 * i], p->o.max_track_error);
}

static int klt_download(hs_tracker* p, int slot, int n, std::vector<float>* pts, std::vector<uint8_t>* st) {
  pts->resize(2 * size_t(n)), st->resize(size_t(n));
  if (n == 0) return HS_OK;
  HIP_TRY(hipMemcpyAsync(pts->data(), p->fpts[slot].p, 8 * size_t(n), hipMemcpyDeviceToHost, p->stream));
  HIP_TRY(hipMemcpyAsync(st->data(), p->fst[slot].p, size_t(n), hipMemcpyDeviceToHost, p->stream));
  return HS_OK;
}

}  // namespace
