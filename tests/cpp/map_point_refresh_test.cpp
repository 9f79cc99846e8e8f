// include/orbfe/MapPointRefresh.h over a small stub map (tests/cpp/mprefresh_stub): 3 keyframes (one of them bad), 20
// MapPoints (one bad, one without observations, one whose reference keyframe is not among its observations).  The stub
// objects' fields after orbfe::RefreshMapPoints must equal, byte for byte, what the restatement
// tests/cpp/map_point_refresh_ref.cpp computes from arrays this program builds on its own; MapPoints the reference functions
// return early for must keep their fields.
//   default             links liborbfe.so (tests/test_gpu_map_point_refresh.py); the table's rows are compared too
//   -DMPR_HOST_BACKEND  the three C calls the facade makes are defined HERE on top of the restatement, so that the facade's
//                       marshalling runs on a machine without a GPU (tests/test_map_point_refresh.py)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "MapPoint.h"
#include "KeyFrame.h"
#include "orbfe/MapPointRefresh.h"

extern "C" int mpr_refresh_rows(uint8_t* table, int what, int n_kf, const uint8_t* const* kf_desc, const int32_t* const* kf_oct,
                                const float* kf_Ow, const float* scale_factors, int nlevels, int n_mp, const int32_t* rows,
                                const int32_t* obs_offsets, const int32_t* obs_kf, const int32_t* obs_kp, const uint8_t* obs_flags,
                                const int32_t* ref_kf, const int32_t* ref_kp, int32_t* best_obs, float* normal, float* min_raw,
                                float* max_raw);

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

namespace {
constexpr int kKF = 3, kMP = 20, kKP = 80, kLevels = 8, kCap = 32;
uint32_t g_state = 12345u;
uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }
float rndf(float lo, float hi) { return lo + (hi - lo) * (float)(rnd() & 0xffff) / 65536.0f; }
std::vector<int32_t> g_oct[kKF];
}  // namespace

#ifdef MPR_HOST_BACKEND
struct orbfe_frame { const uint8_t* desc; const int32_t* oct; int n; };
struct orbfe_local_map { std::vector<uint8_t> table; int capacity; };
struct orbfe_matcher { int unused; };
extern "C" {
int orbfe_local_map_set_rows(orbfe_local_map* map, int n, const int32_t* rows, const float* pos, const float* normal, const float* min_raw,
                             const float* max_raw, const uint8_t* desc) {
  for (int i = 0; i < n; i++) {
    if (rows[i] < 0 || rows[i] >= map->capacity) return ORBFE_ERR_INVALID;
    float* r = reinterpret_cast<float*>(map->table.data() + 64 * (size_t)rows[i]);
    if (pos) std::memcpy(r, pos + 3 * (size_t)i, 12);
    if (normal) std::memcpy(r + 3, normal + 3 * (size_t)i, 12);
    if (min_raw) r[6] = min_raw[i];
    if (max_raw) r[7] = max_raw[i];
    if (desc) std::memcpy(r + 8, desc + 32 * (size_t)i, 32);
  }
  return ORBFE_OK;
}
int orbfe_local_map_refresh_rows(orbfe_matcher*, orbfe_local_map* map, int what, int n_kf, orbfe_frame* const* kf_frames, const float* kf_Ow,
                                 const float* scale_factors, int nlevels, int n_mp, const int32_t* rows, const int32_t* obs_offsets,
                                 const int32_t* obs_kf, const int32_t* obs_kp, const uint8_t* obs_flags, const int32_t* ref_kf,
                                 const int32_t* ref_kp, int32_t* best_obs, float* normal, float* min_raw, float* max_raw) {
  std::vector<const uint8_t*> d(n_kf, nullptr);
  std::vector<const int32_t*> o(n_kf, nullptr);
  for (int s = 0; s < n_kf; s++)
    if (kf_frames[s]) { d[s] = kf_frames[s]->desc; o[s] = kf_frames[s]->oct; }
  const int rc = mpr_refresh_rows(map->table.data(), what, n_kf, d.data(), o.data(), kf_Ow, scale_factors, nlevels, n_mp, rows, obs_offsets,
                                  obs_kf, obs_kp, obs_flags, ref_kf, ref_kp, best_obs, normal, min_raw, max_raw);
  return rc < 0 ? ORBFE_ERR_INVALID : ORBFE_OK;
}
int orbfe_local_map_download_rows(orbfe_local_map* map, int n, const int32_t* rows, uint8_t* out) {
  for (int i = 0; i < n; i++) std::memcpy(out + 64 * (size_t)i, map->table.data() + 64 * (size_t)rows[i], 64);
  return ORBFE_OK;
}
const char* orbfe_last_error(void) { return "host back end"; }
}
#endif

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)
#define OK(call)                                                                                     \
  do {                                                                                               \
    const int rc_ = (call);                                                                          \
    if (rc_) { std::printf("FAIL %s:%d %s -> %d (%s)\n", __FILE__, __LINE__, #call, rc_, orbfe_last_error()); return 1; } \
  } while (0)

int main() {
  // the map
  static KeyFrame kf[kKF];   // one array: std::map<KeyFrame*, size_t> iterates in index order
  static MapPoint mp[kMP];
  for (int s = 0; s < kKF; s++) {
    kf[s].mnId = s;
    kf[s].mnScaleLevels = kLevels;
    float f = 1.0f;
    for (int l = 0; l < kLevels; l++) { kf[s].mvScaleFactors.push_back(f); f *= 1.2f; }
    kf[s].mDescriptors = cv::Mat(kKP, 32, CV_8U);
    for (int i = 0; i < kKP * 32; i++) kf[s].mDescriptors.data[i] = (unsigned char)rnd();
    g_oct[s].resize(kKP);
    for (int i = 0; i < kKP; i++) g_oct[s][i] = (int32_t)(rnd() % kLevels);
    kf[s].Ow = cv::Mat(3, 1, CV_32F);
    for (int k = 0; k < 3; k++) kf[s].Ow.at<float>(k) = rndf(-1.0f, 1.0f);
    kf[s].bad = s == 2;
  }
  std::vector<MapPoint*> vp;
  std::vector<int32_t> rows;
  for (int p = 0; p < kMP; p++) {
    const float pos[3] = {rndf(-4.0f, 4.0f), rndf(-3.0f, 3.0f), rndf(2.0f, 9.0f)};
    unsigned pick = 1u + rnd() % 7u;               // a non-empty subset of the keyframes
    if (p == 5) pick = 0;                          // no observation
    if (p == 6) pick = 4;                          // observed by the bad keyframe only
    if (p == 7) pick = 2;                          // its reference keyframe (0) does not observe it
    const int ref = (p == 7) ? 0 : ((pick & 1u) ? 0 : ((pick & 2u) ? 1 : 0));
    mp[p].testInit(pos, &kf[ref], p == 9);
    for (int s = 0; s < kKF; s++)
      if (pick & (1u << s)) mp[p].testObserve(&kf[s], rnd() % kKP);
    vp.push_back(&mp[p]);
    rows.push_back((int32_t)((p * 7 + 3) % kCap));
  }

  // what the two reference functions leave, from arrays built here
  std::vector<uint8_t> table(64 * (size_t)kCap, 0);
  std::vector<int32_t> eRows, eOffs(1, 0), eKf, eKp, eRefKf, eRefKp, eOf;
  std::vector<uint8_t> eFl;
  for (int p = 0; p < kMP; p++) {
    if (mp[p].isBad()) continue;
    const auto obs = mp[p].GetObservations();
    if (obs.empty()) continue;
    for (const auto& kv : obs) {
      eKf.push_back((int32_t)(kv.first - kf));
      eKp.push_back((int32_t)kv.second);
      eFl.push_back(kv.first->isBad() ? 1 : 0);
    }
    KeyFrame* r = mp[p].GetReferenceKeyFrame();
    eRefKf.push_back((int32_t)(r - kf));
    eRefKp.push_back(obs.count(r) ? (int32_t)obs.at(r) : 0);
    eOffs.push_back((int32_t)eKf.size());
    eRows.push_back(rows[p]);
    eOf.push_back(p);
    const cv::Mat P = mp[p].GetWorldPos();
    std::memcpy(table.data() + 64 * (size_t)rows[p], P.data, 12);
  }
  const uint8_t* eDesc[kKF];
  const int32_t* eOct[kKF];
  float eOw[3 * kKF];
  for (int s = 0; s < kKF; s++) {
    eDesc[s] = kf[s].mDescriptors.data;
    eOct[s] = g_oct[s].data();
    std::memcpy(eOw + 3 * s, kf[s].Ow.data, 12);
  }
  const int ne = (int)eRows.size();
  std::vector<int32_t> eBest(ne);
  CHECK(ne == kMP - 2);
  CHECK(mpr_refresh_rows(table.data(), 3, kKF, eDesc, eOct, eOw, kf[0].mvScaleFactors.data(), kLevels, ne, eRows.data(), eOffs.data(), eKf.data(),
                         eKp.data(), eFl.data(), eRefKf.data(), eRefKp.data(), eBest.data(), nullptr, nullptr, nullptr) == 0);

  // the back end
  orbfe_matcher* m = nullptr;
  orbfe_local_map* map = nullptr;
  orbfe_frame* fr[kKF] = {nullptr, nullptr, nullptr};
#ifdef MPR_HOST_BACKEND
  orbfe_matcher hm{0};
  orbfe_local_map hmap{std::vector<uint8_t>(64 * (size_t)kCap, 0), kCap};
  orbfe_frame hf[kKF];
  m = &hm;
  map = &hmap;
  for (int s = 0; s < kKF; s++) { hf[s] = orbfe_frame{kf[s].mDescriptors.data, g_oct[s].data(), kKP}; fr[s] = &hf[s]; }
#else
  OK(orbfe_matcher_create(0, &m));
  OK(orbfe_local_map_create(m, kCap, &map));
  const float bounds[4] = {0.0f, 640.0f, 0.0f, 480.0f};
  for (int s = 0; s < kKF; s++) {
    std::vector<OrbfeKeyPoint> kps(kKP);
    for (int i = 0; i < kKP; i++) {
      kps[i] = OrbfeKeyPoint{};
      kps[i].x = rndf(1.0f, 639.0f); kps[i].y = rndf(1.0f, 479.0f);
      kps[i].size = 31.0f; kps[i].angle = rndf(0.0f, 359.0f); kps[i].octave = g_oct[s][i]; kps[i].class_id = -1;
    }
    OK(orbfe_frame_create(m, kps.data(), kf[s].mDescriptors.data, kKP, bounds, &fr[s]));
  }
#endif
  int askedForBad = 0;
  auto frameOf = [&](KeyFrame* pKF) {
    if (pKF->isBad()) askedForBad++;
    return fr[pKF - kf];
  };
  OK(orbfe::RefreshMapPoints(m, map, vp, rows, frameOf));
  CHECK(askedForBad == 0);   // a bad keyframe that is nobody's reference needs no resident copy

  // the objects
  int e = 0, chosen = 0, expected = 0;
  for (int i = 0; i < ne; i++) expected += eBest[i] >= 0;
  CHECK(eBest[6 - 1] == -1 && expected >= ne / 2 && expected < ne);   // MapPoint 6 (entry 5: MapPoint 5 is left out) is seen by the bad keyframe only
  for (int p = 0; p < kMP; p++) {
    const cv::Mat d = mp[p].GetDescriptor(), nv = mp[p].GetNormal();
    if (e < ne && eOf[e] == p) {
      const uint8_t* row = table.data() + 64 * (size_t)rows[p];
      if (eBest[e] >= 0) { CHECK(std::memcmp(d.data, row + 32, 32) == 0); chosen++; }
      else for (int k = 0; k < 32; k++) CHECK(d.data[k] == 0xA5);
      CHECK(std::memcmp(nv.data, row + 12, 12) == 0);
      const float mn = mp[p].testMin(), mx = mp[p].testMax();
      CHECK(std::memcmp(&mn, row + 24, 4) == 0 && std::memcmp(&mx, row + 28, 4) == 0);
      CHECK(mx > 0.0f && mn > 0.0f && mn < mx);
      e++;
    } else {   // bad, or never observed: both functions return at once
      for (int k = 0; k < 32; k++) CHECK(d.data[k] == 0xA5);
      for (int k = 0; k < 3; k++) CHECK(nv.at<float>(k) == -7.0f);
      CHECK(mp[p].testMin() == -1.0f && mp[p].testMax() == -2.0f);
    }
  }
  CHECK(e == ne && chosen == expected);

  // the table
  std::vector<uint8_t> got(64 * (size_t)ne);
  OK(orbfe_local_map_download_rows(map, ne, eRows.data(), got.data()));
  for (int i = 0; i < ne; i++) CHECK(std::memcmp(got.data() + 64 * (size_t)i, table.data() + 64 * (size_t)eRows[i], 64) == 0);

#ifndef MPR_HOST_BACKEND
  for (int s = 0; s < kKF; s++) orbfe_frame_destroy(fr[s]);
  orbfe_local_map_destroy(map);
  orbfe_matcher_destroy(m);
#endif
  std::printf("PASS\n");
  return 0;
}
