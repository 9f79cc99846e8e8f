// local_map_test.cpp -- Tracking::SearchLocalPoints (src/Tracking.cc:781-825) driven through include/orbfe/orb_shim.hpp's
// SearchLocalPoints on minimal Frame / MapPoint structs of its own, over a short tracking-shaped sequence:
//
//   per frame   F.mvpMapPoints starts with a few MapPoints already matched (TrackWithMotionModel); the loop of
//               Tracking.cc:784-796 marks them (mnLastFrameSeen = mnId, mbTrackInView = false, IncreaseVisible), then
//               SearchLocalPoints projects and searches the local map (th = 1, frame 3: 5 as after a relocalisation)
//   between     MapPoints move, normals and depth ranges change, descriptors are recomputed, some go bad, new ones join,
//               the local map vector is rebuilt in another order (Tracking::UpdateLocalPoints)
//
// Every call's inputs and outputs are written to <dir>/f<k>.*; tests/local_map_facade.py checks them against the reference
// restatement (tests/cpp/is_in_frustum_ref.cpp) and the CPU oracle's SearchByProjection.
//
//   usage: local_map_test <dir>      reads <dir>/meta.txt (W H N NMP NFRAMES), kps.bin, desc.bin, sf.bin, mp.bin, cam.bin
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "orbfe/orb_shim.hpp"

struct KeyPoint { float x, y, size, angle, response; int octave, class_id; };  // cv::KeyPoint layout
struct MatF {   // the parts of cv::Mat the shim touches
  float v[16] = {0};
  int rows = 0, cols = 0;
  unsigned char* data = nullptr;
  size_t step = 0;
  template <class T> T at(int r, int c) const { return (T)v[r * cols + c]; }
};
struct MapPoint {
  float pos[3], normal[3], minD = 0, maxD = 0;   // protected in os1 (MapPoint.h): handed over by the geometry functor
  unsigned char desc[32];
  bool bad = false, mbTrackInView = false, plCandidato = false;
  int nObs = 0, mnTrackScaleLevel = -99, nVisible = 0;
  unsigned long mnLastFrameSeen = 0;
  float mTrackProjX = -1, mTrackProjY = -1, mTrackViewCos = -1;
  MatF GetDescriptor() { MatF m; m.data = desc; m.step = 32; m.rows = 1; return m; }
  bool isBad() { return bad; }
  int Observations() { return nObs; }
  void IncreaseVisible() { nVisible++; }
};
struct Frame {
  unsigned long mnId = 0;
  std::vector<KeyPoint> mvKeys, mvKeysUn;
  std::vector<unsigned char> descStore;
  MatF mDescriptors, mTcw, Ow;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<float> mvScaleFactors;
  float fx = 0, fy = 0, cx = 0, cy = 0, mfLogScaleFactor = 0;
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;
  MatF GetCameraCenter() { return Ow; }
};
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;

template <class T>
static std::vector<T> readAll(const std::string& path, size_t n) {
  std::vector<T> v(n);
  FILE* f = fopen(path.c_str(), "rb");
  if (!f || fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "cannot read %s\n", path.c_str()); exit(2); }
  fclose(f);
  return v;
}
template <class T>
static void writeAll(const std::string& path, const std::vector<T>& v) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) exit(3);
  fwrite(v.data(), sizeof(T), v.size(), f);
  fclose(f);
}

static unsigned long long g_rng = 88172645463325252ull;
static unsigned rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (unsigned)(g_rng >> 11); }

int main(int argc, char** argv) {
  if (argc < 2) return 1;
  const std::string dir = argv[1];
  int W, H, N, NMP, NF;
  FILE* mf = fopen((dir + "/meta.txt").c_str(), "r");
  if (!mf || fscanf(mf, "%d %d %d %d %d", &W, &H, &N, &NMP, &NF) != 5) return 2;
  fclose(mf);
  const auto kps = readAll<KeyPoint>(dir + "/kps.bin", N);
  const auto desc = readAll<unsigned char>(dir + "/desc.bin", (size_t)N * 32);
  const auto sf = readAll<float>(dir + "/sf.bin", 8);
  const auto mpRec = readAll<float>(dir + "/mp.bin", (size_t)NMP * 16);     // pos3 normal3 min max desc(32 bytes)
  const auto camRec = readAll<float>(dir + "/cam.bin", (size_t)NF * 20);    // Rcw9 tcw3 Ow3 fx fy cx cy logScaleFactor

  std::vector<MapPoint*> all;
  auto addMP = [&](int k) {
    MapPoint* p = new MapPoint();
    memcpy(p->pos, &mpRec[16 * (size_t)k], 12);
    memcpy(p->normal, &mpRec[16 * (size_t)k + 3], 12);
    p->minD = mpRec[16 * (size_t)k + 6];
    p->maxD = mpRec[16 * (size_t)k + 7];
    memcpy(p->desc, &mpRec[16 * (size_t)k + 8], 32);
    p->nObs = (rnd() % 10) ? 2 : 0;
    p->plCandidato = (rnd() % 20) == 0;
    all.push_back(p);
  };
  for (int k = 0; k < NMP - 100; k++) addMP(k);   // the last 100 records join later

  orbfe::MatcherContext ctx(0);
  auto geometry = [](MapPoint* p, float* pos, float* normal, float& minRaw, float& maxRaw) {
    memcpy(pos, p->pos, 12);
    memcpy(normal, p->normal, 12);
    minRaw = p->minD;
    maxRaw = p->maxD;
  };
  Frame::mnMinX = 0; Frame::mnMaxX = (float)W; Frame::mnMinY = 0; Frame::mnMaxY = (float)H;
  for (int fi = 0; fi < NF; fi++) {
    // between frames: the map changes
    if (fi == 1) for (int k = 0; k < 60; k++) { MapPoint* p = all[rnd() % all.size()]; for (int c = 0; c < 3; c++) p->pos[c] *= 1.002f; }
    if (fi == 2) for (int k = 0; k < 60; k++) { MapPoint* p = all[rnd() % all.size()]; p->desc[rnd() % 32] ^= 0x5a; }
    if (fi == 2) for (int k = 0; k < 40; k++) { MapPoint* p = all[rnd() % all.size()]; p->maxD *= 1.3f; p->minD *= 0.9f; }
    if (fi == 3) for (int k = 0; k < 30; k++) all[rnd() % all.size()]->bad = true;
    if (fi == 3) for (int k = NMP - 100; k < NMP; k++) addMP(k);
    if (fi == 4) for (int k = 0; k < 60; k++) { MapPoint* p = all[rnd() % all.size()]; for (int c = 0; c < 3; c++) p->normal[c] = -p->normal[c]; }
    std::vector<MapPoint*> local;   // Tracking::UpdateLocalPoints: a new vector, another order (bad ones stay in it here)
    for (size_t k = 0; k < all.size(); k++) local.push_back(all[(k * 7919 + fi * 131) % all.size()]);

    Frame F;
    F.mnId = (unsigned long)(fi + 1);
    F.mvKeys = kps; F.mvKeysUn = kps;
    F.descStore = desc;
    F.mDescriptors.data = F.descStore.data(); F.mDescriptors.step = 32; F.mDescriptors.rows = N;
    F.mvScaleFactors = sf;
    const float* cr = &camRec[20 * (size_t)fi];
    F.mTcw.rows = 4; F.mTcw.cols = 4;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) F.mTcw.v[4 * r + c] = cr[3 * r + c]; F.mTcw.v[4 * r + 3] = cr[9 + r]; }
    F.mTcw.v[15] = 1.f;
    F.Ow.rows = 3; F.Ow.cols = 1; memcpy(F.Ow.v, cr + 12, 12);
    F.fx = cr[15]; F.fy = cr[16]; F.cx = cr[17]; F.cy = cr[18]; F.mfLogScaleFactor = cr[19];
    F.mvpMapPoints.assign(N, nullptr);
    for (int k = 0; k < 40; k++) {   // matched by the motion model already
      MapPoint* p = all[rnd() % all.size()];
      if (p->bad || p->nObs == 0) continue;
      F.mvpMapPoints[rnd() % N] = p;
    }
    // Tracking.cc:784-796
    for (auto& p : F.mvpMapPoints)
      if (p) {
        if (p->isBad()) p = nullptr;
        else { p->IncreaseVisible(); p->mnLastFrameSeen = F.mnId; p->mbTrackInView = false; }
      }
    // snapshot of the inputs, per local MapPoint: record (pos3 normal3 min max, desc), flags (2 bad, 4 candidato, 8 observed,
    // 16 skip); occupancy; the MapPoint fields before the call
    const size_t n = local.size();
    std::vector<float> rec(16 * n);
    std::vector<unsigned char> fl(n), occ(N);
    std::vector<int> visBefore(n);
    std::vector<MapPoint*> before = F.mvpMapPoints;
    for (size_t i = 0; i < n; i++) {
      MapPoint* p = local[i];
      memcpy(&rec[16 * i], p->pos, 12); memcpy(&rec[16 * i + 3], p->normal, 12);
      rec[16 * i + 6] = p->minD; rec[16 * i + 7] = p->maxD; memcpy(&rec[16 * i + 8], p->desc, 32);
      fl[i] = (unsigned char)((p->bad ? 2 : 0) | (p->plCandidato ? 4 : 0) | (p->nObs > 0 ? 8 : 0) | (p->mnLastFrameSeen == F.mnId ? 16 : 0));
      visBefore[i] = p->nVisible;
      p->mbTrackInView = false; p->mTrackProjX = p->mTrackProjY = p->mTrackViewCos = -1; p->mnTrackScaleLevel = -99;
    }
    for (int i = 0; i < N; i++) occ[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0;
    const float th = fi == 3 ? 5.f : 1.f;
    const int nm = orbfe::SearchLocalPoints(ctx, F, local, th, 0.5f, geometry);
    // outputs: per local MapPoint (mbTrackInView, X, Y, level, viewCos, visible increments); per keypoint the index into
    // `local` of a newly assigned MapPoint (-1: unchanged); nmatches, th
    std::vector<float> out(6 * n);
    for (size_t i = 0; i < n; i++) {
      MapPoint* p = local[i];
      out[6 * i] = p->mbTrackInView ? 1.f : 0.f;
      out[6 * i + 1] = p->mTrackProjX; out[6 * i + 2] = p->mTrackProjY;
      out[6 * i + 3] = (float)p->mnTrackScaleLevel; out[6 * i + 4] = p->mTrackViewCos;
      out[6 * i + 5] = (float)(p->nVisible - visBefore[i]);
    }
    std::vector<int> assigned(N, -1);
    for (int i = 0; i < N; i++)
      if (F.mvpMapPoints[i] != before[i]) {
        int last = -1;   // SearchByProjection writes vpMapPoints[i]: the LAST entry of `local` holding that MapPoint
        for (size_t k = 0; k < n; k++) if (local[k] == F.mvpMapPoints[i]) last = (int)k;
        assigned[i] = last;
      }
    const std::string pre = dir + "/f" + std::to_string(fi);
    writeAll(pre + ".rec", rec); writeAll(pre + ".flags", fl); writeAll(pre + ".occ", occ);
    writeAll(pre + ".out", out); writeAll(pre + ".assigned", assigned);
    writeAll(pre + ".nm", std::vector<float>{(float)nm, th, (float)n});
  }
  printf("local map rows %zu, rows sent %zu\n", ctx.localMapRows(), ctx.localMapRowsSent());
  for (MapPoint* p : all) delete p;
  return 0;
}
