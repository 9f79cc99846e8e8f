// source_projection_test.cpp -- the two frame-rate searches whose projection loops run on the GPU, driven through
// include/orbfe/orb_shim.hpp's SearchByProjectionLastFrame / SearchByProjectionKeyFrame the way Tracking.cc drives them, every
// call compared with the CPU oracle's whole-function restatements (oracle/orb_oracle_pose.h: orc_sbp_frame, orc_sbp_keyframe):
//
//   per frame      Frame::Frame: ExtractORB -> the frame's resident copy (from the extractor's arena)
//   frame 0        the initial map: a MapPoint for about half of the keypoints
//   frames >= 1    Tracking::TrackWithMotionModel: SearchByProjection(Cur, Last, 15); on frame 2 the 2*th call follows on the
//                  same frame (Tracking.cc:596-614) and must send no row; on frame 1 both searches run a second time through a
//                  context whose frame cache is off (their host-projection form) and must equal the oracle as well
//                  Tracking::Relocalization's SearchByProjection(Cur, pKF, sAlreadyFound, 10, 100) against frame 0 as KeyFrame
//                  (Tracking.cc:1456) on a copy of the frame's matches
//                  Tracking::SearchLocalPoints through the same context: its MapPoints share the rows
//   between        a few MapPoints move, a few descriptors are recomputed, new MapPoints join, outliers are marked
//
// Scene as in tracking_sequence_test.cpp: a textured plane at depth Z, frame k = frame 0 shifted by k * (dx, dy) px.
//
//   usage: source_projection_test <dir> [time]     (time: frames 0 and 1 only, then the medians of 200 blocking calls of the
//          old and the new last-frame search through the facade)     reads <dir>/meta.txt (W H NFRAMES NFEATURES DX DY), <dir>/f%03d.gray
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "orb_oracle_pose.h"
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
  int id = 0;
  float pos[3] = {0, 0, 0}, normal[3] = {0, 0, -1}, minD = 0, maxD = 0;
  unsigned char desc[32];
  bool bad = false, mbTrackInView = false, plCandidato = false;
  int nObs = 0, mnTrackScaleLevel = 0, nVisible = 0;
  unsigned long mnLastFrameSeen = ~0ul;
  float mTrackProjX = 0, mTrackProjY = 0, mTrackViewCos = 1;
  MatF GetWorldPos() { MatF m; m.rows = 3; m.cols = 1; memcpy(m.v, pos, 12); return m; }
  MatF GetDescriptor() { MatF m; m.data = desc; m.step = 32; m.rows = 1; return m; }
  float GetMinDistanceInvariance() { return 0.8f * minD; }
  float GetMaxDistanceInvariance() { return 1.2f * maxD; }
  int PredictScale(const float& currentDist, const float& logScaleFactor) {
    const float ratio = maxD / currentDist;
    return std::ceil(std::log(ratio) / logScaleFactor);
  }
  bool isBad() { return bad; }
  int Observations() { return nObs; }
  void IncreaseVisible() { nVisible++; }
};
struct Frame {
  unsigned long mnId = 0;
  int N = 0;
  std::vector<KeyPoint> mvKeys, mvKeysUn;
  std::vector<unsigned char> descStore;
  MatF mDescriptors, mTcw;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  std::vector<float> mvScaleFactors;
  float fx = 0, fy = 0, cx = 0, cy = 0, mfLogScaleFactor = 0;
  static float mnMinX, mnMaxX, mnMinY, mnMaxY;
  void bind() { mDescriptors.data = descStore.data(); mDescriptors.step = 32; mDescriptors.rows = N; }
  MatF GetCameraCenter() const { MatF m; m.rows = 3; m.cols = 1; for (int r = 0; r < 3; r++) m.v[r] = -mTcw.v[4 * r + 3]; return m; }   // R = I
  Frame() {}
  Frame(const Frame& o) { *this = o; }
  Frame& operator=(const Frame& o) {
    mnId = o.mnId; N = o.N; mvKeys = o.mvKeys; mvKeysUn = o.mvKeysUn; descStore = o.descStore; mvpMapPoints = o.mvpMapPoints;
    mvbOutlier = o.mvbOutlier; mvScaleFactors = o.mvScaleFactors; fx = o.fx; fy = o.fy; cx = o.cx; cy = o.cy;
    mfLogScaleFactor = o.mfLogScaleFactor; mTcw = o.mTcw;
    bind();
    return *this;
  }
};
float Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY;
struct KeyFrame {   // KeyFrame::KeyFrame(Frame&, ...) copies the features (KeyFrame.cc:37-60)
  std::vector<KeyPoint> mvKeys, mvKeysUn;
  std::vector<unsigned char> descStore;
  MatF mDescriptors;
  std::vector<MapPoint*> matches;
  float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
  explicit KeyFrame(const Frame& F) : mvKeys(F.mvKeys), mvKeysUn(F.mvKeysUn), descStore(F.descStore), matches(F.mvpMapPoints) {
    mDescriptors.data = descStore.data(); mDescriptors.step = 32; mDescriptors.rows = F.N;
    mnMinX = Frame::mnMinX; mnMaxX = Frame::mnMaxX; mnMinY = Frame::mnMinY; mnMaxY = Frame::mnMaxY;
  }
  std::vector<MapPoint*> GetMapPointMatches() { return matches; }
};

struct Rng {
  unsigned long long s;
  explicit Rng(unsigned long long seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
  unsigned long long next() { s += 0x9E3779B97F4A7C15ull; unsigned long long z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
  double uni(double a, double b) { return a + (b - a) * uni(); }
  int below(int n) { return (int)(next() % (unsigned long long)n); }
};

static std::vector<unsigned char> readFile(const std::string& p) {
  FILE* f = fopen(p.c_str(), "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", p.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<unsigned char> v(n);
  if (fread(v.data(), 1, n, f) != (size_t)n) exit(2);
  fclose(f);
  return v;
}

static int failures = 0, checks = 0;
static void expect(bool ok, const char* what, int frame, long got, long want) {
  checks++;
  if (!ok) {
    failures++;
    printf("FAIL frame %d: %s (got %ld, want %ld)\n", frame, what, got, want);
  }
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  const std::string dir = argv[1];
  const bool timing = argc > 2 && std::string(argv[2]) == "time";
  int W = 0, H = 0, NF = 0, nfeat = 0, dxs = 0, dys = 0;
  {
    FILE* f = fopen((dir + "/meta.txt").c_str(), "r");
    if (!f || fscanf(f, "%d %d %d %d %d %d", &W, &H, &NF, &nfeat, &dxs, &dys) != 6) return 2;
    fclose(f);
  }
  const float fx = 500.f, fy = 498.f, cx = W * 0.5f + 0.5f, cy = H * 0.5f - 0.25f, Z = 5.f;
  const int device = orbfe::detail::defaultDevice();
  orbfe::Extractor extractor(nfeat, 1.2f, 8, 20, 7, device);
  orbfe::MatcherContext ctx(device);
  orbfe::MatcherContext ctxOff(device);   // frame cache off: the two searches take their host-projection form (checked at frame 1)
  ctxOff.setFrameCacheCapacity(0);
  const std::vector<float> sf = extractor.GetScaleFactors();
  const float logSf = std::log(1.2f);
  Frame::mnMinX = 0; Frame::mnMaxX = (float)W; Frame::mnMinY = 0; Frame::mnMaxY = (float)H;
  const float bounds[4] = {Frame::mnMinX, Frame::mnMaxX, Frame::mnMinY, Frame::mnMaxY};
  auto geometry = [](MapPoint* p, float* pos, float* normal, float& minRaw, float& maxRaw) {
    memcpy(pos, p->pos, 12);
    memcpy(normal, p->normal, 12);
    minRaw = p->minD;
    maxRaw = p->maxD;
  };

  Rng rng(1234);
  std::vector<MapPoint*> map;   // owned; ids = index
  Frame last;
  KeyFrame* kf = nullptr;
  int lastCalls = 0, kfCalls = 0, totalLast = 0, totalKf = 0, totalLocal = 0, pruned = 0;

  auto poseOf = [&](int k, float ex, float ey, Frame& F) {   // Tcw = [I | t_k + error]
    F.mTcw = MatF();
    F.mTcw.rows = F.mTcw.cols = 4;
    F.mTcw.v[0] = F.mTcw.v[5] = F.mTcw.v[10] = F.mTcw.v[15] = 1.f;
    F.mTcw.v[3] = (float)(k * dxs) * Z / fx + ex;
    F.mTcw.v[7] = (float)(k * dys) * Z / fy + ey;
  };
  auto newPoint = [&](const Frame& F, int idx) {   // a MapPoint triangulated at keypoint idx of F (on the plane)
    MapPoint* p = new MapPoint();
    p->id = (int)map.size();
    const KeyPoint& k = F.mvKeysUn[idx];
    p->pos[0] = (k.x - cx) / fx * Z - F.mTcw.v[3];
    p->pos[1] = (k.y - cy) / fy * Z - F.mTcw.v[7];
    p->pos[2] = Z;
    const float PO[3] = {p->pos[0] + F.mTcw.v[3], p->pos[1] + F.mTcw.v[7], p->pos[2]};
    const float d = std::sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2]);
    for (int c = 0; c < 3; c++) p->normal[c] = PO[c] / d;
    p->maxD = d * sf[k.octave < 6 ? k.octave : 6];   // MapPoint::UpdateNormalAndDepth (MapPoint.cc:315-355)
    p->minD = p->maxD / sf[7];
    memcpy(p->desc, &F.descStore[(size_t)idx * 32], 32);
    p->nObs = rng.below(4);
    map.push_back(p);
    return p;
  };
  std::vector<float> tpos, tmin, tmax, tnrm;
  std::vector<uint8_t> tdesc, tbad;
  std::vector<int32_t> tobs, tidx;
  auto table = [&](OrcPoints& P) {
    const size_t M = map.size();
    tpos.resize(3 * M); tnrm.assign(3 * M, 0.f); tmin.resize(M); tmax.resize(M); tdesc.resize(32 * M); tbad.resize(M); tobs.resize(M);
    tidx.assign(M, -1);
    for (size_t i = 0; i < M; i++) {
      memcpy(&tpos[3 * i], map[i]->pos, 12); memcpy(&tdesc[32 * i], map[i]->desc, 32);
      tmin[i] = map[i]->minD; tmax[i] = map[i]->maxD; tbad[i] = map[i]->bad; tobs[i] = map[i]->nObs;
    }
    P.M = (int)M; P.pos = tpos.data(); P.normal = tnrm.data(); P.mfMinDistance = tmin.data(); P.mfMaxDistance = tmax.data();
    P.desc = tdesc.data(); P.bad = tbad.data(); P.nObs = tobs.data(); P.idxInKF = tidx.data();
  };

  size_t changedSinceLastFrame = 0;
  for (int k = 0; k < NF; k++) {
    char name[64];
    snprintf(name, sizeof name, "/f%03d.gray", k);
    std::vector<unsigned char> img = readFile(dir + name);
    Frame cur;
    cur.mnId = (unsigned long)k;
    cur.fx = fx; cur.fy = fy; cur.cx = cx; cur.cy = cy; cur.mfLogScaleFactor = logSf;
    cur.mvScaleFactors = sf;
    extractor.extract(img.data(), H, W, (size_t)W, cur.mvKeys, cur.descStore);
    cur.N = (int)cur.mvKeys.size();
    cur.mvKeysUn = cur.mvKeys;   // no distortion (Frame.cc:288-292)
    cur.bind();
    cur.mvpMapPoints.assign(cur.N, nullptr);
    cur.mvbOutlier.assign(cur.N, false);
    poseOf(k, 0.f, 0.f, cur);
    expect(ctx.resident(cur, 0) != nullptr, "the frame is resident", k, 0, 1);   // taken from the extractor's arena
    if (k == 0) {
      for (int i = 0; i < cur.N; i++)
        if (rng.uni() < 0.5) { cur.mvpMapPoints[i] = newPoint(cur, i); cur.mvpMapPoints[i]->nObs = 1 + rng.below(3); }
      last = Frame(cur);
      kf = new KeyFrame(cur);
      continue;
    }
    poseOf(k, (float)rng.uni(-0.012, 0.012), (float)rng.uni(-0.012, 0.012), cur);   // the motion model's prediction
    OrcView cv;
    cv.kpsUn = reinterpret_cast<const OrcKp*>(cur.mvKeysUn.data()); cv.desc = cur.descStore.data(); cv.n = cur.N;
    memcpy(cv.bounds, bounds, sizeof bounds);
    cv.fx = fx; cv.fy = fy; cv.cx = cx; cv.cy = cy; cv.scaleFactors = sf.data(); cv.invLevelSigma2 = sf.data(); cv.nlevels = 8; cv.logScaleFactor = logSf;
    std::vector<int32_t> lastIds(last.N), curIds(cur.N, -1);
    std::vector<uint8_t> lastOut(last.N);
    for (int i = 0; i < last.N; i++) { lastIds[i] = last.mvpMapPoints[i] ? last.mvpMapPoints[i]->id : -1; lastOut[i] = last.mvbOutlier[i]; }
    if (timing) {   // tools/source_projection_bench.py: median of blocking calls through the facade, old route and new
      auto med = [&](auto&& fn) {
        std::vector<double> t;
        for (int it = 0; it < 220; it++) {
          std::fill(cur.mvpMapPoints.begin(), cur.mvpMapPoints.end(), static_cast<MapPoint*>(nullptr));
          const auto t0 = std::chrono::steady_clock::now();
          fn();
          if (it >= 20) t.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
        }
        std::sort(t.begin(), t.end());
        return t[t.size() / 2];
      };
      int nOld = 0, nNew = 0;
      const double tOld = med([&] { nOld = orbfe::SearchByProjection(ctx, true, cur, last, 15.f); });
      const double tNew = med([&] { nNew = orbfe::SearchByProjectionLastFrame(ctx, true, cur, last, 15.f, geometry); });
      int nsrc = 0;
      for (int i = 0; i < last.N; i++) nsrc += last.mvpMapPoints[i] != nullptr;
      printf("timing {\"facade_last_frame_host_projection_us\": %.2f, \"facade_last_frame_gpu_projection_us\": %.2f, \"n_src\": %d, "
             "\"sources_with_mappoint\": %d, \"nmatches_old\": %d, \"nmatches_new\": %d}\n", tOld, tNew, last.N, nsrc, nOld, nNew);
      delete kf;
      for (MapPoint* p : map) delete p;
      return nOld == nNew ? 0 : 1;
    }
    // ---- Tracking::TrackWithMotionModel -----------------------------------------------------------------------------------
    const size_t rowsBefore = ctx.localMapRowsSent();
    for (int attempt = 0; attempt < (k == 2 ? 2 : 1); attempt++) {
      const float th = attempt ? 30.f : 15.f;
      std::fill(cur.mvpMapPoints.begin(), cur.mvpMapPoints.end(), static_cast<MapPoint*>(nullptr));
      std::fill(curIds.begin(), curIds.end(), -1);
      OrcPoints P;
      table(P);
      const int want = orc_sbp_frame(&cv, cur.mTcw.v, reinterpret_cast<const OrcKp*>(last.mvKeys.data()),
                                     reinterpret_cast<const OrcKp*>(last.mvKeysUn.data()), last.N, lastIds.data(), lastOut.data(), &P,
                                     curIds.data(), th, 1);
      const int wantNoOri = orc_sbp_frame(&cv, cur.mTcw.v, reinterpret_cast<const OrcKp*>(last.mvKeys.data()),
                                          reinterpret_cast<const OrcKp*>(last.mvKeysUn.data()), last.N, lastIds.data(), lastOut.data(), &P,
                                          std::vector<int32_t>(cur.N, -1).data(), th, 0);
      pruned += wantNoOri - want;
      const size_t sentBefore = ctx.localMapRowsSent();
      const int got = orbfe::SearchByProjectionLastFrame(ctx, true, cur, last, th, geometry);
      bool same = got == want;
      for (int i = 0; i < cur.N && same; i++) same = (cur.mvpMapPoints[i] ? cur.mvpMapPoints[i]->id : -1) == curIds[i];
      expect(same, attempt ? "SearchByProjectionLastFrame(Cur, Last, 2*th)" : "SearchByProjectionLastFrame(Cur, Last, th)", k, got, want);
      if (attempt) expect(ctx.localMapRowsSent() == sentBefore, "the 2*th call on the same frame sends no row", k, (long)ctx.localMapRowsSent(), (long)sentBefore);
      if (k == 1) {   // the same call through the context without a frame cache, on a copy of the frame's matches
        const std::vector<MapPoint*> keep = cur.mvpMapPoints;
        std::fill(cur.mvpMapPoints.begin(), cur.mvpMapPoints.end(), static_cast<MapPoint*>(nullptr));
        const int gotOff = orbfe::SearchByProjectionLastFrame(ctxOff, true, cur, last, th, geometry);
        bool sameOff = gotOff == want;
        for (int i = 0; i < cur.N && sameOff; i++) sameOff = (cur.mvpMapPoints[i] ? cur.mvpMapPoints[i]->id : -1) == curIds[i];
        expect(sameOff, "SearchByProjectionLastFrame(Cur, Last, th), frame cache off", k, gotOff, want);
        cur.mvpMapPoints = keep;
      }
      lastCalls++;
      totalLast += got;
    }
    // ---- Tracking::Relocalization's projection search against frame 0 as KeyFrame, on a copy of the frame's matches ---------
    {
      const std::vector<MapPoint*> keep = cur.mvpMapPoints;
      std::set<MapPoint*> sFound;
      for (int i = 0; i < cur.N; i++)
        if (i % 3 == 0) cur.mvpMapPoints[i] = nullptr;   // (PoseOptimization dropped some)
        else if (cur.mvpMapPoints[i]) sFound.insert(cur.mvpMapPoints[i]);
      std::vector<int32_t> kfIds(kf->matches.size()), ids(cur.N);
      for (size_t i = 0; i < kf->matches.size(); i++) kfIds[i] = kf->matches[i] ? kf->matches[i]->id : -1;
      for (int i = 0; i < cur.N; i++) ids[i] = cur.mvpMapPoints[i] ? cur.mvpMapPoints[i]->id : -1;
      std::vector<uint8_t> already(map.size(), 0);
      for (MapPoint* p : sFound) already[p->id] = 1;
      OrcPoints P;
      table(P);
      const int want = orc_sbp_keyframe(&cv, cur.mTcw.v, reinterpret_cast<const OrcKp*>(kf->mvKeysUn.data()), (int)kfIds.size(), kfIds.data(),
                                        already.data(), &P, ids.data(), 10.f, 100, 1);
      const std::vector<MapPoint*> before = cur.mvpMapPoints;
      const int got = orbfe::SearchByProjectionKeyFrame(ctx, true, cur, kf, sFound, 10.f, 100, geometry);
      bool same = got == want;
      for (int i = 0; i < cur.N && same; i++) same = (cur.mvpMapPoints[i] ? cur.mvpMapPoints[i]->id : -1) == ids[i];
      expect(same, "SearchByProjectionKeyFrame(Cur, pKF, sAlreadyFound, 10, 100)", k, got, want);
      if (k == 1) {   // the same call through the context without a frame cache, from the same matches
        cur.mvpMapPoints = before;
        const int gotOff = orbfe::SearchByProjectionKeyFrame(ctxOff, true, cur, kf, sFound, 10.f, 100, geometry);
        bool sameOff = gotOff == want;
        for (int i = 0; i < cur.N && sameOff; i++) sameOff = (cur.mvpMapPoints[i] ? cur.mvpMapPoints[i]->id : -1) == ids[i];
        expect(sameOff, "SearchByProjectionKeyFrame(Cur, pKF, sAlreadyFound, 10, 100), frame cache off", k, gotOff, want);
      }
      kfCalls++;
      totalKf += got;
      cur.mvpMapPoints = keep;
    }
    // ---- Tracking::SearchLocalPoints: the local map = every MapPoint, through the same rows ------------------------------------
    {
      for (auto& p : cur.mvpMapPoints)
        if (p) { p->IncreaseVisible(); p->mnLastFrameSeen = cur.mnId; p->mbTrackInView = false; }   // Tracking.cc:784-796
      totalLocal += orbfe::SearchLocalPoints(ctx, cur, map, 1.f, 0.5f, geometry);
    }
    // rows: one per MapPoint whoever asks; after frame 1 only MapPoints that are new or changed are sent
    expect(ctx.localMapRows() <= map.size(), "a MapPoint keeps one row", k, (long)ctx.localMapRows(), (long)map.size());
    if (k >= 2)
      expect(ctx.localMapRowsSent() - rowsBefore <= changedSinceLastFrame, "rows sent this frame <= MapPoints changed or created", k,
             (long)(ctx.localMapRowsSent() - rowsBefore), (long)changedSinceLastFrame);
    // ---- between frames ----------------------------------------------------------------------------------------------------
    changedSinceLastFrame = 0;
    std::set<MapPoint*> touched;
    for (int i = 0; i < cur.N; i++)
      if (cur.mvpMapPoints[i] && rng.uni() < 0.05) cur.mvbOutlier[i] = true;          // pose optimisation marks outliers
    for (size_t j = 0; j < map.size(); j++) {
      if (rng.uni() < 0.03) { for (int c = 0; c < 2; c++) map[j]->pos[c] += 0.0005f; touched.insert(map[j]); }      // local BA
      if (rng.uni() < 0.03) { map[j]->desc[rng.below(32)] ^= (unsigned char)(1 << rng.below(8)); touched.insert(map[j]); }
    }
    poseOf(k, 0.f, 0.f, cur);
    int added = 0;
    for (int i = 0; i < cur.N && added < 100; i++)
      if (!cur.mvpMapPoints[i] && rng.uni() < 0.3) { cur.mvpMapPoints[i] = newPoint(cur, i); touched.insert(cur.mvpMapPoints[i]); added++; }
    changedSinceLastFrame = touched.size();
    for (int i = 0; i < cur.N; i++)
      if (cur.mvpMapPoints[i] && !cur.mvbOutlier[i] && rng.uni() < 0.3) cur.mvpMapPoints[i]->nObs++;
    last = Frame(cur);
  }
  printf("frames %d last_calls %d kf_calls %d matches_last %d matches_kf %d matches_local %d pruned %d\n", NF, lastCalls, kfCalls, totalLast,
         totalKf, totalLocal, pruned);
  printf("resident uploads %zu from_extract %zu rows %zu rows_sent %zu map %zu\n", ctx.residentUploads(), ctx.residentFromExtract(),
         ctx.localMapRows(), ctx.localMapRowsSent(), map.size());
  expect(ctx.residentUploads() == 0, "a frame's features were uploaded although the extractor held them", -1, (long)ctx.residentUploads(), 0);
  expect((int)ctx.residentFromExtract() == NF, "frames built from the extractor's arena", -1, (long)ctx.residentFromExtract(), NF);
  expect(totalLast > 25 * lastCalls && totalKf > 0, "the searches found matches", -1, totalLast, totalKf);
  delete kf;
  for (MapPoint* p : map) delete p;
  printf("%s %d checks, %d failures\n", failures ? "FAIL" : "PASS", checks, failures);
  return failures ? 1 : 0;
}
