// keyframe_projection_test.cpp -- orb_shim.hpp's SearchByProjectionScw / FuseKeyFrame / FuseScw / SearchBySim3Device (the
// keyframe-side searches with their projection loops on the GPU, orbfe_search_projected_keyframe_frame) against the oracle's
// whole-function restatements (oracle/orb_oracle_pose.h), on facade_pose_test.cpp's mock model and seeded scenes: the
// stand-in Frame / KeyFrame / MapPoint types, the scene generator and the oracle's flat tables are that file's, taken as they
// are (its main() is compiled under another name and not called).
//   SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th)  ORBmatcher.cc:285-398
//   Fuse(KeyFrame*, vpMapPoints, th)                             ORBmatcher.cc:806-939
//   Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint)           ORBmatcher.cc:941-1064
//   SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th)     ORBmatcher.cc:1066-1290
// Each scene is searched twice, by the existing host-projection template on one copy of the model and by the new template
// on another; both must equal the oracle.  Then all four run once more with the frame cache off, where the new templates are
// the existing ones: same counts, same oracle comparison.  Prints one line per function, a statistics line, and PASS / FAIL; exit code 0 iff
// every comparison is exact.
//   build: g++ -std=c++17 -O1 -ffp-contract=off -Iinclude -Ioracle tests/cpp/keyframe_projection_test.cpp os1_amd/liborbfe.so
//          oracle/liborb_oracle.so
#define main facade_pose_test_main
#include "facade_pose_test.cpp"
#undef main

namespace {

// the integrator's functor: MapPoint fields the device table holds (raw mfMinDistance / mfMaxDistance)
struct Geometry {
  void operator()(MapPoint* p, float* pos, float* normal, float& minRaw, float& maxRaw) const {
    memcpy(pos, p->pos, 12);
    memcpy(normal, p->normal, 12);
    minRaw = p->mfMinDistance;
    maxRaw = p->mfMaxDistance;
  }
};

// searches into one KeyFrame (facade_pose_test.cpp's sections 3-5); returns the function's result or -1
int oneKeyFrame(orbfe::MatcherContext& ctx, unsigned long long seed, int which, float th, bool fused) {
  Rng r(seed * 10 + 4 + which);
  KeyFrame kf;
  makeView(r, kf, 1600);
  const float scale = which == 1 ? 1.f : 1.35f;    // Fuse(KF, points) uses the keyframe's own pose, the others a Sim3
  float T[16];
  makePose(r, scale, T);
  setTcw(kf, T);
  if (which == 1) setOw(kf, 1.f);
  const int M = 2600, E = 500;   // candidates (more than one 2 048-query chunk of the bookkeeping kernel), points in the keyframe
  std::vector<MapPoint> mp(M + E);
  std::vector<MapPoint*> pts;
  for (int i = 0; i < M + E; i++) { mp[i].id = i; mp[i].kf = &kf; }
  for (int i = 0; i < E; i++) {
    const int k = r.below(kf.N);
    makePoint(r, mp[M + i], kf, k, T, scale);
    if (kf.mvpMapPoints[k]) continue;
    kf.mvpMapPoints[k] = &mp[M + i];
    mp[M + i].idxInKF = k;
    mp[M + i].nObs = 1 + r.below(5);
  }
  for (int i = 0; i < M; i++) {
    makePoint(r, mp[i], kf, r.below(kf.N), T, scale);
    pts.push_back(&mp[i]);
  }
  if (which == 1) { for (int i = 0; i < 40; i++) pts[r.below(M)] = nullptr; }
  {   // points already in the keyframe, each at most once (vpMapPoints holds distinct points)
    std::set<int> used;
    for (int i = 0; i < 60; i++) { const int e = r.below(E); if (used.insert(e).second) pts.push_back(&mp[M + e]); }
  }
  Table tab(mp);
  OrcView kv = viewOf(kf);
  std::vector<int32_t> ids = idsOf(pts);
  Geometry geometry;
  bool ok = false;
  int got = -1, want = -1;
  if (which == 0) {
    std::vector<MapPoint*> vpMatched = kf.mvpMapPoints;
    std::vector<int32_t> m = idsOf(vpMatched);
    want = orc_sbp_scw(&kv, T, ids.data(), (int)ids.size(), &tab.P, m.data(), (int)th);
    got = fused ? orbfe::SearchByProjectionScw(ctx, &kf, kf.mTcw, pts, vpMatched, (int)th, geometry)
                : orbfe::SearchByProjection(ctx, &kf, kf.mTcw, pts, vpMatched, (int)th);
    ok = got == want && idsOf(vpMatched) == m && want > 100;
  } else if (which == 1) {
    std::vector<int32_t> slot = idsOf(kf.mvpMapPoints);
    want = orc_fuse(&kv, T, ids.data(), (int)ids.size(), &tab.P, slot.data(), th);
    got = fused ? orbfe::FuseKeyFrame(ctx, &kf, pts, th, geometry) : orbfe::Fuse(ctx, &kf, pts, th);
    ok = got == want && idsOf(kf.mvpMapPoints) == slot && tab.sameState(mp) && want > 100;
  } else {
    std::vector<int32_t> slot = idsOf(kf.mvpMapPoints), rep(ids.size(), -1);
    std::vector<MapPoint*> vpReplacePoint(pts.size(), nullptr);
    want = orc_fuse_scw(&kv, T, ids.data(), (int)ids.size(), &tab.P, slot.data(), th, rep.data());
    got = fused ? orbfe::FuseScw(ctx, &kf, kf.mTcw, pts, th, vpReplacePoint, geometry) : orbfe::Fuse(ctx, &kf, kf.mTcw, pts, th, vpReplacePoint);
    ok = got == want && idsOf(kf.mvpMapPoints) == slot && idsOf(vpReplacePoint) == rep && tab.sameState(mp) && want > 100;
  }
  static const char* const names[3][2] = {{"SearchByProjection(KeyFrame, Scw, ...)", "SearchByProjectionScw"},
                                          {"Fuse(KeyFrame, vpMapPoints, th)", "FuseKeyFrame"},
                                          {"Fuse(KeyFrame, Scw, ...)", "FuseScw"}};
  report(names[which][fused ? 1 : 0], ok, got, want, (int)ids.size());
  return ok ? got : -1;
}

// facade_pose_test.cpp's section 6, with a Sim3 scale of s12
int sim3(orbfe::MatcherContext& ctx, unsigned long long seed, float s12, float th, bool fused) {
  Rng r(seed * 10 + 8);
  KeyFrame kf1, kf2;
  makeView(r, kf1, 1500);
  makeView(r, kf2, 1500);
  float T1[16], T2[16];
  makePose(r, 1.f, T1);
  makePose(r, 1.f, T2);
  setTcw(kf1, T1);
  setTcw(kf2, T2);
  // the two keyframes see the same points; the Sim3 between the cameras is the true relative pose scaled by s12 (the
  // projections do not move, the distances and with them the predicted levels do)
  float R12[9], t12[3];
  {
    double R1[9], R2[9], t1[3], t2[3];
    for (int i = 0; i < 3; i++) { for (int j = 0; j < 3; j++) { R1[3 * i + j] = T1[4 * i + j]; R2[3 * i + j] = T2[4 * i + j]; } t1[i] = T1[4 * i + 3]; t2[i] = T2[4 * i + 3]; }
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) { double s = 0; for (int k = 0; k < 3; k++) s += R1[3 * i + k] * R2[3 * j + k]; R12[3 * i + j] = (float)s; }   // R1 R2^T
    for (int i = 0; i < 3; i++) { double s = t1[i]; for (int k = 0; k < 3; k++) s -= (double)R12[3 * i + k] * t2[k]; t12[i] = (float)(s * s12); }
  }
  const int M = 1200;
  std::vector<MapPoint> mp(M), twin(M);
  for (int i = 0; i < M; i++) {
    mp[i].id = i;
    mp[i].kf = &kf2;
    const int k2 = r.below(kf2.N);
    // predicted levels stay inside the pyramid from both cameras and under the scale (the reference indexes mvScaleFactors unchecked)
    kf2.mvKeys[k2].octave = kf2.mvKeysUn[k2].octave = 2 + kf2.mvKeysUn[k2].octave % 2;
    makePoint(r, mp[i], kf2, k2, T2, 1.f);
    twin[i] = mp[i];
    twin[i].id = M + i;
    double Xc[3];
    for (int a = 0; a < 3; a++) Xc[a] = (double)T1[4 * a] * mp[i].pos[0] + (double)T1[4 * a + 1] * mp[i].pos[1] + (double)T1[4 * a + 2] * mp[i].pos[2] + T1[4 * a + 3];
    const int k1 = r.below(kf1.N);
    if (Xc[2] > 0.5 && !kf1.mvpMapPoints[k1] && !kf2.mvpMapPoints[k2]) {
      const double u = kf1.fx * Xc[0] / Xc[2] + kf1.cx, v = kf1.fy * Xc[1] / Xc[2] + kf1.cy;
      if (u > 15 && u < W - 15 && v > 15 && v < H - 15) {
        kf1.mvKeys[k1].x = kf1.mvKeysUn[k1].x = (float)(u + r.uni(-1, 1));
        kf1.mvKeys[k1].y = kf1.mvKeysUn[k1].y = (float)(v + r.uni(-1, 1));
        kf1.mvKeys[k1].octave = kf1.mvKeysUn[k1].octave = kf2.mvKeysUn[k2].octave;
        memcpy(&kf1.descStore[(size_t)k1 * 32], mp[i].desc, 32);
        kf1.mvpMapPoints[k1] = &mp[i];
        if (r.uni() < 0.9) { kf2.mvpMapPoints[k2] = &twin[i]; twin[i].idxInKF = k2; }
      }
    }
  }
  std::vector<MapPoint*> vpMatches12(kf1.N, nullptr);
  for (int k = 0; k < 60; k++) {
    const int i1 = r.below(kf1.N);
    if (kf1.mvpMapPoints[i1]) vpMatches12[i1] = &twin[kf1.mvpMapPoints[i1]->id];
  }
  std::vector<MapPoint> all(mp);
  all.insert(all.end(), twin.begin(), twin.end());
  Table tab(all);
  OrcView v1 = viewOf(kf1), v2 = viewOf(kf2);
  std::vector<int32_t> mp1 = idsOf(kf1.mvpMapPoints), mp2 = idsOf(kf2.mvpMapPoints), m12 = idsOf(vpMatches12);
  const int want = orc_search_by_sim3(&v1, T1, mp1.data(), &v2, T2, mp2.data(), &tab.P, m12.data(), s12, R12, t12, th);
  MatF R12m, t12m;
  R12m.rows = R12m.cols = 3; memcpy(R12m.v, R12, 36);
  t12m.rows = 3; t12m.cols = 1; memcpy(t12m.v, t12, 12);
  Geometry geometry;
  const int got = fused ? orbfe::SearchBySim3Device(ctx, &kf1, &kf2, vpMatches12, s12, R12m, t12m, th, geometry)
                        : orbfe::SearchBySim3(ctx, &kf1, &kf2, vpMatches12, s12, R12m, t12m, th);
  const bool ok = got == want && idsOf(vpMatches12) == m12 && want > 30;
  report(fused ? "SearchBySim3Device" : "SearchBySim3", ok, got, want, M);
  return ok ? got : -1;
}

}  // namespace

int main(int argc, char** argv) {
  const unsigned long long seed = argc > 1 ? strtoull(argv[1], nullptr, 10) : 7;
  orbfe::MatcherContext ctx;
  const float ths[3] = {10.f, 3.0f, 4.0f};
  int total[4] = {0, 0, 0, 0};
  for (int which = 0; which < 3; which++) {
    const int a = oneKeyFrame(ctx, seed, which, ths[which], false);
    const int b = oneKeyFrame(ctx, seed, which, ths[which], true);
    if (a != b) failures++;
    total[which] = b;
  }
  const size_t rowsOnce = ctx.localMapRowsSent();
  // the same scenes again (new objects at new addresses or the same: the rows are keyed by address and compared by content)
  for (int which = 0; which < 3; which++)
    if (oneKeyFrame(ctx, seed + 1, which, ths[which], true) < 0) failures++;
  const float scales[2] = {1.0f, 1.1f};
  int sim3Found[2] = {0, 0};
  for (int k = 0; k < 2; k++) {
    const int a = sim3(ctx, seed, scales[k], 7.5f, false);
    const int b = sim3(ctx, seed, scales[k], 7.5f, true);
    if (a != b || b < 0) failures++;
    sim3Found[k] = b;
    total[3] += b;
  }
  // with the frame cache off the new templates are the existing functions: the same counts, and the oracle comparisons
  // inside oneKeyFrame / sim3 hold again
  ctx.setFrameCacheCapacity(0);
  for (int which = 0; which < 3; which++)
    if (oneKeyFrame(ctx, seed, which, ths[which], true) != total[which]) failures++;
  for (int k = 0; k < 2; k++)
    if (sim3(ctx, seed, scales[k], 7.5f, true) != sim3Found[k]) failures++;
  printf("sbp_scw %d fuse %d fuse_scw %d sim3 %d rows_sent %d\n", total[0], total[1], total[2], total[3], (int)rowsOnce);
  printf("%s\n", failures ? "FAIL" : "PASS");
  return failures ? 1 : 0;
}
