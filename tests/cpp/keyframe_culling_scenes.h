// Shared by tests/cpp/keyframe_culling_facade_test.cpp (CPU, the restated counter) and tests/cpp/keyframe_culling_test.cpp (GPU,
// orbfe_redundant_observations): four small maps of stub objects (culling_stub/), the sequential loop of LocalMapping::KeyFrameCulling
// written again on them, and the comparison of the state orbfe::KeyFrameCullingWith leaves with the state that loop leaves on a
// second copy of the same map: which keyframes are bad or marked mbToBeErased, how often SetBadFlag was called on each, every
// keyframe's MapPoint vector, which MapPoints are bad, every observation list and Observations().
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <map>
#include <memory>
#include <utility>
#include <vector>

#include "KeyFrame.h"
#include "orbfe/KeyFrameCulling.h"

extern "C" int kfcull_ref_counts(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs,
                                 int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level,
                                 int th_obs, int32_t* out_n_mps, int32_t* out_n_redundant);

namespace culling_scenes {

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

#define CHECK(cond)                                                                 \
  do {                                                                              \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

struct Obs {
  KeyFrame* kf;
  int octave;
};

struct Scene {
  std::vector<std::unique_ptr<KeyFrame> > kfs;
  std::vector<std::unique_ptr<MapPoint> > mps;
  std::vector<KeyFrame*> local;      // vpLocalKeyFrames
  KeyFrame* H[4];                    // four helper keyframes outside the local list

  KeyFrame* kf(long unsigned id, bool isLocal = true) {
    kfs.emplace_back(new KeyFrame);
    kfs.back()->mnId = id;
    if (isLocal) local.push_back(kfs.back().get());
    return kfs.back().get();
  }
  void helpers() {
    for (int i = 0; i < 4; i++) H[i] = kf(100 + i, false);
  }
  MapPoint* mp(std::initializer_list<Obs> observers) {
    mps.emplace_back(new MapPoint);
    for (const Obs& o : observers) o.kf->testAddKeyPoint(o.octave, mps.back().get());
    return mps.back().get();
  }
  void many(int n, std::initializer_list<Obs> observers) {
    for (int i = 0; i < n; i++) mp(observers);
  }
  int kfIndex(KeyFrame* p) const {
    for (size_t i = 0; i < kfs.size(); i++)
      if (kfs[i].get() == p) return (int)i;
    return -1;
  }
  int mpIndex(MapPoint* p) const {
    if (!p) return -1;
    for (size_t i = 0; i < mps.size(); i++)
      if (mps[i].get() == p) return (int)i;
    return -2;
  }
  // everything the loop can change, by index
  std::vector<long> state() const {
    std::vector<long> s;
    for (size_t i = 0; i < kfs.size(); i++) {
      KeyFrame* k = kfs[i].get();
      s.push_back(k->isBad());
      s.push_back(k->testToBeErased());
      s.push_back(k->testSetBadFlagCalls);
      for (MapPoint* p : k->GetMapPointMatches()) s.push_back(mpIndex(p));
      s.push_back(-7);
    }
    for (size_t i = 0; i < mps.size(); i++) {
      MapPoint* p = mps[i].get();
      s.push_back(p->isBad());
      s.push_back(p->Observations());
      // (keyed by pointer in the object; by keyframe index here, so that two copies of a map compare equal)
      std::vector<std::pair<int, long> > obs;
      for (const auto& o : p->GetObservations()) obs.push_back(std::make_pair(kfIndex(o.first), (long)o.second));
      std::sort(obs.begin(), obs.end());
      for (const auto& o : obs) { s.push_back(o.first); s.push_back(o.second); }
      s.push_back(-8);
    }
    return s;
  }
  int nBadKeyFrames() const { int n = 0; for (const auto& k : kfs) n += k->isBad(); return n; }
  int nBadMapPoints() const { int n = 0; for (const auto& p : mps) n += p->isBad(); return n; }
};

// (a) nothing is culled: half of every keyframe's MapPoints are redundant; keyframe 1 also holds MapPoints seen by three others
// two levels up, which do not count
inline void sceneA(Scene& S) {
  S.helpers();
  KeyFrame* K[4];
  for (int i = 0; i < 4; i++) K[i] = S.kf(1 + i);
  S.many(6, {{K[0], 0}, {K[1], 0}, {K[2], 1}, {K[3], 0}});
  for (int i = 0; i < 4; i++) S.many(6, {{K[i], 0}, {S.H[0], 0}, {S.H[1], 0}});
  S.many(2, {{K[0], 0}, {S.H[0], 2}, {S.H[1], 2}, {S.H[2], 2}});
}
// (b) a keyframe held by mbNotErase passes the threshold: only mbToBeErased moves
inline void sceneB(Scene& S) {
  S.helpers();
  KeyFrame* B = S.kf(5);
  KeyFrame* F = S.kf(6);
  B->SetNotErase();
  S.many(10, {{B, 0}, {S.H[0], 0}, {S.H[1], 0}, {S.H[2], 0}, {S.H[3], 0}});
  S.many(4, {{F, 0}, {S.H[0], 0}, {S.H[1], 0}});
}
// (c) local = [A, C, D, E].  A is culled (11 of 12 redundant).  C holds 9 MapPoints seen by three helpers (one level up: they
// count) and one seen by A and two helpers: with the counts taken before A went it stands at 10 of 10, above 90 %, afterwards
// that MapPoint has three observations left, is not looked at, and C stands at 9 of 10 = 90 %: not above.  D is culled whenever
// it is counted.  One MapPoint of A, E and a helper goes bad with A and leaves E.
inline void sceneC(Scene& S) {
  S.helpers();
  KeyFrame *A = S.kf(1), *C = S.kf(2), *D = S.kf(3), *E = S.kf(4);
  S.many(10, {{A, 0}, {S.H[0], 0}, {S.H[1], 1}, {S.H[2], 0}, {S.H[3], 0}});
  S.many(9, {{C, 2}, {S.H[0], 3}, {S.H[1], 3}, {S.H[2], 0}});
  S.mp({{C, 0}, {A, 0}, {S.H[0], 0}, {S.H[1], 0}});
  S.many(10, {{D, 1}, {S.H[0], 0}, {S.H[1], 0}, {S.H[2], 2}, {S.H[3], 3}});
  S.many(5, {{E, 0}, {S.H[0], 0}, {S.H[1], 0}});
  S.mp({{A, 0}, {E, 0}, {S.H[0], 0}});
}
// (d) keyframe 0 is in the list and would pass the threshold
inline void sceneD(Scene& S) {
  S.helpers();
  KeyFrame* Z = S.kf(0);
  KeyFrame* G = S.kf(7);
  S.many(10, {{Z, 0}, {S.H[0], 0}, {S.H[1], 0}, {S.H[2], 0}, {S.H[3], 0}});
  S.many(4, {{G, 0}, {S.H[0], 0}, {S.H[1], 0}});
}

// LocalMapping::KeyFrameCulling's loop (reference src/LocalMapping.cc:564-602), written again on the stubs: one keyframe after the
// other, every count read from the objects as they are at that moment.
inline void sequential(const std::vector<KeyFrame*>& vpLocalKeyFrames) {
  for (KeyFrame* pKF : vpLocalKeyFrames) {
    if (pKF->mnId == 0) continue;
    const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
    const int thObs = 3;
    int nRedundantObservations = 0, nMPs = 0;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
      MapPoint* pMP = vpMapPoints[i];
      if (!pMP || pMP->isBad()) continue;
      nMPs++;
      if (pMP->Observations() <= thObs) continue;
      const int scaleLevel = pKF->mvKeysUn[i].octave;
      const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
      int nObs = 0;
      for (const auto& ob : observations) {
        if (ob.first == pKF) continue;
        if (ob.first->mvKeysUn[ob.second].octave <= scaleLevel + 1 && ++nObs >= thObs) break;
      }
      if (nObs >= thObs) nRedundantObservations++;
    }
    if (nRedundantObservations > 0.9 * nMPs) pKF->SetBadFlag();
  }
}

// run(vpLocalKeyFrames, &stats) -> rc is the form under test
template <class Run>
int one(const char* name, void (*build)(Scene&), Run&& run, int calls, int culled, int subjects, int badMapPoints) {
  Scene got, want;
  build(got);
  build(want);
  CHECK(got.state() == want.state());
  orbfe::KeyFrameCullingStats st = {-1, -1, -1};
  const int rc = run(got.local, &st);
  if (rc) { std::printf("FAIL scene %s: rc %d (%s)\n", name, rc, orbfe_last_error()); return 1; }
  sequential(want.local);
  if (got.state() != want.state()) { std::printf("FAIL scene %s: the state differs from the sequential loop's\n", name); return 1; }
  if (st.calls != calls || st.culled != culled || st.subjects != subjects || got.nBadKeyFrames() != culled || got.nBadMapPoints() != badMapPoints) {
    std::printf("FAIL scene %s: calls %d culled %d subjects %d, bad keyframes %d, bad MapPoints %d\n", name, st.calls, st.culled, st.subjects,
                got.nBadKeyFrames(), got.nBadMapPoints());
    return 1;
  }
  std::printf("scene %s: calls %d, culled %d\n", name, st.calls, st.culled);
  return 0;
}

// scene (c) cannot be passed without the recount: with the restated counter alone, C's verdict from the counts taken before A
// went bad differs from its verdict afterwards
inline int stale_and_fresh_verdicts_differ() {
  Scene S;
  sceneC(S);
  std::vector<int32_t> nMPs, nRed;
  CHECK(orbfe::KeyFrameCullingCount(kfcull_ref_counts, S.local, 0, nMPs, nRed) == ORBFE_OK && nMPs.size() == 4);
  CHECK(nMPs[0] == 12 && nRed[0] == 11);
  CHECK(nMPs[1] == 10 && nRed[1] == 10 && nRed[1] > 0.9 * nMPs[1]);          // stale: cull
  S.local[0]->SetBadFlag();
  CHECK(S.local[0]->isBad());
  CHECK(orbfe::KeyFrameCullingCount(kfcull_ref_counts, S.local, 1, nMPs, nRed) == ORBFE_OK && nMPs.size() == 3);
  CHECK(nMPs[0] == 10 && nRed[0] == 9 && !(nRed[0] > 0.9 * nMPs[0]));        // fresh: keep
  CHECK(nMPs[1] == 10 && nRed[1] == 10);
  CHECK(nMPs[2] == 5 && nRed[2] == 0);                                         // E has lost the MapPoint that went bad with A
  return 0;
}

template <class Run>
int all(Run&& run) {
  if (stale_and_fresh_verdicts_differ()) return 1;
  if (one("a", sceneA, run, 1, 0, 4, 0)) return 1;
  if (one("b", sceneB, run, 1, 0, 2, 0)) return 1;
  if (one("c", sceneC, run, 3, 2, 4 + 3 + 1, 1)) return 1;
  if (one("d", sceneD, run, 1, 0, 2, 0)) return 1;
  {   // (b) and (d) again, by name: the verdict reached the held keyframe, and never reached keyframe 0
    Scene S;
    sceneB(S);
    CHECK(run(S.local, nullptr) == ORBFE_OK && S.local[0]->testToBeErased() && !S.local[0]->isBad() && S.local[0]->testSetBadFlagCalls == 1);
    Scene T;
    sceneD(T);
    CHECK(run(T.local, nullptr) == ORBFE_OK && T.local[0]->testSetBadFlagCalls == 0 && !T.local[0]->isBad());
  }
  {   // refusals that change nothing: a keyframe named twice, an octave outside a byte
    Scene S, same;
    sceneC(S);
    sceneC(same);
    std::vector<KeyFrame*> twice = S.local;
    twice.push_back(S.local[1]);
    orbfe::KeyFrameCullingStats st = {-1, -1, -1};
    CHECK(run(twice, &st) == ORBFE_ERR_INVALID && st.calls == 0 && S.state() == same.state());
    S.H[3]->mvKeysUn[0].octave = 256;
    same.H[3]->mvKeysUn[0].octave = 256;
    CHECK(run(S.local, &st) == ORBFE_ERR_INVALID && st.calls == 0 && st.culled == 0 && S.state() == same.state());
    S.H[3]->mvKeysUn[0].octave = -1;
    CHECK(run(S.local, &st) == ORBFE_ERR_INVALID && st.calls == 0);
    std::vector<KeyFrame*> none;
    CHECK(run(none, &st) == ORBFE_OK && st.calls == 0 && st.subjects == 0);
  }
  return 0;
}

}  // namespace culling_scenes
