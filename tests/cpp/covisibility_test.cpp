// include/orbfe/Covisibility.h over a stub map shaped like a small one (tests/cpp/covis_stub): 40 keyframes of 200 keypoint
// entries each, MapPoints with 2 to 12 observations in neighbouring keyframes.  Among them: a keyframe with ten MapPoints only
// (nobody reaches the threshold 15: the maximum rule), one without MapPoints (an empty counter), a bad one (AddConnection and
// the final assignment refuse it), keyframe 0 (never given a parent), a MapPoint named twice by one keyframe, and MapPoints
// that are bad, plCandidato or plLejano.
//
// Two identical worlds are built.  World A gets the WHOLE reference function, written again below (KeyFrame.cc:303-402), called
// keyframe by keyframe; world B gets one orbfe::UpdateConnectionsBatch.  Every keyframe's mConnectedKeyFrameWeights, ordered
// lists, parent, first-connection flag and children must then agree (pointers compared as indices).  Twice:
//   map load    observations are added keyframe by keyframe and each keyframe is updated right after its own (Osmap.cpp:569-579),
//               in an order that is not pointer order; B adds all observations first and passes limitToPredecessors = true
//   loop close  all observations are there; 30 of the 40 keyframes are updated, the other ten observe from outside the vector
// and orbfe::CountObservers against the loop of Tracking.cc:862-879.
//   default               links liborbfe.so (tests/test_gpu_covisibility.py)
//   -DCOVIS_HOST_BACKEND  orbfe_covisibility_counts is defined HERE on top of tests/cpp/covisibility_ref.cpp, so that the
//                         facade's marshalling runs -- also under the sanitizers -- on a machine without a GPU
#include <cstdint>
#include <cstdio>
#include <list>
#include <vector>

#include "KeyFrame.h"
#include "MapPoint.h"
#include "orbfe/Covisibility.h"

using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::MapPoint;

// ---- the reference function, restated (not pinned) ---------------------------------------------------------------------
namespace ORB_SLAM2 {
struct CovisibilityRestated {
  static void UpdateConnections(KeyFrame* self) {
    std::map<KeyFrame*, int> KFcounter;
    std::vector<MapPoint*> vpMP;
    {
      std::unique_lock<std::mutex> lockMPs(self->mMutexFeatures);
      vpMP = self->mvpMapPoints;
    }
    for (std::vector<MapPoint*>::iterator vit = vpMP.begin(); vit != vpMP.end(); ++vit) {
      MapPoint* pMP = *vit;
      if (!pMP || pMP->isBad() || pMP->plCandidato || pMP->plLejano) continue;
      std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
      for (std::map<KeyFrame*, size_t>::iterator mit = observations.begin(); mit != observations.end(); ++mit) {
        if (mit->first->mnId == self->mnId) continue;
        KFcounter[mit->first]++;
      }
    }
    if (KFcounter.empty()) return;
    int nmax = 0;
    KeyFrame* pKFmax = nullptr;
    const int th = 15;
    std::vector<std::pair<int, KeyFrame*> > vPairs;
    for (std::map<KeyFrame*, int>::iterator mit = KFcounter.begin(); mit != KFcounter.end(); ++mit) {
      if (mit->second > nmax) { nmax = mit->second; pKFmax = mit->first; }
      if (mit->second >= th) {
        vPairs.push_back(std::make_pair(mit->second, mit->first));
        mit->first->AddConnection(self, mit->second);
      }
    }
    if (vPairs.empty()) {
      vPairs.push_back(std::make_pair(nmax, pKFmax));
      pKFmax->AddConnection(self, nmax);
    }
    std::sort(vPairs.begin(), vPairs.end());
    std::list<KeyFrame*> lKFs;
    std::list<int> lWs;
    for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(vPairs[i].second); lWs.push_front(vPairs[i].first); }
    std::unique_lock<std::mutex> lockCon(self->mMutexConnections);
    if (self->mbBad) return;
    self->mConnectedKeyFrameWeights = KFcounter;
    self->mvpOrderedConnectedKeyFrames = std::vector<KeyFrame*>(lKFs.begin(), lKFs.end());
    self->mvOrderedWeights = std::vector<int>(lWs.begin(), lWs.end());
    if (self->mbFirstConnection && self->mnId != 0) {
      self->mpParent = self->mvpOrderedConnectedKeyFrames.front();
      self->mpParent->AddChild(self);
      self->mbFirstConnection = false;
    }
  }
};
}  // namespace ORB_SLAM2

extern "C" int covis_ref_counts(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj, const int32_t* subj_self,
                                const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp, int32_t* out_offsets,
                                int32_t* out_kf, int32_t* out_count, int cap, int* n_needed);

#ifdef COVIS_HOST_BACKEND
struct orbfe_matcher { int unused; };
static int g_calls = 0;
extern "C" {
int orbfe_covisibility_counts(orbfe_matcher*, int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj,
                              const int32_t* subj_self, const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp,
                              int32_t* out_offsets, int32_t* out_kf, int32_t* out_count, int cap, int* n_needed) {
  g_calls++;
  return covis_ref_counts(n_kf, n_mp, obs_offsets, obs_kf, n_subj, subj_self, subj_limit, subj_offsets, subj_mp, out_offsets, out_kf, out_count,
                          cap, n_needed);
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

namespace {
constexpr int kKF = 40, kEntries = 200, kMP = 1400;
constexpr int kFew = 37, kNone = 38, kBad = 33, kTwice = 5;

struct World {
  KeyFrame kf[kKF];    // one array each: std::map<KeyFrame*, ...> iterates in index order in both worlds
  MapPoint mp[kMP];
  int used = 0;        // MapPoints that got their 2..12 observers
};

uint32_t g_state = 1u;
uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

// the keyframes' MapPoint vectors; no observation is added here
void build(World& W) {
  g_state = 20240607u;
  std::vector<std::vector<MapPoint*> > v(kKF, std::vector<MapPoint*>(kEntries, nullptr));
  int fill[kKF] = {0}, room[kKF];
  for (int k = 0; k < kKF; k++) room[k] = k == kNone ? 0 : (k == kFew ? 10 : kEntries - 8);   // a few entries stay null everywhere
  for (int p = 0; p < kMP; p++) {
    const int want = 2 + (int)(rnd() % 11u), centre = (int)(rnd() % (unsigned)kKF);
    std::vector<int> cand;
    for (int k = std::max(0, centre - 6); k <= std::min(kKF - 1, centre + 6); k++)
      if (fill[k] < room[k]) cand.push_back(k);
    if ((int)cand.size() < 2) continue;
    for (int i = (int)cand.size() - 1; i > 0; i--) std::swap(cand[i], cand[rnd() % (unsigned)(i + 1)]);
    const int n = std::min(want, (int)cand.size());
    MapPoint* pMP = &W.mp[W.used++];
    for (int i = 0; i < n; i++) v[cand[i]][fill[cand[i]]++] = pMP;
  }
  v[kTwice][kEntries - 1] = v[kTwice][0];      // one MapPoint at two keypoints of a keyframe: it counts twice
  W.mp[3].testSetBad(true);
  W.mp[4].plCandidato = true;
  W.mp[6].plLejano = MapPoint::lejano;
  for (int k = 0; k < kKF; k++) {
    W.kf[k].mnId = (long unsigned int)k;
    W.kf[k].testSetMapPoints(v[k]);
  }
  W.kf[kBad].testSetBad(true);
}

void observe(World& W, int k) {
  const std::vector<MapPoint*> v = W.kf[k].GetMapPointMatches();
  for (size_t i = 0; i < v.size(); i++)
    if (v[i]) v[i]->AddObservation(&W.kf[k], i);
}

int idx(const World& W, const KeyFrame* p) { return p ? (int)(p - W.kf) : -1; }

// 0 when every keyframe of the two worlds holds the same covisibility state
int same(const World& A, const World& B) {
  for (int k = 0; k < kKF; k++) {
    const KeyFrame &a = A.kf[k], &b = B.kf[k];
    CHECK(a.testWeights().size() == b.testWeights().size());
    std::map<KeyFrame*, int>::const_iterator ia = a.testWeights().begin(), ib = b.testWeights().begin();
    for (; ia != a.testWeights().end(); ++ia, ++ib) CHECK(idx(A, ia->first) == idx(B, ib->first) && ia->second == ib->second);
    CHECK(a.testOrdered().size() == b.testOrdered().size() && a.testOrderedWeights() == b.testOrderedWeights());
    CHECK(a.testOrdered().size() == a.testOrderedWeights().size());
    for (size_t i = 0; i < a.testOrdered().size(); i++) CHECK(idx(A, a.testOrdered()[i]) == idx(B, b.testOrdered()[i]));
    CHECK(idx(A, a.testParent()) == idx(B, b.testParent()) && a.testFirstConnection() == b.testFirstConnection());
    CHECK(a.testChildren().size() == b.testChildren().size());
    std::set<KeyFrame*>::const_iterator ca = a.testChildren().begin(), cb = b.testChildren().begin();
    for (; ca != a.testChildren().end(); ++ca, ++cb) CHECK(idx(A, *ca) == idx(B, *cb));
  }
  return 0;
}

World g_A, g_B, g_C, g_D;
}  // namespace

int main() {
  orbfe_matcher* m = nullptr;
#ifdef COVIS_HOST_BACKEND
  orbfe_matcher hm{0};
  m = &hm;
#else
  OK(orbfe_matcher_create(0, &m));
#endif

  // ---- map load: an order that is not pointer order -------------------------------------------------------------------
  std::vector<int> order(kKF);
  for (int k = 0; k < kKF; k++) order[k] = (k * 7 + 3) % kKF;    // 7 and 40 are coprime: every keyframe once
  build(g_A);
  build(g_B);
  CHECK(g_A.used == g_B.used && g_A.used > 800);
  for (int i = 0; i < kKF; i++) {
    observe(g_A, order[i]);
    ORB_SLAM2::CovisibilityRestated::UpdateConnections(&g_A.kf[order[i]]);
  }
  std::vector<KeyFrame*> vB;
  for (int i = 0; i < kKF; i++) { observe(g_B, order[i]); vB.push_back(&g_B.kf[order[i]]); }
  OK(orbfe::UpdateConnectionsBatch(m, vB, true));
  CHECK(same(g_A, g_B) == 0);
  // the scene does what it was built for
  {
    int threshold = 0, maximum = 0, withParent = 0;
    for (int k = 0; k < kKF; k++) {
      const std::vector<int>& w = g_A.kf[k].testOrderedWeights();
      if (!w.empty() && w[0] >= 15) threshold++;      // (the lists are re-sorted by the partners' AddConnection: best first)
      if (!w.empty() && w[0] < 15) maximum++;
      withParent += g_A.kf[k].testParent() != nullptr;
    }
    CHECK(threshold >= 30 && maximum >= 1 && withParent >= 30);
    CHECK(g_A.kf[kNone].testWeights().empty() && g_A.kf[kNone].testFirstConnection());
    CHECK(g_A.kf[kBad].testWeights().empty());                       // bad: nothing assigned, no AddConnection accepted
    CHECK(g_A.kf[0].testParent() == nullptr);
    const std::vector<int>& few = g_A.kf[kFew].testOrderedWeights();
    CHECK(!few.empty() && few[0] < 15);
  }

  // ---- loop closing: everything observed, 30 keyframes updated, ten observe from outside -------------------------------------
  build(g_C);
  build(g_D);
  for (int k = 0; k < kKF; k++) { observe(g_C, k); observe(g_D, k); }
  std::vector<KeyFrame*> vD;
  for (int i = 0; i < 30; i++) {
    ORB_SLAM2::CovisibilityRestated::UpdateConnections(&g_C.kf[order[i]]);
    vD.push_back(&g_D.kf[order[i]]);
  }
  OK(orbfe::UpdateConnectionsBatch(m, vD, false));
  CHECK(same(g_C, g_D) == 0);
  {
    // an observer outside the vector is among somebody's weights, and the keyframe that names a MapPoint twice counted it twice
    bool outside = false;
    for (int i = 0; i < 30 && !outside; i++)
      for (const auto& kv : g_D.kf[order[i]].testWeights()) {
        bool in = false;
        for (int j = 0; j < 30; j++) in = in || kv.first == &g_D.kf[order[j]];
        outside = outside || !in;
      }
    CHECK(outside);
    // a second call changes nothing (AddConnection with the weight it has returns early; mbFirstConnection is spent)
    OK(orbfe::UpdateConnectionsBatch(m, vD, false));
    CHECK(same(g_C, g_D) == 0);
    std::vector<KeyFrame*> twice(2, &g_D.kf[1]);
    CHECK(orbfe::UpdateConnectionsBatch(m, twice, false) == ORBFE_ERR_INVALID);
    CHECK(orbfe::UpdateConnectionsBatch(m, std::vector<KeyFrame*>(), false) == ORBFE_OK);
  }

  // ---- Tracking::UpdateLocalKeyFrames' keyframeCounter ----------------------------------------------------------------------
  {
    std::vector<MapPoint*> frame = g_D.kf[12].GetMapPointMatches();      // a frame that tracked keyframe 12's points ...
    const std::vector<MapPoint*> more = g_D.kf[20].GetMapPointMatches();
    frame.insert(frame.end(), more.begin(), more.begin() + 50);          // ... and some of keyframe 20's
    std::map<KeyFrame*, int> want;
    for (size_t i = 0; i < frame.size(); i++) {
      MapPoint* pMP = frame[i];
      if (!pMP || pMP->isBad()) continue;
      const std::map<KeyFrame*, size_t> observations = pMP->GetObservations();
      for (std::map<KeyFrame*, size_t>::const_iterator it = observations.begin(); it != observations.end(); ++it) want[it->first]++;
    }
    int rc = -99;
    const std::map<KeyFrame*, int> got = orbfe::CountObservers(m, frame, &rc);
    CHECK(rc == ORBFE_OK && got == want && want.count(&g_D.kf[12]) && want.size() > 5);
    const std::map<KeyFrame*, int> none = orbfe::CountObservers(m, std::vector<MapPoint*>(7, nullptr), &rc);
    CHECK(rc == ORBFE_OK && none.empty());
  }

#ifdef COVIS_HOST_BACKEND
  CHECK(g_calls == 4);   // one C call per batch (the refused and the empty ones make none), one for the frame
#else
  orbfe_matcher_destroy(m);
#endif
  std::printf("PASS\n");
  return 0;
}
