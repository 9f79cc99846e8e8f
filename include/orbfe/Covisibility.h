// Covisibility.h -- KeyFrame::UpdateConnections() (reference src/KeyFrame.cc:303-402) for a whole vector of keyframes, and the
// keyframeCounter of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:862-879), with the counting loop in one GPU call
// (orbfe_covisibility_counts, include/orbfe.h).  Every MapPoint of the given keyframes is walked ONCE on the host to write down
// who observes it; the per-keyframe, per-MapPoint, per-observer counting -- the std::map work of the reference -- runs on the
// device; what follows the counting (the threshold 15, AddConnection on the partners, the maximum rule, the sort, the weights,
// the first-connection parent) runs here per keyframe, in the order given, on the real pointers.  After the call the objects
// hold what the reference's UpdateConnections calls, made in the same order, would have left.
//
// Where the map load runs (src/Osmap.cpp:569-579)
//     for (KeyFrame* pKF : vectorKeyFrames) { /* AddObservation for pKF's MapPoints */  pKF->UpdateConnections(); }
// add every keyframe's observations first, then write
//     orbfe::UpdateConnectionsBatch(matcher, vectorKeyFrames, /*limitToPredecessors=*/true);
// (keyframe k then counts only observers 0..k of the vector, which is what it saw inside the loop).  Where LoopClosing runs
// UpdateConnections over a set of keyframes whose observations do not change in between (src/LoopClosing.cc:561), pass them
// with limitToPredecessors = false.  Tracking::UpdateLocalKeyFrames replaces its counting loop (Tracking.cc:862-879) by
//     std::map<KeyFrame*, int> keyframeCounter = orbfe::CountObservers(matcher, mCurrentFrame.mvpMapPoints);
// -- but see INTEGRATION.md for whether one frame's worth of counting is worth a device call.
//
// Needs the reference's own KeyFrame.h / MapPoint.h.  mConnectedKeyFrameWeights, mvpOrderedConnectedKeyFrames, mvOrderedWeights,
// mbFirstConnection, mpParent, mbBad and mMutexConnections are protected there: add `friend struct orbfe::CovisibilityAccess;`
// to class KeyFrame (or pass an Access type of your own with the same static function).
//
// Order: the reference iterates std::map<KeyFrame*, int>, i.e. in pointer order, and so does this header -- the device returns
// slots, the host turns them back into pointers and fills a std::map before any rule is applied.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "../orbfe.h"

namespace orbfe {

struct CovisibilityAccess {
  // KeyFrame.cc:374-392: under mMutexConnections; a keyframe that went bad keeps what it had
  template <class KF>
  static void setConnections(KF* pKF, const std::map<KF*, int>& KFcounter, const std::vector<KF*>& ordered, const std::vector<int>& weights) {
    std::unique_lock<std::mutex> lockCon(pKF->mMutexConnections);
    if (pKF->mbBad) return;
    pKF->mConnectedKeyFrameWeights = KFcounter;
    pKF->mvpOrderedConnectedKeyFrames = ordered;
    pKF->mvOrderedWeights = weights;
    if (pKF->mbFirstConnection && pKF->mnId != 0) {
      pKF->mpParent = pKF->mvpOrderedConnectedKeyFrames.front();
      pKF->mpParent->AddChild(pKF);
      pKF->mbFirstConnection = false;
    }
  }
};

// The two CSRs of one orbfe_covisibility_counts call, written down from the objects.  Keyframes get slots in the order they are
// registered (the subjects first, so that slot == position); observers met later get the slots after them.
template <class KF, class MP>
struct CovisibilityCsr {
  std::map<KF*, int32_t> slotOf;
  std::vector<KF*> kfs;                       // slot -> keyframe
  std::map<MP*, int32_t> indexOf;
  std::vector<int32_t> obsOffsets, obsKf;     // MapPoint -> observer slots
  std::vector<int32_t> subjSelf, subjLimit, subjOffsets, subjMp;
  CovisibilityCsr() : obsOffsets(1, 0), subjOffsets(1, 0) {}

  int32_t slot(KF* pKF) {
    typename std::map<KF*, int32_t>::iterator it = slotOf.find(pKF);
    if (it != slotOf.end()) return it->second;
    const int32_t s = (int32_t)kfs.size();
    slotOf[pKF] = s;
    kfs.push_back(pKF);
    return s;
  }
  // the MapPoint's index; its observations are read the first time it is seen, and `seen(pMP, observations)` is told of them
  template <class Seen>
  int32_t mapPoint(MP* pMP, Seen&& seen) {
    typename std::map<MP*, int32_t>::iterator it = indexOf.find(pMP);
    if (it != indexOf.end()) return it->second;
    const int32_t p = (int32_t)obsOffsets.size() - 1;
    indexOf[pMP] = p;
    const std::map<KF*, size_t> observations = pMP->GetObservations();
    for (typename std::map<KF*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) obsKf.push_back(slot(mit->first));
    obsOffsets.push_back((int32_t)obsKf.size());
    seen(pMP, observations);
    return p;
  }
  // one subject: `skip(pMP)` says which entries the reference loop passes over; `entry(i, p)` is told of every entry, skipped (p
  // is -1) or not, after `seen` has been told of its MapPoint
  template <class Skip, class Seen, class Entry>
  void subject(int32_t self, int32_t limit, const std::vector<MP*>& vpMP, Skip skip, Seen&& seen, Entry&& entry) {
    for (size_t i = 0; i < vpMP.size(); i++) {
      subjMp.push_back(skip(vpMP[i]) ? -1 : mapPoint(vpMP[i], seen));
      entry(i, subjMp.back());
    }
    subjSelf.push_back(self);
    subjLimit.push_back(limit);
    subjOffsets.push_back((int32_t)subjMp.size());
  }
  template <class Skip>
  void subject(int32_t self, int32_t limit, const std::vector<MP*>& vpMP, Skip skip) {
    subject(self, limit, vpMP, skip, [](MP*, const std::map<KF*, size_t>&) {}, [](size_t, int32_t) {});
  }
  int nSubjects() const { return (int)subjSelf.size(); }
  // no call needs more entries: per subject min(limit, observations reachable); limit < 0 stands for "every slot"
  long long bound() const {
    long long total = 0;
    for (int s = 0; s < nSubjects(); s++) {
      long long reach = 0;
      for (int32_t e = subjOffsets[s]; e < subjOffsets[s + 1]; e++)
        if (subjMp[e] >= 0) reach += obsOffsets[subjMp[e] + 1] - obsOffsets[subjMp[e]];
      const long long lim = subjLimit[s] < 0 ? (long long)kfs.size() : (long long)subjLimit[s];
      total += std::min(reach, lim);
    }
    return total;
  }
  // the call; limits < 0 become n_kf, known only now
  int run(orbfe_matcher* m, std::vector<int32_t>& outOffsets, std::vector<int32_t>& outKf, std::vector<int32_t>& outCount) {
    const int32_t nkf = (int32_t)kfs.size();
    const long long cap = bound();
    if (cap > 0x7fffffffLL) return ORBFE_ERR_INVALID;
    for (size_t s = 0; s < subjLimit.size(); s++)
      if (subjLimit[s] < 0) subjLimit[s] = nkf;
    outOffsets.assign((size_t)nSubjects() + 1, 0);
    outKf.assign((size_t)cap + 1, 0);
    outCount.assign((size_t)cap + 1, 0);
    int needed = 0;      // (an empty CSR's data() may be null: the call takes that)
    return orbfe_covisibility_counts(m, nkf, (int)obsOffsets.size() - 1, obsOffsets.data(), obsKf.data(), nSubjects(), subjSelf.data(), subjLimit.data(),
                                     subjOffsets.data(), subjMp.data(), outOffsets.data(), outKf.data(), outCount.data(), (int)cap, &needed);
  }
};

// KeyFrame::UpdateConnections() for vpKFs[0], vpKFs[1], ... in that order.  limitToPredecessors: keyframe k counts only the
// observers vpKFs[0..k] (the map load, where the later ones have not added their observations when k is updated); otherwise
// every observer, inside vpKFs or not.  A keyframe must not appear twice.  Returns ORBFE_OK or the C call's error code
// (orbfe_last_error() tells why); on an error no object has been changed.
template <class KeyFrameT, class Access = CovisibilityAccess>
inline int UpdateConnectionsBatch(orbfe_matcher* m, const std::vector<KeyFrameT*>& vpKFs, bool limitToPredecessors) {
  typedef decltype(vpKFs[0]->GetMapPointMatches()) MapPointVector;
  typedef typename MapPointVector::value_type MapPointPtr;
  typedef typename std::remove_pointer<MapPointPtr>::type MapPointT;
  if (vpKFs.empty()) return ORBFE_OK;
  CovisibilityCsr<KeyFrameT, MapPointT> csr;
  for (size_t k = 0; k < vpKFs.size(); k++)
    if (csr.slot(vpKFs[k]) != (int32_t)k) return ORBFE_ERR_INVALID;      // named twice
  for (size_t k = 0; k < vpKFs.size(); k++)
    csr.subject((int32_t)k, limitToPredecessors ? (int32_t)k + 1 : -1, vpKFs[k]->GetMapPointMatches(),
                [](MapPointT* pMP) { return !pMP || pMP->isBad() || pMP->plCandidato || pMP->plLejano; });   // KeyFrame.cc:320
  std::vector<int32_t> offs, okf, ocnt;
  const int rc = csr.run(m, offs, okf, ocnt);
  if (rc) return rc;

  for (size_t k = 0; k < vpKFs.size(); k++) {
    KeyFrameT* pKF = vpKFs[k];
    std::map<KeyFrameT*, int> KFcounter;
    for (int32_t i = offs[k]; i < offs[k + 1]; i++) KFcounter[csr.kfs[okf[i]]] = ocnt[i];
    if (KFcounter.empty()) continue;                                     // KeyFrame.cc:334
    int nmax = 0;
    KeyFrameT* pKFmax = nullptr;
    const int th = 15;
    std::vector<std::pair<int, KeyFrameT*> > vPairs;
    vPairs.reserve(KFcounter.size());
    for (typename std::map<KeyFrameT*, int>::iterator mit = KFcounter.begin(); mit != KFcounter.end(); ++mit) {
      if (mit->second > nmax) { nmax = mit->second; pKFmax = mit->first; }
      if (mit->second >= th) {
        vPairs.push_back(std::make_pair(mit->second, mit->first));
        mit->first->AddConnection(pKF, mit->second);
      }
    }
    if (vPairs.empty()) {
      vPairs.push_back(std::make_pair(nmax, pKFmax));
      pKFmax->AddConnection(pKF, nmax);
    }
    std::sort(vPairs.begin(), vPairs.end());
    std::vector<KeyFrameT*> ordered;
    std::vector<int> weights;
    for (size_t i = vPairs.size(); i-- > 0;) { ordered.push_back(vPairs[i].second); weights.push_back(vPairs[i].first); }   // push_front of each
    Access::setConnections(pKF, KFcounter, ordered, weights);
  }
  return ORBFE_OK;
}

// keyframeCounter of Tracking::UpdateLocalKeyFrames for the frame's mvpMapPoints: every observer of every MapPoint that is
// neither null nor bad, nobody excluded.  (The reference also resets the bad entries of the frame to NULL in the same loop; that
// stays with the caller.)  rc, if given, receives ORBFE_OK or the C call's error code; on an error the map is empty.
template <class MapPointT>
inline auto CountObservers(orbfe_matcher* m, const std::vector<MapPointT*>& frameMapPoints, int* rc = nullptr)
    -> std::map<typename decltype(frameMapPoints[0]->GetObservations())::key_type, int> {
  typedef typename decltype(frameMapPoints[0]->GetObservations())::key_type KeyFramePtr;
  typedef typename std::remove_pointer<KeyFramePtr>::type KeyFrameT;
  std::map<KeyFramePtr, int> keyframeCounter;
  if (rc) *rc = ORBFE_OK;
  CovisibilityCsr<KeyFrameT, MapPointT> csr;
  csr.subject(-1, -1, frameMapPoints, [](MapPointT* pMP) { return !pMP || pMP->isBad(); });
  if (csr.kfs.empty()) return keyframeCounter;
  std::vector<int32_t> offs, okf, ocnt;
  const int r = csr.run(m, offs, okf, ocnt);
  if (rc) *rc = r;
  if (r) return keyframeCounter;
  for (int32_t i = offs[0]; i < offs[1]; i++) keyframeCounter[csr.kfs[okf[i]]] = ocnt[i];
  return keyframeCounter;
}

}  // namespace orbfe
