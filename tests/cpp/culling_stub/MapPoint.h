// TEST INFRASTRUCTURE ONLY -- the members of the reference's MapPoint (include/MapPoint.h) that include/orbfe/KeyFrameCulling.h
// touches, with WORKING EraseObservation / SetBadFlag behaviour (src/MapPoint.cc: a MapPoint left with two observations or fewer
// goes bad, drops its observations and leaves the keyframes that matched it), written again so that a cull changes the graph the
// next count reads.  The two functions that call into KeyFrame are defined at the end of KeyFrame.h.  In a real build the
// reference's own header is used.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
 public:
  std::map<KeyFrame*, size_t> GetObservations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mObservations; }
  int Observations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return nObs; }
  bool isBad() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mbBad; }
  void AddObservation(KeyFrame* pKF, size_t idx) {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
    nObs++;
  }
  inline void EraseObservation(KeyFrame* pKF);
  inline void SetBadFlag();
  // test side
  void testSetNobs(int n) { nObs = n; }

 protected:
  std::map<KeyFrame*, size_t> mObservations;
  int nObs = 0;
  bool mbBad = false;
  std::mutex mMutexFeatures;
};
}  // namespace ORB_SLAM2
