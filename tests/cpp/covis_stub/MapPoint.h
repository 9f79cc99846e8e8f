// TEST INFRASTRUCTURE ONLY -- the members of the reference's MapPoint (include/MapPoint.h) that include/orbfe/Covisibility.h
// touches: the observation map and the three marks UpdateConnections skips a MapPoint for.  In a real build the reference's own
// header is used.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>

namespace ORB_SLAM2 {
class KeyFrame;
class MapPoint {
 public:
  enum lejania { cercano = 0, lejano = 1, muyLejano = 2 };
  std::map<KeyFrame*, size_t> GetObservations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mObservations; }
  bool isBad() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mbBad; }
  void AddObservation(KeyFrame* pKF, size_t idx) {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    if (mObservations.count(pKF)) return;
    mObservations[pKF] = idx;
  }
  bool plCandidato = false;
  lejania plLejano = cercano;
  // test side
  void testSetBad(bool b) { mbBad = b; }

 protected:
  std::map<KeyFrame*, size_t> mObservations;
  bool mbBad = false;
  std::mutex mMutexFeatures;
};
}  // namespace ORB_SLAM2
