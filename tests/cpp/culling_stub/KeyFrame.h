// TEST INFRASTRUCTURE ONLY -- the members of the reference's KeyFrame (include/KeyFrame.h) that include/orbfe/KeyFrameCulling.h
// touches, with WORKING SetBadFlag behaviour (src/KeyFrame.cc:478-): keyframe 0 is never erased, a keyframe held by mbNotErase
// only notes mbToBeErased, any other goes bad and erases its observation from every MapPoint it matched -- which may send that
// MapPoint bad in turn (MapPoint.h).  The spanning tree, the connections, the map and the keyframe database are left out: the
// culling loop reads none of them.
#pragma once
#include <mutex>
#include <vector>

#include "MapPoint.h"
namespace cv {
struct KeyPoint {       // the one member the loop reads
  int octave = 0;
};
}  // namespace cv
namespace ORB_SLAM2 {
class KeyFrame {
 public:
  long unsigned int mnId = 0;
  std::vector<cv::KeyPoint> mvKeysUn;
  std::vector<MapPoint*> GetMapPointMatches() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mvpMapPoints; }
  bool isBad() { std::unique_lock<std::mutex> lock(mMutexConnections); return mbBad; }
  void SetNotErase() { std::unique_lock<std::mutex> lock(mMutexConnections); mbNotErase = true; }
  void EraseMapPointMatch(const size_t& idx) { std::unique_lock<std::mutex> lock(mMutexFeatures); mvpMapPoints[idx] = nullptr; }
  void SetBadFlag() {
    testSetBadFlagCalls++;
    {
      std::unique_lock<std::mutex> lock(mMutexConnections);
      if (mnId == 0) return;
      if (mbNotErase) { mbToBeErased = true; return; }
      if (mbBad) return;
      mbBad = true;
    }
    for (size_t i = 0; i < mvpMapPoints.size(); i++)
      if (mvpMapPoints[i]) mvpMapPoints[i]->EraseObservation(this);
  }
  // test side: one keypoint at `octave` matched to pMP (null: unmatched); the observation is added on the MapPoint's side
  size_t testAddKeyPoint(int octave, MapPoint* pMP) {
    cv::KeyPoint kp;
    kp.octave = octave;
    mvKeysUn.push_back(kp);
    mvpMapPoints.push_back(pMP);
    if (pMP) pMP->AddObservation(this, mvKeysUn.size() - 1);
    return mvKeysUn.size() - 1;
  }
  bool testToBeErased() const { return mbToBeErased; }
  int testSetBadFlagCalls = 0;      // how often the loop applied a verdict to this keyframe

 protected:
  std::vector<MapPoint*> mvpMapPoints;
  bool mbNotErase = false, mbToBeErased = false, mbBad = false;
  std::mutex mMutexConnections;
  std::mutex mMutexFeatures;
};

inline void MapPoint::EraseObservation(KeyFrame* pKF) {
  bool bBad = false;
  {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    if (mObservations.count(pKF)) {
      nObs--;
      mObservations.erase(pKF);
      if (nObs <= 2) bBad = true;
    }
  }
  if (bBad) SetBadFlag();
}
inline void MapPoint::SetBadFlag() {
  std::map<KeyFrame*, size_t> obs;
  {
    std::unique_lock<std::mutex> lock(mMutexFeatures);
    mbBad = true;
    obs = mObservations;
    mObservations.clear();
  }
  for (std::map<KeyFrame*, size_t>::iterator mit = obs.begin(); mit != obs.end(); ++mit) mit->first->EraseMapPointMatch(mit->second);
}
}  // namespace ORB_SLAM2
