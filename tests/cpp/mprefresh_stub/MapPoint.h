// TEST INFRASTRUCTURE ONLY -- the members of the reference's MapPoint (include/MapPoint.h) that
// include/orbfe/MapPointRefresh.h touches: the observation map, the reference keyframe, and the PROTECTED fields the two
// refreshed functions write, opened to the facade by the one friend line an integrator adds to the real header.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>

#include <opencv2/core/core.hpp>

#include "KeyFrame.h"
namespace orbfe { struct MapPointRefreshAccess; }
namespace ORB_SLAM2 {
class MapPoint {
 public:
  std::map<KeyFrame*, size_t> GetObservations() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mObservations; }
  KeyFrame* GetReferenceKeyFrame() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mpRefKF; }
  cv::Mat GetWorldPos() { std::unique_lock<std::mutex> lock(mMutexPos); return mWorldPos.clone(); }
  cv::Mat GetNormal() { std::unique_lock<std::mutex> lock(mMutexPos); return mNormalVector.clone(); }
  cv::Mat GetDescriptor() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mDescriptor.clone(); }
  bool isBad() { std::unique_lock<std::mutex> lock(mMutexFeatures); return mbBad; }
  // test side: build the object, read the raw fields back
  void testInit(const float pos[3], KeyFrame* ref, bool bad) {
    mWorldPos = cv::Mat(3, 1, CV_32F);
    mNormalVector = cv::Mat(3, 1, CV_32F);
    mDescriptor = cv::Mat(1, 32, CV_8U);
    for (int k = 0; k < 3; k++) { mWorldPos.at<float>(k) = pos[k]; mNormalVector.at<float>(k) = -7.0f; }
    for (int k = 0; k < 32; k++) mDescriptor.at<unsigned char>(k) = 0xA5;
    mfMinDistance = -1.0f; mfMaxDistance = -2.0f;
    mpRefKF = ref; mbBad = bad;
  }
  void testObserve(KeyFrame* kf, size_t idx) { mObservations[kf] = idx; }
  float testMin() const { return mfMinDistance; }
  float testMax() const { return mfMaxDistance; }

 protected:
  friend struct orbfe::MapPointRefreshAccess;
  cv::Mat mWorldPos;
  std::map<KeyFrame*, size_t> mObservations;
  cv::Mat mNormalVector;
  cv::Mat mDescriptor;
  KeyFrame* mpRefKF = nullptr;
  bool mbBad = false;
  float mfMinDistance = 0, mfMaxDistance = 0;
  std::mutex mMutexPos;
  std::mutex mMutexFeatures;
};
}  // namespace ORB_SLAM2
