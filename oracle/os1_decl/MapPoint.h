/* Stand-in for the reference's MapPoint.h, written for one purpose: to compile the reference's ORBmatcher.cc, unmodified, into
 * oracle/_ref/libos1_matcher.so.  Our own text: a plain data holder with the fields and accessors that file touches.
 *
 * What is a RESTATEMENT here (not compiled reference code):
 *   GetMinDistanceInvariance / GetMaxDistanceInvariance   0.8f / 1.2f times the raw fields        (src/MapPoint.cc:358-368)
 *   PredictScale                                          ceil(log(max / dist) / logScaleFactor), float overloads of <cmath>
 *                                                         on the host: logf, ceilf               (src/MapPoint.cc:370-379)
 *   AddObservation / Replace / IsInKeyFrame / GetIndexInKeyFrame   the SIMPLIFIED bookkeeping model that oracle/orb_oracle_pose.h
 *       documents for OrcPoints: a point observes ONE keyframe of interest (obsKF) at slot idxInKF (-1: not), nObs counts its
 *       observations in all keyframes.  AddObservation is src/MapPoint.cc:72-78 without the far-point re-triangulation that
 *       follows it; Replace is src/MapPoint.cc:158-198 over that one observation (the observations in other keyframes move to
 *       the replacing point as a count), without the found / visible counters, ComputeDistinctiveDescriptors and the map.
 * TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_DECL_MAPPOINT_H_
#define OS1_DECL_MAPPOINT_H_
#include <cmath>
#include <cstddef>
#include <map>
#include <set>
#include <vector>
#include <opencv2/core/core.hpp>

using namespace std;   // the reference's headers name vector / pair / set unqualified (ORBmatcher.h)

namespace ORB_SLAM2 {

class KeyFrame;
class Frame;

class MapPoint {
 public:
  MapPoint()
      : mTrackProjX(0), mTrackProjY(0), mbTrackInView(false), mnTrackScaleLevel(0), mTrackViewCos(0), plCandidato(false), id(-1),
        mfMinDistance(0), mfMaxDistance(0), mbBad(false), nObs(0), idxInKF(-1), obsKF(NULL) {}

  // what Frame::isInFrustum leaves on the point for SearchByProjection(Frame&, vpMapPoints, th)
  float mTrackProjX, mTrackProjY;
  bool mbTrackInView;
  int mnTrackScaleLevel;
  float mTrackViewCos;
  bool plCandidato;

  // the table row behind the point
  int id;
  cv::Mat mWorldPos, mNormalVector, mDescriptor;
  float mfMinDistance, mfMaxDistance;
  bool mbBad;
  int nObs;
  int idxInKF;
  KeyFrame* obsKF;

  cv::Mat GetWorldPos() { return mWorldPos.clone(); }
  cv::Mat GetNormal() { return mNormalVector.clone(); }
  cv::Mat GetDescriptor() { return mDescriptor.clone(); }
  bool isBad() { return mbBad; }
  int Observations() { return nObs; }
  float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
  float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
  int PredictScale(const float& currentDist, const float& logScaleFactor) {
    const float ratio = mfMaxDistance / currentDist;
    return (int)std::ceil(std::log(ratio) / logScaleFactor);
  }
  bool IsInKeyFrame(KeyFrame*) { return idxInKF >= 0; }
  int GetIndexInKeyFrame(KeyFrame*) { return idxInKF; }
  void AddObservation(KeyFrame* pKF, size_t idx) {
    if (idxInKF >= 0) return;
    idxInKF = (int)idx;
    obsKF = pKF;
    nObs++;
  }
  inline void Replace(MapPoint* pMP);   // (KeyFrame.h: it writes the keyframe's slot)
};

}  // namespace ORB_SLAM2
#endif
