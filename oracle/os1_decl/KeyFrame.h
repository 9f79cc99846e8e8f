/* Stand-in for the reference's KeyFrame.h, written for one purpose: to compile the reference's ORBmatcher.cc, unmodified, into
 * oracle/_ref/libos1_matcher.so.  Our own text: a plain data holder with the fields and accessors that file touches.
 *
 * What is a RESTATEMENT here (not compiled reference code):
 *   GetFeaturesInArea   src/KeyFrame.cc:637-676: the Frame's grid and window test without a level filter (Frame.h's FeatureGrid)
 *   IsInImage           src/KeyFrame.cc:678-681: x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY
 *   SetPose             src/KeyFrame.cc:89-102: Rwc = Rcw.t() evaluated, then Ow = -Rwc*tcw (a plain gemm with alpha = -1, NOT the
 *                       transposed path of `-Rcw.t()*tcw`); GetRotation / GetTranslation / GetCameraCenter return clones (:116-132)
 *   GetMapPoints        src/KeyFrame.cc:249-262: the slots that are neither NULL nor bad
 *   AddMapPoint and the slot writes of MapPoint::Replace (ReplaceMapPointMatch / EraseMapPointMatch): the simplified bookkeeping
 *                       model of oracle/orb_oracle_pose.h (see MapPoint.h)
 * The image bounds are kept as the floats the oracle's OrcView carries; the reference's KeyFrame declares them `const int`.
 * TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_DECL_KEYFRAME_H_
#define OS1_DECL_KEYFRAME_H_
#include <set>
#include <vector>
#include "Frame.h"
#include "MapPoint.h"

namespace ORB_SLAM2 {

class KeyFrame {
 public:
  KeyFrame() : N(0), fx(0), fy(0), cx(0), cy(0), mbf(0), mfLogScaleFactor(0), mnMinX(0), mnMaxX(0), mnMinY(0), mnMaxY(0) {}

  int N;
  std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  cv::Mat mDescriptors;
  std::vector<MapPoint*> mvpMapPoints;
  DBoW2::FeatureVector mFeatVec;
  float fx, fy, cx, cy, mbf;
  std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
  float mfLogScaleFactor;
  float mnMinX, mnMaxX, mnMinY, mnMaxY;

  void AssignFeaturesToGrid() { grid.build(mvKeysUn, mnMinX, mnMaxX, mnMinY, mnMaxY); }
  void SetPose(const cv::Mat& Tcw_) {
    Tcw = Tcw_.clone();
    const cv::Mat R = Tcw.rowRange(0, 3).colRange(0, 3), t = Tcw.rowRange(0, 3).col(3);
    const cv::Mat Rt = R.t();   // the transpose is evaluated first ...
    Ow = -Rt * t;               // ... so this is the plain product with alpha = -1
  }
  void SetCameraCenter(const cv::Mat& c) { Ow = c.clone(); }   // (the wrapper's: an epipole given as a number)
  cv::Mat GetRotation() { return Tcw.rowRange(0, 3).colRange(0, 3).clone(); }
  cv::Mat GetTranslation() { return Tcw.rowRange(0, 3).col(3).clone(); }
  cv::Mat GetCameraCenter() { return Ow.clone(); }

  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
  std::set<MapPoint*> GetMapPoints() {
    std::set<MapPoint*> s;
    for (MapPoint* p : mvpMapPoints)
      if (p && !p->isBad()) s.insert(p);
    return s;
  }
  void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }

  std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r) const {
    return grid.inArea(mvKeysUn, x, y, r, -1, -1);
  }
  bool IsInImage(const float& x, const float& y) const { return x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY; }

 private:
  cv::Mat Tcw, Ow;
  FeatureGrid grid;
};

// this->Replace(pMP) in the simplified model (MapPoint.h)
inline void MapPoint::Replace(MapPoint* pMP) {
  if (pMP->id == id) return;
  mbBad = true;
  const int ia = idxInKF;
  KeyFrame* pKF = obsKF;
  pMP->nObs += nObs - (ia >= 0 ? 1 : 0);   // the observations in other keyframes move over
  nObs = 0;
  idxInKF = -1;
  if (ia >= 0) {
    if (!pMP->IsInKeyFrame(pKF)) {
      pKF->mvpMapPoints[ia] = pMP;
      pMP->AddObservation(pKF, ia);
    } else {
      pKF->mvpMapPoints[ia] = NULL;
    }
  }
}

}  // namespace ORB_SLAM2
#endif
