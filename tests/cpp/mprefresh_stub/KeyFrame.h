// TEST INFRASTRUCTURE ONLY -- the members of the reference's KeyFrame (include/KeyFrame.h) that
// include/orbfe/MapPointRefresh.h touches, with just enough behaviour for tests/cpp/map_point_refresh_test.cpp to build a small
// map.  In a real build the reference's own header is used.
#pragma once
#include <vector>

#include <opencv2/core/core.hpp>
namespace ORB_SLAM2 {
class KeyFrame {
 public:
  long unsigned int mnId = 0;
  int mnScaleLevels = 0;
  std::vector<float> mvScaleFactors;
  cv::Mat mDescriptors;                       // [N][32] CV_8U
  cv::Mat GetCameraCenter() { return Ow.clone(); }
  bool isBad() { return bad; }
  // test side
  cv::Mat Ow;
  bool bad = false;
};
}  // namespace ORB_SLAM2
