/* Stand-in for the reference's Frame.h for oracle/_ref/libos1_initializer.so: the two members src/Initializer.cc reads of a Frame
 * (the constructor and Initialize take mK and mvKeysUn).  The reference's headers name std's containers unqualified, as the
 * reference's own Frame.h lets them.  Our own text.  TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_INITIALIZER_DECL_FRAME_H_
#define OS1_INITIALIZER_DECL_FRAME_H_
#include <utility>
#include <vector>

#include <opencv2/opencv.hpp>

using namespace std;

namespace ORB_SLAM2 {

class Frame {
 public:
  cv::Mat mK;
  std::vector<cv::KeyPoint> mvKeysUn;
};

}  // namespace ORB_SLAM2
#endif
