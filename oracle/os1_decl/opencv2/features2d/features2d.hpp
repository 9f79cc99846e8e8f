/* Stand-in for <opencv2/features2d/features2d.hpp>: cv::KeyPoint is all ORBmatcher.cc takes from it, and the stand-in core
 * header declares it.  Our own text.  TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_DECL_OPENCV2_FEATURES2D_FEATURES2D_HPP_
#define OS1_DECL_OPENCV2_FEATURES2D_FEATURES2D_HPP_
#include "../core/core.hpp"
#endif
