/* Stand-in for the reference's Frame.h, written for one purpose: to compile the reference's ORBmatcher.cc, unmodified, into
 * oracle/_ref/libos1_matcher.so.  Our own text: a plain data holder with the fields that file reads and writes.
 *
 * What is a RESTATEMENT here (not compiled reference code): the feature grid -- its cell size (src/Frame.cc:98-99), the cell of a
 * keypoint (PosInGrid, src/Frame.cc:264-274: round() half away from zero, keypoints outside the grid are in no cell), the fill in
 * index order (AssignFeaturesToGrid, src/Frame.cc:114-129) and GetFeaturesInArea (src/Frame.cc:209-262: the four early returns,
 * bCheckLevels = minLevel > 0 || maxLevel >= 0, columns outside rows inside, strict |d| < r).  KeyFrame.h reuses it.
 * TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_DECL_FRAME_H_
#define OS1_DECL_FRAME_H_
#include <algorithm>
#include <cmath>
#include <vector>
#include <opencv2/core/core.hpp>
#include "FeatureVector.h"   // DBoW2's own, found through the include path (oracle/Makefile)
#include "MapPoint.h"

#define FRAME_GRID_ROWS 48
#define FRAME_GRID_COLS 64

namespace ORB_SLAM2 {

struct FeatureGrid {
  float minX, maxX, minY, maxY, invW, invH;
  std::vector<size_t> cell[FRAME_GRID_COLS][FRAME_GRID_ROWS];

  void build(const std::vector<cv::KeyPoint>& keysUn, float mnX, float mxX, float mnY, float mxY) {
    minX = mnX; maxX = mxX; minY = mnY; maxY = mxY;
    invW = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(maxX - minX);
    invH = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(maxY - minY);
    for (int c = 0; c < FRAME_GRID_COLS; c++)
      for (int r = 0; r < FRAME_GRID_ROWS; r++) cell[c][r].clear();
    for (size_t i = 0; i < keysUn.size(); i++) {
      const int px = (int)std::round((keysUn[i].pt.x - minX) * invW);
      const int py = (int)std::round((keysUn[i].pt.y - minY) * invH);
      if (px < 0 || px >= FRAME_GRID_COLS || py < 0 || py >= FRAME_GRID_ROWS) continue;
      cell[px][py].push_back(i);
    }
  }
  std::vector<size_t> inArea(const std::vector<cv::KeyPoint>& keysUn, float x, float y, float r, int minLevel, int maxLevel) const {
    std::vector<size_t> out;
    const int c0 = std::max(0, (int)std::floor((x - minX - r) * invW));
    if (c0 >= FRAME_GRID_COLS) return out;
    const int c1 = std::min((int)FRAME_GRID_COLS - 1, (int)std::ceil((x - minX + r) * invW));
    if (c1 < 0) return out;
    const int r0 = std::max(0, (int)std::floor((y - minY - r) * invH));
    if (r0 >= FRAME_GRID_ROWS) return out;
    const int r1 = std::min((int)FRAME_GRID_ROWS - 1, (int)std::ceil((y - minY + r) * invH));
    if (r1 < 0) return out;
    const bool levels = (minLevel > 0) || (maxLevel >= 0);
    for (int c = c0; c <= c1; c++)
      for (int rr = r0; rr <= r1; rr++)
        for (size_t j = 0; j < cell[c][rr].size(); j++) {
          const cv::KeyPoint& kp = keysUn[cell[c][rr][j]];
          if (levels) {
            if (kp.octave < minLevel) continue;
            if (maxLevel >= 0 && kp.octave > maxLevel) continue;
          }
          const float dx = kp.pt.x - x, dy = kp.pt.y - y;
          if (std::fabs(dx) < r && std::fabs(dy) < r) out.push_back(cell[c][rr][j]);
        }
    return out;
  }
};

class Frame {
 public:
  Frame() : N(0), fx(0), fy(0), cx(0), cy(0), mbf(0), mfLogScaleFactor(0), mnMinX(0), mnMaxX(0), mnMinY(0), mnMaxY(0) {}

  int N;
  std::vector<cv::KeyPoint> mvKeys, mvKeysUn;
  cv::Mat mDescriptors;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<bool> mvbOutlier;
  DBoW2::FeatureVector mFeatVec;
  cv::Mat mTcw;
  float fx, fy, cx, cy, mbf;
  std::vector<float> mvScaleFactors, mvLevelSigma2, mvInvLevelSigma2;
  float mfLogScaleFactor;
  float mnMinX, mnMaxX, mnMinY, mnMaxY;

  void AssignFeaturesToGrid() { grid.build(mvKeysUn, mnMinX, mnMaxX, mnMinY, mnMaxY); }
  std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, const int minLevel = -1,
                                        const int maxLevel = -1) const {
    return grid.inArea(mvKeysUn, x, y, r, minLevel, maxLevel);
  }

 private:
  FeatureGrid grid;
};

}  // namespace ORB_SLAM2
#endif
