// triangulation_search_syntax.cpp -- instantiates include/orbfe/TriangulationSearch.h with cv::Mat and ORB_SLAM2::KeyFrame of the
// declaration-level stand-ins in tests/cpp/opencv_stub and tests/cpp/os1_stub, at the call site that replaces
// LocalMapping.cc:207-232.  Compiled with -fsyntax-only (tests/test_triangulation_search_facade.py).  Never linked, never run.
#include "orbfe/ORBmatcher.h"
#include "orbfe/TriangulationSearch.h"

using namespace ORB_SLAM2;

int createNewMapPoints(orbfe::MatcherContext& ctx, KeyFrame* mpCurrentKeyFrame, const std::vector<KeyFrame*>& vpNeighKFs,
                       const std::vector<cv::Mat>& vF12) {
  orbfe::TriangulationSearch<KeyFrame> S(ctx, true, mpCurrentKeyFrame, vpNeighKFs, vF12);
  int n = 0;
  for (size_t i = 0; i < S.size(); i++) {
    std::vector<std::pair<size_t, size_t> > vMatchedIndices;
    n += S.pairs(i, vMatchedIndices);
  }
  return n + S.fallbacks() + (S.batched() ? 1 : 0) + (int)S.ex(0) + (int)S.ey(0);
}
