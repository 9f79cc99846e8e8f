// TEST INFRASTRUCTURE ONLY -- the member NAMES of the reference's KeyFrame / Frame / ORBVocabulary that
// include/orbfe/KeyFrameDatabase.h touches (reference include/KeyFrame.h, Frame.h, ORBVocabulary.h), declarations only, for the
// syntax check in tests/test_kfdb.py.  In a real build the reference's own headers are used.
#pragma once
#include <map>
#include <set>
#include <vector>
namespace DBoW2 {
typedef std::map<unsigned int, double> BowVector;
enum ScoringType { L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT };   // BowVector.h:45-53
}
namespace ORB_SLAM2 {
class KeyFrame {
 public:
  long unsigned int mnId;           // KeyFrame.h:574
  DBoW2::BowVector mBowVec;
  long unsigned int mnLoopQuery;    // KeyFrame.h:613-628
  int mnLoopWords;
  float mLoopScore;
  long unsigned int mnRelocQuery;
  int mnRelocWords;
  float mRelocScore;
  std::set<KeyFrame*> GetConnectedKeyFrames();
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames();
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N);
  bool isBad();
};
class Frame {
 public:
  long unsigned int mnId;           // Frame.h:399
  DBoW2::BowVector mBowVec;
};
class ORBVocabulary {               // DBoW2::TemplatedVocabulary<...>: TemplatedVocabulary.h:122, 231
 public:
  unsigned int size() const;
  DBoW2::ScoringType getScoringType() const;
};
}  // namespace ORB_SLAM2
