/* Stand-in for the reference's KeyFrame.h, written to compile its src/KeyFrameDatabase.cc unmodified into
 * oracle/_ref/libos1_kfdb.so (oracle/Makefile).  Our own text: a plain data holder with exactly the members and the two getters
 * that file uses, in the reference's types (KeyFrame.h: long unsigned int ids and queries, int word counts, float scores).  The
 * reference's constructor zeroes the queries and the word counts and leaves the two scores uninitialised; here they start at 0, as
 * in the restatements.  `index` and `bad` are the wrapper's (oracle/os1_kfdb_wrap.cpp).  TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_KFDB_DECL_KEYFRAME_H_
#define OS1_KFDB_DECL_KEYFRAME_H_
#include <set>
#include <vector>

#include "BowVector.h"

namespace ORB_SLAM2 {

class KeyFrame {
 public:
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
  long unsigned int mnLoopQuery = 0;
  int mnLoopWords = 0;
  float mLoopScore = 0;
  long unsigned int mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0;

  std::set<KeyFrame*> GetConnectedKeyFrames() { return connected; }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {   // the first N of the ordered list
    if ((int)covisible.size() < N) return covisible;
    return std::vector<KeyFrame*>(covisible.begin(), covisible.begin() + N);
  }

  std::set<KeyFrame*> connected;
  std::vector<KeyFrame*> covisible;
  bool bad = false;
  int index = 0;
};

}  // namespace ORB_SLAM2
#endif
