/* Stand-in for the reference's Frame.h for oracle/_ref/libos1_kfdb.so: the two members src/KeyFrameDatabase.cc reads of a Frame.
 * Our own text.  TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_KFDB_DECL_FRAME_H_
#define OS1_KFDB_DECL_FRAME_H_
#include "BowVector.h"

namespace ORB_SLAM2 {

class Frame {
 public:
  long unsigned int mnId = 0;
  DBoW2::BowVector mBowVec;
};

}  // namespace ORB_SLAM2
#endif
