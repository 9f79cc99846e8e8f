// KeyFrameDatabase.h -- drop-in ORB_SLAM2::KeyFrameDatabase (reference include/KeyFrameDatabase.h:41-148) backed by liborbfe.so.
// Same constructor, same member functions, same signatures: put this file in place of the reference's
// include/KeyFrameDatabase.h and drop src/KeyFrameDatabase.cc from the build; System.cc, Tracking.cc, LoopClosing.cc, KeyFrame.cc
// and Map handling compile unchanged.  The inverted file and the mpVoc->score calls are one GPU query over the BowVectors of the
// map's keyframes, which live in HBM (include/orbfe.h, keyframe database section); the bookkeeping on the KeyFrame members and
// the candidate selection are the reference's, statement for statement (orbfe::KeyFrameDatabaseT in include/orbfe/orb_shim.hpp).
//
// Needs the reference's own KeyFrame.h / Frame.h / ORBVocabulary.h (the signatures use their types).  The vocabulary is only
// asked for its size and its scoring type: L1_NORM (ORBvoc's), L2_NORM, CHI_SQUARE and DOT_PRODUCT are built; with a KL or
// BHATTACHARYYA vocabulary the first add throws.
#pragma once
#include <mutex>
#include <set>
#include <vector>

#include "Frame.h"
#include "KeyFrame.h"
#include "ORBVocabulary.h"
#include "orb_shim.hpp"

namespace ORB_SLAM2 {

class KeyFrameDatabase {
 public:
  KeyFrameDatabase(const ORBVocabulary& voc)
      : mpVoc(&voc), mDb(orbfe::detail::defaultDevice(), voc.size(), (int)voc.getScoringType()) {}   // ORBFE_DEVICE, as the matcher

  void add(KeyFrame* pKF) { mDb.add(pKF); }
  // Not in the reference: add(pKF) for every keyframe of a loaded map in one call (the add loop of Osmap::rebuild, src/Osmap.cpp)
  void add(const std::vector<KeyFrame*>& vpKFs) { mDb.add(vpKFs); }
  void erase(KeyFrame* pKF) { mDb.erase(pKF); }
  void clear() { mDb.clear(); }

  // Loop Detection
  std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* pKF, float minScore) { return mDb.DetectLoopCandidates(pKF, minScore); }

  // Relocalization
  std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* F) { return mDb.DetectRelocalizationCandidates(F); }

  void resizeInvertedFile(size_t n) { mDb.resizeInvertedFile(n); }

  // Not in the reference: the reference minimum score of LoopClosing::DetectLoop (src/LoopClosing.cc:125-140), computed on the
  // BowVectors the database already holds in HBM.  `float minScore = mpKeyFrameDB->MinCovisibleScore(mpCurrentKF);` replaces
  // those sixteen lines; leaving them as they are is correct too (they score on the host through DBoW2).
  float MinCovisibleScore(KeyFrame* pKF) { return mDb.MinCovisibleScore(pKF); }

  int verbose = 0;   // (the reference prints statistics when set; this class prints nothing)

 protected:
  const ORBVocabulary* mpVoc;
  orbfe::KeyFrameDatabaseT<KeyFrame> mDb;
};

}  // namespace ORB_SLAM2
