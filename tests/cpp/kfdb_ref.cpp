// kfdb_ref.cpp -- TEST INFRASTRUCTURE: a literal restatement of the reference's keyframe database and of the scorings it calls,
// on a model keyframe, behind a C interface (Python drives it through ctypes, tests/cpp/kfdb_test.cpp links it).
//   KeyFrameDatabase::add / erase / clear / DetectLoopCandidates / DetectRelocalizationCandidates   src/KeyFrameDatabase.cc:38-334
//   the covisible minimum score of LoopClosing::DetectLoop                                            src/LoopClosing.cc:125-140
//   L1Scoring / L2Scoring / ChiSquareScoring / DotProductScoring ::score            Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311
// Statement for statement, with the reference's containers (std::vector<std::list<KF*>> inverted file, std::map BowVectors,
// std::set / std::list in the Detect* bodies) and its float / double / int types.  The scorings are restated rather than
// compiled from the reference because ScoringObject.cpp includes TemplatedVocabulary.h and with it OpenCV.
// Lines marked "(counter)" are not in the reference: they count how often a branch was taken, for the tests' shape assertions.
// Build: g++ -std=c++17 -O2 -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <utility>
#include <vector>

namespace {

typedef std::map<unsigned int, double> BowVector;   // DBoW2/BowVector.h:56-58 (WordId -> WordValue)
typedef double WordValue;

// ---- ScoringObject.cpp --------------------------------------------------------------------------------------------------
// double L1Scoring::score(const BowVector &v1, const BowVector &v2) const   ScoringObject.cpp:23-68
double scoreL1(const BowVector& v1, const BowVector& v2) {
  BowVector::const_iterator v1_it, v2_it;
  const BowVector::const_iterator v1_end = v1.end();
  const BowVector::const_iterator v2_end = v2.end();
  v1_it = v1.begin();
  v2_it = v2.begin();
  double score = 0;
  while (v1_it != v1_end && v2_it != v2_end) {
    const WordValue& vi = v1_it->second;
    const WordValue& wi = v2_it->second;
    if (v1_it->first == v2_it->first) {
      score += fabs(vi - wi) - fabs(vi) - fabs(wi);
      ++v1_it;
      ++v2_it;
    } else if (v1_it->first < v2_it->first) {
      v1_it = v1.lower_bound(v2_it->first);
    } else {
      v2_it = v2.lower_bound(v1_it->first);
    }
  }
  score = -score / 2.0;
  return score;
}

// double L2Scoring::score(...) const   ScoringObject.cpp:73-120
double scoreL2(const BowVector& v1, const BowVector& v2) {
  BowVector::const_iterator v1_it, v2_it;
  const BowVector::const_iterator v1_end = v1.end();
  const BowVector::const_iterator v2_end = v2.end();
  v1_it = v1.begin();
  v2_it = v2.begin();
  double score = 0;
  while (v1_it != v1_end && v2_it != v2_end) {
    const WordValue& vi = v1_it->second;
    const WordValue& wi = v2_it->second;
    if (v1_it->first == v2_it->first) {
      score += vi * wi;
      ++v1_it;
      ++v2_it;
    } else if (v1_it->first < v2_it->first) {
      v1_it = v1.lower_bound(v2_it->first);
    } else {
      v2_it = v2.lower_bound(v1_it->first);
    }
  }
  if (score >= 1)
    score = 1.0;
  else
    score = 1.0 - sqrt(1.0 - score);
  return score;
}

// double ChiSquareScoring::score(...) const   ScoringObject.cpp:125-170
double scoreChi(const BowVector& v1, const BowVector& v2) {
  BowVector::const_iterator v1_it, v2_it;
  const BowVector::const_iterator v1_end = v1.end();
  const BowVector::const_iterator v2_end = v2.end();
  v1_it = v1.begin();
  v2_it = v2.begin();
  double score = 0;
  while (v1_it != v1_end && v2_it != v2_end) {
    const WordValue& vi = v1_it->second;
    const WordValue& wi = v2_it->second;
    if (v1_it->first == v2_it->first) {
      if (vi + wi != 0.0) score += vi * wi / (vi + wi);
      ++v1_it;
      ++v2_it;
    } else if (v1_it->first < v2_it->first) {
      v1_it = v1.lower_bound(v2_it->first);
    } else {
      v2_it = v2.lower_bound(v1_it->first);
    }
  }
  score = 2. * score;
  return score;
}

// double DotProductScoring::score(...) const   ScoringObject.cpp:271-311
double scoreDot(const BowVector& v1, const BowVector& v2) {
  BowVector::const_iterator v1_it, v2_it;
  const BowVector::const_iterator v1_end = v1.end();
  const BowVector::const_iterator v2_end = v2.end();
  v1_it = v1.begin();
  v2_it = v2.begin();
  double score = 0;
  while (v1_it != v1_end && v2_it != v2_end) {
    const WordValue& vi = v1_it->second;
    const WordValue& wi = v2_it->second;
    if (v1_it->first == v2_it->first) {
      score += vi * wi;
      ++v1_it;
      ++v2_it;
    } else if (v1_it->first < v2_it->first) {
      v1_it = v1.lower_bound(v2_it->first);
    } else {
      v2_it = v2.lower_bound(v1_it->first);
    }
  }
  return score;
}

// ---- the model: what KeyFrameDatabase.cc touches of a KeyFrame (include/KeyFrame.h:574, 613-628) and of a Frame -------------
struct KF {
  long unsigned int mnId = 0;
  BowVector mBowVec;
  // KeyFrame.cc:44 zeroes the two queries and the two word counts; the two scores are left uninitialised there, 0 here
  long unsigned int mnLoopQuery = 0;
  int mnLoopWords = 0;
  float mLoopScore = 0;
  long unsigned int mnRelocQuery = 0;
  int mnRelocWords = 0;
  float mRelocScore = 0;
  bool bad = false;
  int index = 0;                  // position in Db::kfs (the C interface names keyframes by it)
  std::set<KF*> connected;        // GetConnectedKeyFrames()
  std::vector<KF*> covisible;     // mvpOrderedConnectedKeyFrames: GetVectorCovisibleKeyFrames(), GetBestCovisibilityKeyFrames(N)
  std::set<KF*> GetConnectedKeyFrames() { return connected; }
  std::vector<KF*> GetVectorCovisibleKeyFrames() { return covisible; }
  std::vector<KF*> GetBestCovisibilityKeyFrames(const int& N) {   // KeyFrame.cc: the first N of the ordered list
    if ((int)covisible.size() < N) return covisible;
    return std::vector<KF*>(covisible.begin(), covisible.begin() + N);
  }
  bool isBad() { return bad; }
};
struct FrameModel {
  long unsigned int mnId = 0;
  BowVector mBowVec;
};

enum { C_CANDIDATES, C_DUPLICATES, C_STALE, C_CONNECTED_SKIPS, C_BEST_OTHER, C_UNUSED, C_MAXCOMMON, C_MINCOMMON, C_N };

struct Db {
  int scoring = 0;
  size_t nWords = 0;
  std::vector<std::list<KF*> > mvInvertedFile;
  std::vector<KF*> kfs;
  long counters[C_N] = {0};
  ~Db() { for (KF* k : kfs) delete k; }

  double score(const BowVector& a, const BowVector& b) const {   // mpVoc->score -> m_scoring_object->score
    switch (scoring) {
      case 0: return scoreL1(a, b);
      case 1: return scoreL2(a, b);
      case 2: return scoreChi(a, b);
      default: return scoreDot(a, b);
    }
  }

  // KeyFrameDatabase.cc:38-44
  void add(KF* pKF) {
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++)
      mvInvertedFile[vit->first].push_back(pKF);
  }
  // KeyFrameDatabase.cc:46-65
  void erase(KF* pKF) {
    for (BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) {
      std::list<KF*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KF*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
        if (pKF == *lit) {
          lKFs.erase(lit);
          break;
        }
      }
    }
  }
  // KeyFrameDatabase.cc:67-71
  void clear() {
    mvInvertedFile.clear();
    mvInvertedFile.resize(nWords);
  }

  // KeyFrameDatabase.cc:74-197
  std::vector<KF*> DetectLoopCandidates(KF* pKF, float minScore) {
    std::set<KF*> spConnectedKeyFrames = pKF->GetConnectedKeyFrames();
    std::list<KF*> lKFsSharingWords;
    {
      for (BowVector::const_iterator vit = pKF->mBowVec.begin(), vend = pKF->mBowVec.end(); vit != vend; vit++) {
        std::list<KF*>& lKFs = mvInvertedFile[vit->first];
        for (std::list<KF*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
          KF* pKFi = *lit;
          if (pKFi->mnLoopQuery != pKF->mnId) {
            pKFi->mnLoopWords = 0;
            if (!spConnectedKeyFrames.count(pKFi)) {
              pKFi->mnLoopQuery = pKF->mnId;
              lKFsSharingWords.push_back(pKFi);
            } else
              counters[C_CONNECTED_SKIPS]++;   // (counter)
          }
          pKFi->mnLoopWords++;
        }
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KF*>();
    std::list<std::pair<float, KF*> > lScoreAndMatch;
    int maxCommonWords = 0;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      if ((*lit)->mnLoopWords > maxCommonWords) maxCommonWords = (*lit)->mnLoopWords;
    }
    int minCommonWords = maxCommonWords * 0.8f;
    counters[C_MAXCOMMON] = maxCommonWords; counters[C_MINCOMMON] = minCommonWords;   // (counter)
    int nscores = 0;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      KF* pKFi = *lit;
      if (pKFi->mnLoopWords > minCommonWords) {
        nscores++;
        float si = score(pKF->mBowVec, pKFi->mBowVec);
        pKFi->mLoopScore = si;
        if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KF*>();
    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = minScore;
    for (std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KF* pKFi = it->second;
      std::vector<KF*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = it->first;
      KF* pBestKF = pKFi;
      for (std::vector<KF*>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
        KF* pKF2 = *vit;
        if (pKF2->mnLoopQuery == pKF->mnId && pKF2->mnLoopWords > minCommonWords) {
          accScore += pKF2->mLoopScore;
          if (pKF2->mLoopScore > bestScore) {
            pBestKF = pKF2;
            bestScore = pKF2->mLoopScore;
          }
        }
      }
      if (pBestKF != pKFi) counters[C_BEST_OTHER]++;   // (counter)
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KF*> spAlreadyAddedKF;
    std::vector<KF*> vpLoopCandidates;
    vpLoopCandidates.reserve(lAccScoreAndMatch.size());
    for (std::list<std::pair<float, KF*> >::iterator it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
      if (it->first > minScoreToRetain) {
        KF* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpLoopCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        } else
          counters[C_DUPLICATES]++;   // (counter)
      }
    }
    counters[C_CANDIDATES] += (long)vpLoopCandidates.size();   // (counter)
    return vpLoopCandidates;
  }

  // KeyFrameDatabase.cc:199-334 (the `verbose` printing left out)
  std::vector<KF*> DetectRelocalizationCandidates(FrameModel* F) {
    std::list<KF*> lKFsSharingWords;
    {
      for (BowVector::const_iterator vit = F->mBowVec.begin(), vend = F->mBowVec.end(); vit != vend; vit++) {
        std::list<KF*>& lKFs = mvInvertedFile[vit->first];
        for (std::list<KF*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
          KF* pKFi = *lit;
          if (pKFi->mnRelocQuery != F->mnId) {
            pKFi->mnRelocWords = 0;
            pKFi->mnRelocQuery = F->mnId;
            lKFsSharingWords.push_back(pKFi);
          }
          pKFi->mnRelocWords++;
        }
      }
    }
    if (lKFsSharingWords.empty()) return std::vector<KF*>();
    int maxCommonWords = 0;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      if ((*lit)->mnRelocWords > maxCommonWords) maxCommonWords = (*lit)->mnRelocWords;
    }
    int minCommonWords = maxCommonWords * 0.8f;
    counters[C_MAXCOMMON] = maxCommonWords; counters[C_MINCOMMON] = minCommonWords;   // (counter)
    std::list<std::pair<float, KF*> > lScoreAndMatch;
    int nscores = 0;
    std::set<KF*> scoredNow;   // (counter)
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(), lend = lKFsSharingWords.end(); lit != lend; lit++) {
      KF* pKFi = *lit;
      if (pKFi->mnRelocWords > minCommonWords) {
        nscores++;
        float si = score(F->mBowVec, pKFi->mBowVec);
        pKFi->mRelocScore = si;
        scoredNow.insert(pKFi);   // (counter)
        lScoreAndMatch.push_back(std::make_pair(si, pKFi));
      }
    }
    if (lScoreAndMatch.empty()) return std::vector<KF*>();
    std::list<std::pair<float, KF*> > lAccScoreAndMatch;
    float bestAccScore = 0;
    for (std::list<std::pair<float, KF*> >::iterator it = lScoreAndMatch.begin(), itend = lScoreAndMatch.end(); it != itend; it++) {
      KF* pKFi = it->second;
      std::vector<KF*> vpNeighs = pKFi->GetBestCovisibilityKeyFrames(10);
      float bestScore = it->first;
      float accScore = bestScore;
      KF* pBestKF = pKFi;
      for (std::vector<KF*>::iterator vit = vpNeighs.begin(), vend = vpNeighs.end(); vit != vend; vit++) {
        KF* pKF2 = *vit;
        if (pKF2->mnRelocQuery != F->mnId) continue;
        if (!scoredNow.count(pKF2) && pKF2->mRelocScore != 0) counters[C_STALE]++;   // (counter) a score of an earlier query
        accScore += pKF2->mRelocScore;
        if (pKF2->mRelocScore > bestScore) {
          pBestKF = pKF2;
          bestScore = pKF2->mRelocScore;
        }
      }
      if (pBestKF != pKFi) counters[C_BEST_OTHER]++;   // (counter)
      lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
      if (accScore > bestAccScore) bestAccScore = accScore;
    }
    float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KF*> spAlreadyAddedKF;
    std::vector<KF*> vpRelocCandidates;
    vpRelocCandidates.reserve(lAccScoreAndMatch.size());
    for (std::list<std::pair<float, KF*> >::iterator it = lAccScoreAndMatch.begin(), itend = lAccScoreAndMatch.end(); it != itend; it++) {
      const float& si = it->first;
      if (si > minScoreToRetain) {
        KF* pKFi = it->second;
        if (!spAlreadyAddedKF.count(pKFi)) {
          vpRelocCandidates.push_back(pKFi);
          spAlreadyAddedKF.insert(pKFi);
        } else
          counters[C_DUPLICATES]++;   // (counter)
      }
    }
    counters[C_CANDIDATES] += (long)vpRelocCandidates.size();   // (counter)
    return vpRelocCandidates;
  }

  // LoopClosing.cc:125-140
  float minCovisibleScore(KF* mpCurrentKF) {
    const std::vector<KF*> vpConnectedKeyFrames = mpCurrentKF->GetVectorCovisibleKeyFrames();
    const BowVector& CurrentBowVec = mpCurrentKF->mBowVec;
    float minScore = 1;
    for (size_t i = 0; i < vpConnectedKeyFrames.size(); i++) {
      KF* pKF = vpConnectedKeyFrames[i];
      if (pKF->isBad()) continue;
      const BowVector& BowVec = pKF->mBowVec;
      float score = this->score(CurrentBowVec, BowVec);
      if (score < minScore) minScore = score;
    }
    return minScore;
  }

  // The walk of :85-104 / :207-222 alone, with no member of any keyframe read or written: the keyframes sharing a word with v in
  // order of first encounter, their common-word counts and mpVoc->score(v, keyframe) of each.  (What orbfe_kfdb_query returns.)
  int sharing(const BowVector& v, int* out, int* common, double* scores, int cap) {
    std::list<KF*> lKFsSharingWords;
    std::map<KF*, int> words;
    for (BowVector::const_iterator vit = v.begin(), vend = v.end(); vit != vend; vit++) {
      std::list<KF*>& lKFs = mvInvertedFile[vit->first];
      for (std::list<KF*>::iterator lit = lKFs.begin(), lend = lKFs.end(); lit != lend; lit++) {
        KF* pKFi = *lit;
        if (!words.count(pKFi)) {
          words[pKFi] = 0;
          lKFsSharingWords.push_back(pKFi);
        }
        words[pKFi]++;
      }
    }
    int n = 0;
    for (std::list<KF*>::iterator lit = lKFsSharingWords.begin(); lit != lKFsSharingWords.end(); lit++, n++) {
      if (n >= cap) continue;
      out[n] = index(*lit);
      common[n] = words[*lit];
      if (scores) scores[n] = score(v, (*lit)->mBowVec);
    }
    return n;
  }
  int index(KF* k) const { return k->index; }
};

BowVector bow(const unsigned* words, const double* values, int n) {
  BowVector v;
  for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair(words[i], values[i]));
  return v;
}
int put(const std::vector<KF*>& r, Db* d, int* out, int cap) {
  for (size_t i = 0; i < r.size() && (int)i < cap; i++) out[i] = d->index(r[i]);
  return (int)r.size();
}

}  // namespace

extern "C" {

void* kref_create(int n_words, int scoring) {
  Db* d = new Db;
  d->scoring = scoring;
  d->nWords = (size_t)n_words;
  d->mvInvertedFile.resize(d->nWords);   // KeyFrameDatabase.cc:31-35
  return d;
}
void kref_destroy(void* h) { delete (Db*)h; }
// a model keyframe (not yet in the database); returns its index
int kref_new_kf(void* h, uint64_t mnId, const unsigned* words, const double* values, int n) {
  Db* d = (Db*)h;
  KF* k = new KF;
  k->mnId = (long unsigned int)mnId;
  k->mBowVec = bow(words, values, n);
  k->index = (int)d->kfs.size();
  d->kfs.push_back(k);
  return (int)d->kfs.size() - 1;
}
void kref_set_connected(void* h, int kf, const int* others, int n) {
  Db* d = (Db*)h;
  d->kfs[kf]->connected.clear();
  for (int i = 0; i < n; i++) d->kfs[kf]->connected.insert(d->kfs[others[i]]);
}
void kref_set_covisible(void* h, int kf, const int* others, int n) {
  Db* d = (Db*)h;
  d->kfs[kf]->covisible.clear();
  for (int i = 0; i < n; i++) d->kfs[kf]->covisible.push_back(d->kfs[others[i]]);
}
void kref_set_bad(void* h, int kf, int bad) { ((Db*)h)->kfs[kf]->bad = bad != 0; }
void kref_add(void* h, int kf) { Db* d = (Db*)h; d->add(d->kfs[kf]); }
void kref_erase(void* h, int kf) { Db* d = (Db*)h; d->erase(d->kfs[kf]); }
void kref_clear(void* h) { ((Db*)h)->clear(); }
int kref_detect_loop(void* h, int kf, float minScore, int* out, int cap) {
  Db* d = (Db*)h;
  return put(d->DetectLoopCandidates(d->kfs[kf], minScore), d, out, cap);
}
int kref_detect_reloc(void* h, uint64_t frame_id, const unsigned* words, const double* values, int n, int* out, int cap) {
  Db* d = (Db*)h;
  FrameModel F;
  F.mnId = (long unsigned int)frame_id;
  F.mBowVec = bow(words, values, n);
  return put(d->DetectRelocalizationCandidates(&F), d, out, cap);
}
float kref_min_covisible_score(void* h, int kf) { Db* d = (Db*)h; return d->minCovisibleScore(d->kfs[kf]); }
int kref_sharing(void* h, const unsigned* words, const double* values, int n, int* out, int* common, double* scores, int cap) {
  return ((Db*)h)->sharing(bow(words, values, n), out, common, scores, cap);
}
double kref_score(void* h, const unsigned* words, const double* values, int n, int kf) {
  Db* d = (Db*)h;
  return d->score(bow(words, values, n), d->kfs[kf]->mBowVec);
}
// {mnLoopQuery, mnRelocQuery}, {mnLoopWords, mnRelocWords}, {mLoopScore, mRelocScore}
void kref_members(void* h, int kf, uint64_t* queries, int32_t* words, float* scores) {
  const KF* k = ((Db*)h)->kfs[kf];
  queries[0] = k->mnLoopQuery; queries[1] = k->mnRelocQuery;
  words[0] = k->mnLoopWords; words[1] = k->mnRelocWords;
  scores[0] = k->mLoopScore; scores[1] = k->mRelocScore;
}
// candidates, duplicates, stale-score uses, connected skips, pBestKF != pKFi, (unused), last maxCommonWords, last minCommonWords
void kref_counters(void* h, long* out) {
  for (int i = 0; i < C_N; i++) out[i] = ((Db*)h)->counters[i];
}

}  // extern "C"
