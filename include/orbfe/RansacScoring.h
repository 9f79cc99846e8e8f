// RansacScoring.h -- the host side of orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses (include/orbfe.h): what
// Sim3Solver (reference src/Sim3Solver.cc) and PnPsolver (src/PnPsolver.cc) do around their CheckInliers, without cv or os1 headers.
//
//   * Packing.  Sim3Row / PnPRow build one correspondence row from what the solvers' constructors hold (Sim3Solver.cc:62-112,
//     PnPsolver.cc:83-105, :158-160); Sim3Round / PnPRound collect the segments (solvers) and hypotheses of one scoring call.
//   * Sim3RansacWalk / PnPRansacWalk carry the state the solvers keep between two iterate() calls and replay
//     Sim3Solver::iterate (:143-210) / PnPsolver::iterate (:169-263) over the counts and masks of the next block of hypotheses.
//     The selection is sequential and costs nothing, so it stays on the host, in the reference's order.
//
// The application keeps drawing the minimal sets and solving them (Sim3Solver::ComputeSim3 with cv::eigen, EPnP's compute_pose):
// hypotheses() says how many the next iterate(nIterations) may look at, the application computes that many, one scoring call
// scores them for all solvers of the round, and iterate() consumes them.  Hypotheses the loop did not reach (it returned early)
// are dropped, as their random draws would never have happened in the reference.  INTEGRATION.md has the call site.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../orbfe.h"

namespace orbfe {

// ---- packing --------------------------------------------------------------------------------------------------------------
// mvnMaxError1.push_back(9.210*sigmaSquare1) into a vector<size_t> (Sim3Solver.cc:87-88): a double product, truncated; the
// comparison `err1<mvnMaxError1[i]` converts it to float.
inline float Sim3MaxError(float sigmaSquare) { return (float)(size_t)(9.210 * sigmaSquare); }
// mvMaxError[i] = mvSigma2[i]*th2 (PnPsolver.cc:160): a float product
inline float PnPMaxError(float sigma2, float th2) { return sigma2 * th2; }

// One row of orbfe_score_sim3_hypotheses' corr.  X3Dc1 / X3Dc2: mvX3Dc1[i] / mvX3Dc2[i]; P1im1 / P2im2: mvP1im1[i] / mvP2im2[i]
// (FromCameraToImage's results); sigmaSquare1 / 2: mvLevelSigma2 of the two keypoints' octaves.
inline void Sim3Row(float row[12], const float X3Dc1[3], const float X3Dc2[3], const float P1im1[2], const float P2im2[2], float sigmaSquare1,
                    float sigmaSquare2) {
  for (int i = 0; i < 3; i++) { row[i] = X3Dc1[i]; row[3 + i] = X3Dc2[i]; }
  row[6] = P1im1[0]; row[7] = P1im1[1];
  row[8] = P2im2[0]; row[9] = P2im2[1];
  row[10] = Sim3MaxError(sigmaSquare1);
  row[11] = Sim3MaxError(sigmaSquare2);
}
// One row of orbfe_score_pnp_hypotheses' corr: mvP3Dw[i], mvP2D[i], mvSigma2[i] and SetRansacParameters' th2.
inline void PnPRow(float row[6], float X, float Y, float Z, float u, float v, float sigma2, float th2 = 5.991f) {
  row[0] = X; row[1] = Y; row[2] = Z; row[3] = u; row[4] = v;
  row[5] = PnPMaxError(sigma2, th2);
}

inline size_t RansacWords(int n) { return ((size_t)n + 63) / 64; }
inline bool RansacBit(const uint64_t* words, int i) { return (words[i >> 6] >> (i & 63)) & 1u; }

// The segments and hypotheses of one scoring call and its results.  ROW: floats per correspondence; CAM: camera type and count;
// HYP: hypothesis scalar type, 12 per array, NARR arrays (T12 and T21, or Rt alone).
template <int ROW, class CamT, int CAM, class HypT, int NARR>
struct RansacRound {
  std::vector<int32_t> segOff, hypSeg, counts;
  std::vector<float> corr;
  std::vector<CamT> cams;
  std::vector<HypT> hyp[NARR];
  std::vector<int64_t> maskOff;    // packed: where hypothesis k's words start in masks
  std::vector<uint64_t> masks;

  RansacRound() : segOff(1, 0) {}
  void clear() { segOff.assign(1, 0); hypSeg.clear(); counts.clear(); corr.clear(); cams.clear(); maskOff.clear(); masks.clear(); for (int a = 0; a < NARR; a++) hyp[a].clear(); }
  int segments() const { return (int)segOff.size() - 1; }
  int hypotheses() const { return (int)hypSeg.size(); }
  int segmentSize(int s) const { return segOff[s + 1] - segOff[s]; }
  // one solver: its n rows (ROW floats each) and its camera(s); returns the segment's index
  int addSegment(const float* rows, int n, const CamT* cam) {
    if (n > 0) corr.insert(corr.end(), rows, rows + (size_t)ROW * (size_t)n);
    cams.insert(cams.end(), cam, cam + CAM);
    segOff.push_back(segOff.back() + n);
    return segments() - 1;
  }
  // one hypothesis of segment s: 12 scalars per array; returns its index k
  int addHypothesis(int s, const HypT* a, const HypT* b = 0) {
    hypSeg.push_back(s);
    hyp[0].insert(hyp[0].end(), a, a + 12);
    if (NARR > 1) hyp[NARR - 1].insert(hyp[NARR - 1].end(), b, b + 12);
    return hypotheses() - 1;
  }
  const uint64_t* mask(int k) const { return masks.empty() ? (const uint64_t*)0 : masks.data() + maskOff[k]; }
  // sizes the outputs; false for nothing to score
  bool prepare() {
    const int K = hypotheses();
    counts.assign((size_t)K, 0);
    maskOff.assign((size_t)K, 0);
    size_t at = 0;
    for (int k = 0; k < K; k++) { maskOff[k] = (int64_t)at; at += RansacWords(segmentSize(hypSeg[k])); }
    masks.assign(at, 0);
    return K > 0;
  }
};

struct Sim3Round : RansacRound<12, float, 8, float, 2> {
  // ORBFE_OK or the call's error; a round without hypotheses is ORBFE_OK.  Score: anything callable like
  // orbfe_score_sim3_hypotheses without the matcher, so that the walks can run on a CPU.
  template <class Score>
  int scoreWith(Score&& score) {
    if (!prepare()) return ORBFE_OK;
    return score(segments(), segOff.data(), corr.data(), cams.data(), hypotheses(), hypSeg.data(), hyp[0].data(), hyp[1].data(), counts.data(),
                 (const int64_t*)0, masks.data());
  }
  int score(orbfe_matcher* m) {
    return scoreWith([m](int ns, const int32_t* so, const float* c, const float* cam, int nh, const int32_t* hs, const float* a, const float* b,
                         int32_t* cnt, const int64_t* mo, uint64_t* mk) { return orbfe_score_sim3_hypotheses(m, ns, so, c, cam, nh, hs, a, b, cnt, mo, mk); });
  }
};

struct PnPRound : RansacRound<6, double, 4, double, 1> {
  template <class Score>
  int scoreWith(Score&& score) {
    if (!prepare()) return ORBFE_OK;
    return score(segments(), segOff.data(), corr.data(), cams.data(), hypotheses(), hypSeg.data(), hyp[0].data(), counts.data(), (const int64_t*)0,
                 masks.data());
  }
  int score(orbfe_matcher* m) {
    return scoreWith([m](int ns, const int32_t* so, const float* c, const double* cam, int nh, const int32_t* hs, const double* rt, int32_t* cnt,
                         const int64_t* mo, uint64_t* mk) { return orbfe_score_pnp_hypotheses(m, ns, so, c, cam, nh, hs, rt, cnt, mo, mk); });
  }
};

// ---- Sim3Solver::iterate ----------------------------------------------------------------------------------------------------
struct Sim3RansacWalk {
  int N;                               // correspondences the constructor kept (mvpMapPoints1.size())
  int mN1;                             // vpMatched12.size(): the length of vbInliers
  std::vector<int> mvnIndices1;        // [N]
  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts;
  int mnIterations, mnBestInliers;
  int bestHypothesis;                  // the caller's tag of the hypothesis behind mBestT12; -1: none yet
  std::vector<uint64_t> mvbBestInliers;   // its mask words

  Sim3RansacWalk(int mN1_, const std::vector<int>& indices1)
      : N((int)indices1.size()), mN1(mN1_), mvnIndices1(indices1), mnIterations(0), mnBestInliers(0), bestHypothesis(-1) {
    SetRansacParameters();
  }

  // Sim3Solver.cc:117-141
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    if (N > 0) {   // (with N == 0 the reference divides by zero here; iterate() then gives up before it looks at mRansacMaxIts)
      float epsilon = (float)mRansacMinInliers / N;
      int nIterations;
      if (mRansacMinInliers == N) nIterations = 1;
      else {
        const double it = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3)));
        nIterations = it > -2147483649.0 && it < 2147483648.0 ? (int)it : -2147483647 - 1;   // (out of range or NaN: what x86's conversion gives)
      }
      mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    }
    mnIterations = 0;
  }

  // How many hypotheses the next iterate(nIterations) looks at, at the most (0: it returns at once).
  int hypotheses(int nIterations) const {
    if (N < mRansacMinInliers) return 0;
    const int left = mRansacMaxIts - mnIterations;
    return std::max(0, std::min(left, nIterations));
  }

  // Sim3Solver::iterate over the next hypotheses of this solver: counts[j] and the words at masks + maskOff[j] (or, with
  // maskOff == NULL, at masks + j * RansacWords(N)), j < nGiven >= hypotheses(nIterations); tags[j] (or firstTag + j) names
  // hypothesis j towards the caller.  Returns the tag of the hypothesis whose mT12i the reference returns, or -1 for cv::Mat();
  // *consumed: how many hypotheses the loop looked at.
  int iterate(int nIterations, const int32_t* counts, const uint64_t* masks, const int64_t* maskOff, int nGiven, int firstTag, bool& bNoMore,
              std::vector<bool>& vbInliers, int& nInliers, int* consumed = 0) {
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    if (consumed) *consumed = 0;
    if (N < mRansacMinInliers) {
      bNoMore = true;
      return -1;
    }
    const size_t W = RansacWords(N);
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
      if (nCurrentIterations >= nGiven) return -2;   // fewer hypotheses than hypotheses(nIterations): the caller's error
      const int j = nCurrentIterations;
      nCurrentIterations++;
      mnIterations++;
      if (consumed) *consumed = nCurrentIterations;
      const int mnInliersi = counts[j];
      const uint64_t* mvbInliersi = masks + (maskOff ? (size_t)maskOff[j] : (size_t)j * W);
      if (mnInliersi >= mnBestInliers) {
        mvbBestInliers.assign(mvbInliersi, mvbInliersi + W);
        mnBestInliers = mnInliersi;
        bestHypothesis = firstTag + j;
        if (mnInliersi > mRansacMinInliers) {
          nInliers = mnInliersi;
          for (int i = 0; i < N; i++)
            if (RansacBit(mvbInliersi, i)) vbInliers[mvnIndices1[i]] = true;
          return bestHypothesis;
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;
    return -1;
  }
};

// ---- PnPsolver::iterate -------------------------------------------------------------------------------------------------------
constexpr int kPnPNone = -1;       // cv::Mat()
constexpr int kPnPRefined = -2;    // mRefinedTcw: the hypothesis the last Refine callback scored

struct PnPRansacWalk {
  int N;                               // mvP2D.size()
  int nMatches;                        // mvpMapPointMatches.size(): the length of vbInliers
  std::vector<int> mvKeyPointIndices;  // [N]
  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts, mRansacMinSet;
  float mRansacEpsilon;
  int mnIterations, mnBestInliers;
  int bestHypothesis;                  // the caller's tag of the hypothesis behind mBestTcw; -1: none yet
  std::vector<uint64_t> mvbBestInliers;
  int mnRefinedInliers;
  std::vector<uint64_t> mvbRefinedInliers;

  PnPRansacWalk(int nMatches_, const std::vector<int>& keyPointIndices)
      : N((int)keyPointIndices.size()), nMatches(nMatches_), mvKeyPointIndices(keyPointIndices), mnIterations(0), mnBestInliers(0),
        bestHypothesis(-1), mnRefinedInliers(0) {
    SetRansacParameters();
  }

  // PnPsolver.cc:125-161 without mvMaxError, which PnPRow computes with the same th2
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f) {
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    mRansacEpsilon = epsilon;
    mRansacMinSet = minSet;
    int nMinInliers = N * mRansacEpsilon;
    if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    if (N > 0) {   // (with N == 0 the reference divides by zero here; iterate() then gives up before it looks at mRansacMaxIts)
      if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
      int nIterations;
      if (mRansacMinInliers == N) nIterations = 1;
      else {
        const double it = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(mRansacEpsilon, 3)));
        nIterations = it > -2147483649.0 && it < 2147483648.0 ? (int)it : -2147483647 - 1;   // (out of range or NaN: what x86's conversion gives)
      }
      mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    }
  }

  // How many hypotheses the next iterate(nIterations) looks at, at the most.  The loop condition is an OR (PnPsolver.cc:186):
  // it goes on while EITHER budget lasts.
  int hypotheses(int nIterations) const {
    if (N < mRansacMinInliers) return 0;
    return std::max(0, std::max(mRansacMaxIts - mnIterations, nIterations));
  }

  // PnPsolver::iterate over the next hypotheses of this solver (arguments as Sim3RansacWalk::iterate).
  // refine(bestMask, count, mask): PnPsolver::Refine up to its CheckInliers -- the application solves EPnP on the correspondences
  // set in bestMask (RansacWords(N) words), scores the result (an n_hyp = 1 call) and stores its count and mask words.
  // Returns kPnPRefined (mRefinedTcw), the tag of the best hypothesis (mBestTcw, when the iterations ran out) or kPnPNone.
  template <class Refine>
  int iterate(int nIterations, const int32_t* counts, const uint64_t* masks, const int64_t* maskOff, int nGiven, int firstTag, bool& bNoMore,
              std::vector<bool>& vbInliers, int& nInliers, Refine&& refine, int* consumed = 0) {
    bNoMore = false;
    vbInliers.clear();
    nInliers = 0;
    if (consumed) *consumed = 0;
    if (N < mRansacMinInliers) {
      bNoMore = true;
      return kPnPNone;
    }
    const size_t W = RansacWords(N);
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {
      if (nCurrentIterations >= nGiven) return -3;   // fewer hypotheses than hypotheses(nIterations): the caller's error
      const int j = nCurrentIterations;
      nCurrentIterations++;
      mnIterations++;
      if (consumed) *consumed = nCurrentIterations;
      const int mnInliersi = counts[j];
      const uint64_t* mvbInliersi = masks + (maskOff ? (size_t)maskOff[j] : (size_t)j * W);
      if (mnInliersi >= mRansacMinInliers) {
        if (mnInliersi > mnBestInliers) {
          mvbBestInliers.assign(mvbInliersi, mvbInliersi + W);
          mnBestInliers = mnInliersi;
          bestHypothesis = firstTag + j;
        }
        // Refine() (:265-310)
        mvbRefinedInliers.assign(W, 0);
        mnRefinedInliers = 0;
        refine(mvbBestInliers, mnRefinedInliers, mvbRefinedInliers);
        if (mnRefinedInliers > mRansacMinInliers) {
          nInliers = mnRefinedInliers;
          vbInliers = std::vector<bool>(nMatches, false);
          for (int i = 0; i < N; i++)
            if (RansacBit(mvbRefinedInliers.data(), i)) vbInliers[mvKeyPointIndices[i]] = true;
          return kPnPRefined;
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) {
      bNoMore = true;
      if (mnBestInliers >= mRansacMinInliers) {
        nInliers = mnBestInliers;
        vbInliers = std::vector<bool>(nMatches, false);
        for (int i = 0; i < N; i++)
          if (RansacBit(mvbBestInliers.data(), i)) vbInliers[mvKeyPointIndices[i]] = true;
        return bestHypothesis;
      }
    }
    return kPnPNone;
  }
};

}  // namespace orbfe
