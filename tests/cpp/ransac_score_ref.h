// ransac_score_ref.h -- declarations of the restatement tests/cpp/ransac_score_ref.cpp.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

extern "C" {
// Sim3Solver::CheckInliers / PnPsolver::CheckInliers for one hypothesis over n correspondences; returns mnInliersi
int rsr_check_sim3(const float* corr, int n, const float* cams8, const float* T12, const float* T21, uint8_t* inliers);
int rsr_check_pnp(const float* corr, int n, const double* cams4, const double* Rt, uint8_t* inliers);
// The same with the arguments of orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses without the matcher; 0, or -1 for a bad layout
int rsr_score_sim3(int n_seg, const int32_t* seg_off, const float* corr, const float* cams, int n_hyp, const int32_t* hyp_seg, const float* T12,
                   const float* T21, int32_t* counts, const int64_t* mask_off, uint64_t* masks);
int rsr_score_pnp(int n_seg, const int32_t* seg_off, const float* corr, const double* cams, int n_hyp, const int32_t* hyp_seg, const double* Rt,
                  int32_t* counts, const int64_t* mask_off, uint64_t* masks);
}

// Sim3Solver with "ComputeSim3 on a random minimal set" replaced by "take the next hypothesis of a list".
struct RefSim3Solver {
  int N, mN1;
  std::vector<int> mvnIndices1;
  std::vector<float> corr, cams, T12, T21;   // 12 N, 8, 12 per hypothesis each
  size_t next = 0;                           // the hypothesis the next iteration takes
  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts, mnIterations = 0, mnBestInliers = 0, mnInliersi = 0;
  int best = -1;                             // the list index of mBestT12
  std::vector<bool> mvbInliersi, mvbBestInliers;
  RefSim3Solver(int mN1_, const std::vector<int>& indices1, const float* corr_, const float* cams8, const float* T12_, const float* T21_, int n_hyp);
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);
  // the list index of the hypothesis whose mT12i is returned, -1 for cv::Mat(), -9 when the list ran out
  int iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);
  void CheckInliers(size_t h);
};

struct RefPnPSolver {
  int N, nMatches;
  std::vector<int> mvKeyPointIndices;
  std::vector<float> corr;
  std::vector<double> cams, Rt, refinedRt;   // 4; 12 per hypothesis; 12 per Refine() call
  size_t next = 0, nextRefined = 0;
  double mRansacProb;
  int mRansacMinInliers, mRansacMaxIts, mRansacMinSet, mnIterations = 0, mnBestInliers = 0, mnInliersi = 0, mnRefinedInliers = 0;
  float mRansacEpsilon;
  int best = -1;
  std::vector<bool> mvbInliersi, mvbBestInliers, mvbRefinedInliers;
  RefPnPSolver(int nMatches_, const std::vector<int>& keyPointIndices, const float* corr_, const double* cams4, const double* Rt_, int n_hyp,
               const double* refined, int n_refined);
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f);
  // -2: mRefinedTcw; >= 0: the list index of mBestTcw; -1: cv::Mat(); -9: a list ran out
  int iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers);
  void CheckInliers(const double* rt);
  int Refine();   // 1 / 0 as the reference's bool, -9 when the refined list ran out
};
