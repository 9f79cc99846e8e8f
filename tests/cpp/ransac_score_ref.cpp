// ransac_score_ref.cpp -- a scalar restatement of the reference's two RANSAC inlier tests and of the loops around them, the
// yardstick of orbfe_score_sim3_hypotheses / orbfe_score_pnp_hypotheses and of include/orbfe/RansacScoring.h:
//   Sim3Solver::CheckInliers (src/Sim3Solver.cc:343-367) with Sim3Solver::Project (:385-406),
//   Sim3Solver::SetRansacParameters (:117-141), Sim3Solver::iterate (:143-210),
//   PnPsolver::CheckInliers (src/PnPsolver.cc:313-344), PnPsolver::SetRansacParameters (:125-161),
//   PnPsolver::iterate (:169-263), PnPsolver::Refine (:265-310).
// The minimal-set solve (ComputeSim3, compute_pose) is replaced by "take the next hypothesis from a list".  cv::Mat arithmetic
// goes through oracle/cv_small.h: Rcw*X + tcw is cvGemm3 (alpha = beta = 1), dist.dot(dist) is cvDot3 (with a third element of
// 0, which adds +0 to the double sum).  Built -O2 -ffp-contract=off.  TEST INFRASTRUCTURE ONLY.
#include "ransac_score_ref.h"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "cv_small.h"

namespace {

// Sim3Solver::Project for one point (:399-404).  T: the first 12 floats of the 4x4 Tcw; K: fx fy cx cy.
void project(const float* T, const float X[3], const float* K, float out[2]) {
  const float Rcw[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  const float tcw[3] = {T[3], T[7], T[11]};
  float P3Dc[3];
  cvGemm3(Rcw, X, 1.0, tcw, 1.0, P3Dc);
  const float invz = 1 / (P3Dc[2]);
  const float x = P3Dc[0] * invz;
  const float y = P3Dc[1] * invz;
  const float fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  out[0] = fx * x + cx;
  out[1] = fy * y + cy;
}

// one correspondence of Sim3Solver::CheckInliers (:353-359)
bool sim3_inlier(const float* r, const float* cams, const float* T12, const float* T21) {
  const float *X3Dc1 = r, *X3Dc2 = r + 3, *P1im1 = r + 6, *P2im2 = r + 8;
  const float maxError1 = r[10], maxError2 = r[11];   // (float)mvnMaxError1[i]: the comparison's conversion of the size_t
  float vP2im1[2], vP1im2[2];
  project(T12, X3Dc2, cams, vP2im1);
  project(T21, X3Dc1, cams + 4, vP1im2);
  const float dist1[3] = {P1im1[0] - vP2im1[0], P1im1[1] - vP2im1[1], 0.f};
  const float dist2[3] = {vP1im2[0] - P2im2[0], vP1im2[1] - P2im2[1], 0.f};
  const float err1 = (float)cvDot3(dist1, dist1);
  const float err2 = (float)cvDot3(dist2, dist2);
  return err1 < maxError1 && err2 < maxError2;
}

// one correspondence of PnPsolver::CheckInliers (:319-334).  Rt: mRi[3][3], mti[3].  cams: uc vc fu fv.
bool pnp_inlier(const float* r, const double* cams, const double* Rt) {
  const double(*mRi)[3] = reinterpret_cast<const double(*)[3]>(Rt);
  const double* mti = Rt + 9;
  const double uc = cams[0], vc = cams[1], fu = cams[2], fv = cams[3];
  struct { float x, y, z; } P3Dw = {r[0], r[1], r[2]};
  struct { float x, y; } P2D = {r[3], r[4]};
  const float maxError = r[5];

  float Xc = mRi[0][0] * P3Dw.x + mRi[0][1] * P3Dw.y + mRi[0][2] * P3Dw.z + mti[0];
  float Yc = mRi[1][0] * P3Dw.x + mRi[1][1] * P3Dw.y + mRi[1][2] * P3Dw.z + mti[1];
  float invZc = 1 / (mRi[2][0] * P3Dw.x + mRi[2][1] * P3Dw.y + mRi[2][2] * P3Dw.z + mti[2]);

  double ue = uc + fu * Xc * invZc;
  double ve = vc + fv * Yc * invZc;

  float distX = P2D.x - ue;
  float distY = P2D.y - ve;

  float error2 = distX * distX + distY * distY;
  return error2 < maxError;
}

int to_int(double v) { return v > -2147483649.0 && v < 2147483648.0 ? (int)v : -2147483647 - 1; }   // x86's double -> int

bool layout_ok(int n_seg, const int32_t* seg_off, int n_hyp, const int32_t* hyp_seg) {
  if (n_seg < 1 || n_hyp < 1 || !seg_off || !hyp_seg || seg_off[0] < 0) return false;
  for (int s = 0; s < n_seg; s++) if (seg_off[s + 1] < seg_off[s]) return false;
  for (int k = 0; k < n_hyp; k++) if (hyp_seg[k] < 0 || hyp_seg[k] >= n_seg) return false;
  return true;
}

template <class Check>
int score_all(int n_seg, const int32_t* seg_off, int n_hyp, const int32_t* hyp_seg, int32_t* counts, const int64_t* mask_off, uint64_t* masks, Check check) {
  if (!layout_ok(n_seg, seg_off, n_hyp, hyp_seg)) return -1;
  std::vector<uint8_t> inl;
  int64_t at = 0;
  for (int k = 0; k < n_hyp; k++) {
    const int s = hyp_seg[k], n = seg_off[s + 1] - seg_off[s];
    inl.assign((size_t)n + 1, 0);
    const int c = check(k, s, seg_off[s], n, inl.data());
    if (counts) counts[k] = c;
    const int64_t W = ((int64_t)n + 63) / 64;
    if (masks) {
      uint64_t* w = masks + (mask_off ? mask_off[k] : at);
      for (int64_t j = 0; j < W; j++) w[j] = 0;
      for (int i = 0; i < n; i++) if (inl[i]) w[i >> 6] |= 1ull << (i & 63);
    }
    at += W;
  }
  return 0;
}

}  // namespace

extern "C" {

int rsr_check_sim3(const float* corr, int n, const float* cams8, const float* T12, const float* T21, uint8_t* inliers) {
  int mnInliersi = 0;
  for (int i = 0; i < n; i++) {
    const bool in = sim3_inlier(corr + 12 * (size_t)i, cams8, T12, T21);
    inliers[i] = in;
    mnInliersi += in;
  }
  return mnInliersi;
}

int rsr_check_pnp(const float* corr, int n, const double* cams4, const double* Rt, uint8_t* inliers) {
  int mnInliersi = 0;
  for (int i = 0; i < n; i++) {
    const bool in = pnp_inlier(corr + 6 * (size_t)i, cams4, Rt);
    inliers[i] = in;
    mnInliersi += in;
  }
  return mnInliersi;
}

int rsr_score_sim3(int n_seg, const int32_t* seg_off, const float* corr, const float* cams, int n_hyp, const int32_t* hyp_seg, const float* T12,
                   const float* T21, int32_t* counts, const int64_t* mask_off, uint64_t* masks) {
  return score_all(n_seg, seg_off, n_hyp, hyp_seg, counts, mask_off, masks, [&](int k, int s, int first, int n, uint8_t* inl) {
    return rsr_check_sim3(corr + 12 * (size_t)first, n, cams + 8 * (size_t)s, T12 + 12 * (size_t)k, T21 + 12 * (size_t)k, inl);
  });
}

int rsr_score_pnp(int n_seg, const int32_t* seg_off, const float* corr, const double* cams, int n_hyp, const int32_t* hyp_seg, const double* Rt,
                  int32_t* counts, const int64_t* mask_off, uint64_t* masks) {
  return score_all(n_seg, seg_off, n_hyp, hyp_seg, counts, mask_off, masks, [&](int k, int s, int first, int n, uint8_t* inl) {
    return rsr_check_pnp(corr + 6 * (size_t)first, n, cams + 4 * (size_t)s, Rt + 12 * (size_t)k, inl);
  });
}

}  // extern "C"

// ---- Sim3Solver ---------------------------------------------------------------------------------------------------------------
RefSim3Solver::RefSim3Solver(int mN1_, const std::vector<int>& indices1, const float* corr_, const float* cams8, const float* T12_,
                             const float* T21_, int n_hyp)
    : N((int)indices1.size()), mN1(mN1_), mvnIndices1(indices1), corr(corr_, corr_ + 12 * indices1.size()), cams(cams8, cams8 + 8),
      T12(T12_, T12_ + 12 * (size_t)n_hyp), T21(T21_, T21_ + 12 * (size_t)n_hyp) {
  SetRansacParameters();
}

void RefSim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  mRansacMaxIts = maxIterations;

  mvbInliersi.resize(N);

  if (N > 0) {   // (the reference divides by N; with N == 0 iterate() gives up before it looks at mRansacMaxIts)
    float epsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N) nIterations = 1;
    else nIterations = to_int(std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3))));
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
  }
  mnIterations = 0;
}

void RefSim3Solver::CheckInliers(size_t h) {
  mnInliersi = 0;
  for (int i = 0; i < N; i++) {
    if (sim3_inlier(&corr[12 * (size_t)i], cams.data(), &T12[12 * h], &T21[12 * h])) {
      mvbInliersi[i] = true;
      mnInliersi++;
    } else
      mvbInliersi[i] = false;
  }
}

int RefSim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false;
  vbInliers = std::vector<bool>(mN1, false);
  nInliers = 0;

  if (N < mRansacMinInliers) {
    bNoMore = true;
    return -1;
  }

  int nCurrentIterations = 0;
  while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
    nCurrentIterations++;
    mnIterations++;

    if (12 * (next + 1) > T12.size()) return -9;
    const size_t h = next++;   // ComputeSim3(P3Dc1i,P3Dc2i)

    CheckInliers(h);

    if (mnInliersi >= mnBestInliers) {
      mvbBestInliers = mvbInliersi;
      mnBestInliers = mnInliersi;
      best = (int)h;

      if (mnInliersi > mRansacMinInliers) {
        nInliers = mnInliersi;
        for (int i = 0; i < N; i++)
          if (mvbInliersi[i]) vbInliers[mvnIndices1[i]] = true;
        return best;
      }
    }
  }

  if (mnIterations >= mRansacMaxIts) bNoMore = true;

  return -1;
}

// ---- PnPsolver ----------------------------------------------------------------------------------------------------------------
RefPnPSolver::RefPnPSolver(int nMatches_, const std::vector<int>& keyPointIndices, const float* corr_, const double* cams4, const double* Rt_,
                           int n_hyp, const double* refined, int n_refined)
    : N((int)keyPointIndices.size()), nMatches(nMatches_), mvKeyPointIndices(keyPointIndices), corr(corr_, corr_ + 6 * keyPointIndices.size()),
      cams(cams4, cams4 + 4), Rt(Rt_, Rt_ + 12 * (size_t)n_hyp) {
  if (n_refined > 0) refinedRt.assign(refined, refined + 12 * (size_t)n_refined);
  SetRansacParameters();
}

void RefPnPSolver::SetRansacParameters(double probability, int minInliers, int maxIterations, int minSet, float epsilon) {
  mRansacProb = probability;
  mRansacMinInliers = minInliers;
  mRansacMaxIts = maxIterations;
  mRansacEpsilon = epsilon;
  mRansacMinSet = minSet;

  mvbInliersi.resize(N);

  int nMinInliers = N * mRansacEpsilon;
  if (nMinInliers < mRansacMinInliers) nMinInliers = mRansacMinInliers;
  if (nMinInliers < minSet) nMinInliers = minSet;
  mRansacMinInliers = nMinInliers;

  if (N > 0) {   // (as above)
    if (mRansacEpsilon < (float)mRansacMinInliers / N) mRansacEpsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N) nIterations = 1;
    else nIterations = to_int(std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(mRansacEpsilon, 3))));
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
  }
  // mvMaxError[i] = mvSigma2[i]*th2 is column 5 of corr
}

void RefPnPSolver::CheckInliers(const double* rt) {
  mnInliersi = 0;
  for (int i = 0; i < N; i++) {
    if (pnp_inlier(&corr[6 * (size_t)i], cams.data(), rt)) {
      mvbInliersi[i] = true;
      mnInliersi++;
    } else {
      mvbInliersi[i] = false;
    }
  }
}

int RefPnPSolver::Refine() {
  // vIndices, add_correspondence, compute_pose(mRi, mti) on mvbBestInliers: the next refined hypothesis of the list
  if (12 * (nextRefined + 1) > refinedRt.size()) return -9;
  const double* rt = &refinedRt[12 * nextRefined++];

  CheckInliers(rt);

  mnRefinedInliers = mnInliersi;
  mvbRefinedInliers = mvbInliersi;

  if (mnInliersi > mRansacMinInliers) return 1;
  return 0;
}

int RefPnPSolver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers) {
  bNoMore = false;
  vbInliers.clear();
  nInliers = 0;

  if (N < mRansacMinInliers) {
    bNoMore = true;
    return -1;
  }

  int nCurrentIterations = 0;
  while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {
    nCurrentIterations++;
    mnIterations++;

    if (12 * (next + 1) > Rt.size()) return -9;
    const size_t h = next++;   // compute_pose(mRi, mti)

    CheckInliers(&Rt[12 * h]);

    if (mnInliersi >= mRansacMinInliers) {
      if (mnInliersi > mnBestInliers) {
        mvbBestInliers = mvbInliersi;
        mnBestInliers = mnInliersi;
        best = (int)h;
      }

      const int refined = Refine();
      if (refined < 0) return -9;
      if (refined) {
        nInliers = mnRefinedInliers;
        vbInliers = std::vector<bool>(nMatches, false);
        for (int i = 0; i < N; i++) {
          if (mvbRefinedInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
        }
        return -2;
      }
    }
  }

  if (mnIterations >= mRansacMaxIts) {
    bNoMore = true;
    if (mnBestInliers >= mRansacMinInliers) {
      nInliers = mnBestInliers;
      vbInliers = std::vector<bool>(nMatches, false);
      for (int i = 0; i < N; i++) {
        if (mvbBestInliers[i]) vbInliers[mvKeyPointIndices[i]] = true;
      }
      return best;
    }
  }

  return -1;
}
