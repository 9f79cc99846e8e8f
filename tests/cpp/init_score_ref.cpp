// init_score_ref.cpp -- restatement of the scoring side of the reference's monocular initialiser, for the tests of
// orbfe_score_init_hypotheses* (os1_amd/csrc/orbfe_initscore.hip).  Written from src/Initializer.cc:
//   :54-63    the compaction of vnMatches12 into mvMatches12                      -> isr_compact
//   :305-388  Initializer::CheckHomography                                        -> isr_check_homography
//   :390-468  Initializer::CheckFundamental                                       -> isr_check_fundamental
//   :124-172  the RANSAC loop of FindHomography, from the hypothesis on (:163-170) -> isr_find (H part)
//   :175-223  the RANSAC loop of FindFundamental, from the hypothesis on (:214-221) -> isr_find (F part)
// The 8-point solves in front of each hypothesis (ComputeH21 / ComputeF21, cv::SVD) are not restated: hypotheses are inputs.
// Build with -ffp-contract=off (the reference is built for x86-64 without FMA contraction); tests/test_init_score.py also
// builds it WITH contraction to show that the scenes would notice.
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

// :305-388.  pts: n x (u1 v1 u2 v2) = mvKeys1[mvMatches12[i].first].pt, mvKeys2[mvMatches12[i].second].pt
float CheckHomography(const float* H21, const float* H12, const float* pts, int N, std::vector<bool>& vbMatchesInliers, float sigma) {
  const float h11 = H21[0], h12 = H21[1], h13 = H21[2];
  const float h21 = H21[3], h22 = H21[4], h23 = H21[5];
  const float h31 = H21[6], h32 = H21[7], h33 = H21[8];

  const float h11inv = H12[0], h12inv = H12[1], h13inv = H12[2];
  const float h21inv = H12[3], h22inv = H12[4], h23inv = H12[5];
  const float h31inv = H12[6], h32inv = H12[7], h33inv = H12[8];

  vbMatchesInliers.resize(N);
  float score = 0;
  const float th = 5.991;
  const float invSigmaSquare = 1.0 / (sigma * sigma);

  for (int i = 0; i < N; i++) {
    bool bIn = true;
    const float u1 = pts[4 * i], v1 = pts[4 * i + 1], u2 = pts[4 * i + 2], v2 = pts[4 * i + 3];

    // x2in1 = H12*x2   (:352-363)
    const float w2in1inv = 1.0 / (h31inv * u2 + h32inv * v2 + h33inv);
    const float u2in1 = (h11inv * u2 + h12inv * v2 + h13inv) * w2in1inv;
    const float v2in1 = (h21inv * u2 + h22inv * v2 + h23inv) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += th - chiSquare1;

    // x1in2 = H21*x1   (:368-379)
    const float w1in2inv = 1.0 / (h31 * u1 + h32 * v1 + h33);
    const float u1in2 = (h11 * u1 + h12 * v1 + h13) * w1in2inv;
    const float v1in2 = (h21 * u1 + h22 * v1 + h23) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += th - chiSquare2;

    if (bIn) vbMatchesInliers[i] = true;
    else vbMatchesInliers[i] = false;
  }
  return score;
}

// :390-468
float CheckFundamental(const float* F21, const float* pts, int N, std::vector<bool>& vbMatchesInliers, float sigma) {
  const float f11 = F21[0], f12 = F21[1], f13 = F21[2];
  const float f21 = F21[3], f22 = F21[4], f23 = F21[5];
  const float f31 = F21[6], f32 = F21[7], f33 = F21[8];

  vbMatchesInliers.resize(N);
  float score = 0;
  const float th = 3.841;
  const float thScore = 5.991;
  const float invSigmaSquare = 1.0 / (sigma * sigma);

  for (int i = 0; i < N; i++) {
    bool bIn = true;
    const float u1 = pts[4 * i], v1 = pts[4 * i + 1], u2 = pts[4 * i + 2], v2 = pts[4 * i + 3];

    // l2 = F21 x1 = (a2, b2, c2)   (:428-441)
    const float a2 = f11 * u1 + f12 * v1 + f13;
    const float b2 = f21 * u1 + f22 * v1 + f23;
    const float c2 = f31 * u1 + f32 * v1 + f33;
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false;
    else score += thScore - chiSquare1;

    // l1 = x2t F21 = (a1, b1, c1)   (:446-459)
    const float a1 = f11 * u2 + f21 * v2 + f31;
    const float b1 = f12 * u2 + f22 * v2 + f32;
    const float c1 = f13 * u2 + f23 * v2 + f33;
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false;
    else score += thScore - chiSquare2;

    if (bIn) vbMatchesInliers[i] = true;
    else vbMatchesInliers[i] = false;
  }
  return score;
}

void put(const std::vector<bool>& v, uint8_t* out) {
  if (out) for (size_t i = 0; i < v.size(); i++) out[i] = v[i] ? 1 : 0;
}

}  // namespace

extern "C" {

float isr_check_homography(const float* pts, int n, const float* H21, const float* H12, float sigma, uint8_t* inliers) {
  std::vector<bool> in;
  const float s = CheckHomography(H21, H12, pts, n, in, sigma);
  put(in, inliers);
  return s;
}

float isr_check_fundamental(const float* pts, int n, const float* F21, float sigma, uint8_t* inliers) {
  std::vector<bool> in;
  const float s = CheckFundamental(F21, pts, n, in, sigma);
  put(in, inliers);
  return s;
}

// The loops of FindHomography (:136-171) and FindFundamental (:187-222) over K given hypotheses.  A model whose matrices are
// NULL is skipped.  scores_*: currentScore of every iteration; best_*: the iteration that set the result last, -1 = none.
void isr_find(const float* pts, int n, float sigma, int K, const float* H21, const float* H12, const float* F21, float* scores_h,
              float* scores_f, int* best_h, int* best_f, float* SH, float* SF, uint8_t* inliers_h, uint8_t* inliers_f) {
  if (H21 && H12) {
    float score = 0.0;
    std::vector<bool> vbMatchesInliers(n, false), vbCurrentInliers(n, false);
    int best = -1;
    for (int it = 0; it < K; it++) {
      const float currentScore = CheckHomography(H21 + 9 * it, H12 + 9 * it, pts, n, vbCurrentInliers, sigma);
      if (scores_h) scores_h[it] = currentScore;
      if (currentScore > score) {
        best = it;
        vbMatchesInliers = vbCurrentInliers;
        score = currentScore;
      }
    }
    if (best_h) *best_h = best;
    if (SH) *SH = score;
    put(vbMatchesInliers, inliers_h);
  }
  if (F21) {
    float score = 0.0;
    std::vector<bool> vbMatchesInliers(n, false), vbCurrentInliers(n, false);
    int best = -1;
    for (int it = 0; it < K; it++) {
      const float currentScore = CheckFundamental(F21 + 9 * it, pts, n, vbCurrentInliers, sigma);
      if (scores_f) scores_f[it] = currentScore;
      if (currentScore > score) {
        best = it;
        vbMatchesInliers = vbCurrentInliers;
        score = currentScore;
      }
    }
    if (best_f) *best_f = best;
    if (SF) *SF = score;
    put(vbMatchesInliers, inliers_f);
  }
}

// :54-63 and the gather of :341-347.  xy1 / xy2: the undistorted keypoint positions, two floats each.  Returns N.
int isr_compact(const float* xy1, int n1, const float* xy2, const int32_t* vMatches12, float* pts) {
  int N = 0;
  for (int i = 0; i < n1; i++) {
    if (vMatches12[i] >= 0) {
      const int j = vMatches12[i];
      pts[4 * N] = xy1[2 * i]; pts[4 * N + 1] = xy1[2 * i + 1]; pts[4 * N + 2] = xy2[2 * j]; pts[4 * N + 3] = xy2[2 * j + 1];
      N++;
    }
  }
  return N;
}

}  // extern "C"
