// init_score_test.cpp -- orbfe::ScoreInitializerHypotheses (include/orbfe/orb_shim.hpp) against the restatement
// tests/cpp/init_score_ref.cpp on the scene files tests/init_score_util.py writes.  For every scene it prints one line and
// compares SH, SF, the winning iterations, every iteration's score (NaN by class) and the vector<bool> masks.
// -DINIT_SCORE_CV_TYPES: only the instantiation with the reference's own types (cv::KeyPoint, cv::Mat), for a syntax check
// against tests/cpp/opencv_stub.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "orbfe/orb_shim.hpp"

#ifdef INIT_SCORE_CV_TYPES
#include <opencv2/core/core.hpp>
// the shape of the replacement inside Initializer::Initialize
void initialize_body(orbfe::MatcherContext& ctx, const std::vector<cv::KeyPoint>& mvKeys1, const std::vector<cv::KeyPoint>& mvKeys2,
                     const std::vector<std::pair<int, int>>& mvMatches12, float mSigma, const std::vector<cv::Mat>& vH21,
                     const std::vector<cv::Mat>& vH12, const std::vector<cv::Mat>& vF21, orbfe::InitializerScores& S) {
  orbfe::ScoreInitializerHypotheses(ctx, mvKeys1, mvKeys2, mvMatches12, mSigma, vH21, vH12, vF21, S);
}
#else

extern "C" void isr_find(const float* pts, int n, float sigma, int K, const float* H21, const float* H12, const float* F21, float* scores_h,
                         float* scores_f, int* best_h, int* best_f, float* SH, float* SF, uint8_t* inliers_h, uint8_t* inliers_f);

namespace {

struct Point2f { float x, y; };
struct KeyPoint { Point2f pt; float size, angle, response; int octave, class_id; };
struct Mat33 {
  float v[9];
  template <class T> const T& at(int r, int c) const { return v[3 * r + c]; }
};

template <class T>
bool readv(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool same(float a, float b) {
  if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
  return memcmp(&a, &b, 4) == 0;
}

int run(orbfe::MatcherContext& ctx, const char* path) {
  FILE* f = fopen(path, "rb");
  if (!f) { printf("cannot open %s\n", path); return 1; }
  int hdr[6];
  float sigma;
  std::vector<float> xy1, xy2, h21, h12, f21;
  std::vector<int> pr;
  bool ok = fread(hdr, 4, 6, f) == 6 && fread(&sigma, 4, 1, f) == 1;
  const int n1 = hdr[0], n2 = hdr[1], N = hdr[2], K = hdr[3], hasH = hdr[4], hasF = hdr[5];
  ok = ok && readv(f, xy1, 2 * (size_t)n1) && readv(f, xy2, 2 * (size_t)n2) && readv(f, pr, 2 * (size_t)N) &&
       readv(f, h21, hasH ? 9 * (size_t)K : 0) && readv(f, h12, hasH ? 9 * (size_t)K : 0) && readv(f, f21, hasF ? 9 * (size_t)K : 0);
  fclose(f);
  if (!ok) { printf("short scene file %s\n", path); return 1; }

  std::vector<KeyPoint> keys1(n1), keys2(n2);
  for (int i = 0; i < n1; i++) keys1[i] = KeyPoint{{xy1[2 * i], xy1[2 * i + 1]}, 31.f, 0.f, 0.f, 0, -1};
  for (int i = 0; i < n2; i++) keys2[i] = KeyPoint{{xy2[2 * i], xy2[2 * i + 1]}, 31.f, 0.f, 0.f, 0, -1};
  std::vector<std::pair<int, int>> matches12(N);
  std::vector<float> pts(4 * (size_t)N + 4);
  for (int i = 0; i < N; i++) {
    matches12[i] = std::make_pair(pr[2 * i], pr[2 * i + 1]);
    pts[4 * i] = keys1[pr[2 * i]].pt.x; pts[4 * i + 1] = keys1[pr[2 * i]].pt.y;
    pts[4 * i + 2] = keys2[pr[2 * i + 1]].pt.x; pts[4 * i + 3] = keys2[pr[2 * i + 1]].pt.y;
  }
  std::vector<Mat33> H21s(hasH ? K : 0), H12s(hasH ? K : 0), F21s(hasF ? K : 0);
  for (int k = 0; k < K; k++) {
    if (hasH) { memcpy(H21s[k].v, &h21[9 * (size_t)k], 36); memcpy(H12s[k].v, &h12[9 * (size_t)k], 36); }
    if (hasF) memcpy(F21s[k].v, &f21[9 * (size_t)k], 36);
  }

  orbfe::InitializerScores S;
  orbfe::ScoreInitializerHypotheses(ctx, keys1, keys2, matches12, sigma, H21s, H12s, F21s, S);

  std::vector<float> sh(K), sf(K);
  std::vector<uint8_t> ih(N + 1), iF(N + 1);
  int bh = -1, bf = -1;
  float SH = 0.f, SF = 0.f;
  isr_find(pts.data(), N, sigma, K, hasH ? h21.data() : nullptr, hasH ? h12.data() : nullptr, hasF ? f21.data() : nullptr, sh.data(),
           sf.data(), &bh, &bf, &SH, &SF, ih.data(), iF.data());
  int bad = 0;
  if (hasH) {
    bad += S.bestH != bh || !same(S.SH, SH) || (int)S.scoresH.size() != K || (int)S.vbMatchesInliersH.size() != N;
    for (int k = 0; k < K && !bad; k++) bad += !same(S.scoresH[k], sh[k]);
    for (int i = 0; i < N && !bad; i++) bad += S.vbMatchesInliersH[i] != (ih[i] != 0);
  }
  if (hasF) {
    bad += S.bestF != bf || !same(S.SF, SF) || (int)S.scoresF.size() != K || (int)S.vbMatchesInliersF.size() != N;
    for (int k = 0; k < K && !bad; k++) bad += !same(S.scoresF[k], sf[k]);
    for (int i = 0; i < N && !bad; i++) bad += S.vbMatchesInliersF[i] != (iF[i] != 0);
  }
  printf("%s: N %d K %d bestH %d (ref %d) SH %.9g bestF %d (ref %d) SF %.9g %s\n", path, N, K, S.bestH, bh, (double)S.SH, S.bestF, bf,
         (double)S.SF, bad ? "MISMATCH" : "ok");
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  orbfe::MatcherContext ctx(0);
  int bad = 0;
  for (int i = 1; i < argc; i++) bad += run(ctx, argv[i]);
  printf("scenes %d mismatches %d\n", argc - 1, bad);
  printf(bad ? "FAIL\n" : "PASS\n");
  return bad ? 1 : 0;
}
#endif
