// oracle/_ref/libos1_initializer.so -- TEST INFRASTRUCTURE ONLY.
// C entry points over the REFERENCE'S OWN src/Initializer.cc, compiled unmodified and where it lies (oracle/Makefile): one entry per
// member, Initializer::CheckHomography and Initializer::CheckFundamental, and nothing else of the file is ever reached.  This file
// holds no reference code.
// Both members and the three vectors they read (mvKeys1, mvKeys2, mvMatches12) are private.  They are reached without touching the
// source text or its compile line: an explicit template instantiation may name a private member (access checking does not apply
// to its arguments), and the instantiation defines a friend that hands the member pointer out.
// Everything the unreached members need of OpenCV is a counted stub (os1_initializer_decl/opencv2/opencv.hpp); the counter is
// exported here and read after every call.
#include <stdint.h>

#include <utility>
#include <vector>

#include "Initializer.h"

extern "C" {
int os1init_stub_calls = 0;
}

using ORB_SLAM2::Frame;
using ORB_SLAM2::Initializer;

namespace {

template <class Tag, typename Tag::type M>
struct Rob {
  friend typename Tag::type get(Tag) { return M; }
};
struct CheckH {
  typedef float (Initializer::*type)(const cv::Mat&, const cv::Mat&, std::vector<bool>&, float);
  friend type get(CheckH);
};
struct CheckF {
  typedef float (Initializer::*type)(const cv::Mat&, std::vector<bool>&, float);
  friend type get(CheckF);
};
struct Keys1 {
  typedef std::vector<cv::KeyPoint> Initializer::*type;
  friend type get(Keys1);
};
struct Keys2 {
  typedef std::vector<cv::KeyPoint> Initializer::*type;
  friend type get(Keys2);
};
struct Matches12 {
  typedef std::vector<std::pair<int, int> > Initializer::*type;
  friend type get(Matches12);
};
template struct Rob<CheckH, &Initializer::CheckHomography>;
template struct Rob<CheckF, &Initializer::CheckFundamental>;
template struct Rob<Keys1, &Initializer::mvKeys1>;
template struct Rob<Keys2, &Initializer::mvKeys2>;
template struct Rob<Matches12, &Initializer::mvMatches12>;

// An Initializer whose mvKeys1 / mvKeys2 hold match i's two points at index i, and mvMatches12[i] = (i, i)
struct Loaded {
  Frame ref;
  Initializer* ini;
  Loaded(const float* pts, int n, float sigma) {
    ref.mK = cv::Mat(3, 3, CV_32F);
    ini = new Initializer(ref, sigma, 1);
    std::vector<cv::KeyPoint>& k1 = ini->*get(Keys1());
    std::vector<cv::KeyPoint>& k2 = ini->*get(Keys2());
    std::vector<std::pair<int, int> >& m = ini->*get(Matches12());
    k1.resize(n);
    k2.resize(n);
    m.resize(n);
    for (int i = 0; i < n; i++) {
      k1[i].pt = cv::Point2f(pts[4 * i], pts[4 * i + 1]);
      k2[i].pt = cv::Point2f(pts[4 * i + 2], pts[4 * i + 3]);
      m[i] = std::make_pair(i, i);
    }
  }
  ~Loaded() { delete ini; }
};

void put(const std::vector<bool>& v, int n, uint8_t* inliers) {
  for (int i = 0; i < n; i++) inliers[i] = v[i] ? 1 : 0;
}

}  // namespace

extern "C" {

int os1init_is_reference_build() { return 1; }
int os1init_stub_counter() { return os1init_stub_calls; }

// pts[n][4] = (u1, v1, u2, v2); H21, H12 row-major 3x3
float os1init_check_homography(const float* pts, int n, const float* H21, const float* H12, float sigma, uint8_t* inliers) {
  Loaded L(pts, n, sigma);
  const cv::Mat h21(3, 3, CV_32F, H21), h12(3, 3, CV_32F, H12);
  std::vector<bool> in;
  const float s = (L.ini->*get(CheckH()))(h21, h12, in, sigma);
  put(in, n, inliers);
  return s;
}

float os1init_check_fundamental(const float* pts, int n, const float* F21, float sigma, uint8_t* inliers) {
  Loaded L(pts, n, sigma);
  const cv::Mat f21(3, 3, CV_32F, F21);
  std::vector<bool> in;
  const float s = (L.ini->*get(CheckF()))(f21, in, sigma);
  put(in, n, inliers);
  return s;
}

// K hypotheses over one set of matches: scores[K], and the inlier flags of hypothesis `keep` (-1: none)
void os1init_check_many(const float* pts, int n, float sigma, int K, const float* H21, const float* H12, const float* F21, float* scores_h,
                        float* scores_f, int keep_h, int keep_f, uint8_t* inliers_h, uint8_t* inliers_f) {
  Loaded L(pts, n, sigma);
  std::vector<bool> in;
  for (int k = 0; k < K; k++) {
    if (H21) {
      const cv::Mat h21(3, 3, CV_32F, H21 + 9 * k), h12(3, 3, CV_32F, H12 + 9 * k);
      scores_h[k] = (L.ini->*get(CheckH()))(h21, h12, in, sigma);
      if (k == keep_h) put(in, n, inliers_h);
    }
    if (F21) {
      const cv::Mat f21(3, 3, CV_32F, F21 + 9 * k);
      scores_f[k] = (L.ini->*get(CheckF()))(f21, in, sigma);
      if (k == keep_f) put(in, n, inliers_f);
    }
  }
}

}  // extern "C"
