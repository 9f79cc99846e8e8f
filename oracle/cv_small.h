/* cv_small.h -- the small-matrix OpenCV arithmetic the pose-driven searches go through, restated once (RECALLED from OpenCV 4.x
 * core/src/matmul.simd.hpp, matrix_expressions.cpp, norm.cpp; cross-checked against a live OpenCV by tests/test_opencv_live.py):
 *   A*b + c, A 3x3, b 3x1 (gemm, flags 0, len 3: small-matrix path): t = a0*b0 + a1*b1 + a2*b2 in FLOAT, left to right;
 *                          d = (float)((double)t*alpha + (double)c*beta)
 *   -A.t()*b              (gemm with GEMM_1_T: generic GEMMSingleMul<float,double>): double products and sums, d = (float)(s*alpha)
 *   cv::norm(v)           sqrt of a double sum of double squares (returned as double)
 *   a.dot(b)              double sum of double products
 *   M / s, s * M          convertTo with a float scale: m * (float)(1.0/s) resp. m * (float)s
 * Included by oracle/orb_oracle.cpp (the restated searches) and by oracle/os1_decl/opencv2/core/core.hpp (the cv::Mat stand-in the
 * reference's own ORBmatcher.cc is compiled against), so the two sides share one copy.  TEST INFRASTRUCTURE ONLY.  Plain C++11. */
#ifndef ORB_ORACLE_CV_SMALL_H_
#define ORB_ORACLE_CV_SMALL_H_
#include <cmath>

static inline void cvGemm3(const float A[9], const float b[3], double alpha, const float* c, double beta, float d[3]) {
  for (int i = 0; i < 3; i++) {
    const float t = A[3 * i] * b[0] + A[3 * i + 1] * b[1] + A[3 * i + 2] * b[2];
    d[i] = (float)((double)t * alpha + (double)(c ? c[i] : 0.f) * beta);
  }
}
static inline void cvGemmT3(const float A[9], const float b[3], double alpha, float d[3]) {   // alpha * A^T * b
  for (int i = 0; i < 3; i++) {
    double s = 0;
    for (int k = 0; k < 3; k++) s += (double)A[3 * k + i] * (double)b[k];
    d[i] = (float)(s * alpha);
  }
}
static inline double cvNorm3(const float v[3]) {
  double s = 0;
  for (int k = 0; k < 3; k++) s += (double)v[k] * (double)v[k];
  return std::sqrt(s);
}
static inline double cvDot3(const float a[3], const float b[3]) {
  double r = 0;
  for (int k = 0; k < 3; k++) r += (double)a[k] * (double)b[k];
  return r;
}
static inline float cvScaleMul(double s) { return (float)s; }          // s * M:  m * (float)s
static inline float cvScaleDiv(double s) { return (float)(1.0 / s); }   // M / s:  m * (float)(1.0/s)

#endif
