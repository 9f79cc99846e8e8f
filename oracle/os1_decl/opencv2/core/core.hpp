/* A WORKING minimal stand-in for <opencv2/core/core.hpp>, written for one purpose: to compile the reference's ORBmatcher.cc,
 * unmodified and where it lies, into oracle/_ref/libos1_matcher.so (oracle/Makefile).  Our own text; no OpenCV text in it.
 *
 * cv::Mat here is a reference-counted container of CV_32F matrices up to 4x4 and of CV_8U N x 32 descriptor rows, with the view
 * semantics the file relies on (row / col / rowRange / colRange share the storage, clone copies) and exactly the members and
 * operator forms it uses.  The arithmetic is NOT OpenCV's code: each operator form goes through the restatement the oracle uses
 * for the same form (oracle/cv_small.h):
 *     A*b + c         one cvGemm3 with the double epilogue         (-A)*b, A*b   cvGemm3 with alpha = -1 / 1, no c
 *     -A.t()*b        cvGemmT3 (double accumulation)               s*A, A/s, (1.0/s)*A.t()   a float scale
 *     cv::norm(v)     cvNorm3                                      a.dot(b)      cvDot3
 *     A - B           float subtraction
 * Small expression types keep `A*b+c` ONE gemm: a product followed by a separate add would round twice.
 * TEST INFRASTRUCTURE ONLY.  (oracle/cv_decl/ holds the declaration-only header the DBoW2 objects are built with.) */
#ifndef OS1_DECL_OPENCV2_CORE_CORE_HPP_
#define OS1_DECL_OPENCV2_CORE_CORE_HPP_
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>

#include "../../../cv_small.h"

#ifndef CV_8U
#define CV_8U 0
#define CV_32F 5
#endif

namespace cv {

struct Point2f {
  float x, y;
  Point2f() : x(0), y(0) {}
  Point2f(float x_, float y_) : x(x_), y(y_) {}
};

struct KeyPoint {   // 28 bytes, the layout of OrcKp (oracle/orb_oracle_pose.h)
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
  KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};

class Mat {
 public:
  int rows, cols;

  Mat() : rows(0), cols(0), type_(CV_32F), step_(0), data_(nullptr) {}
  Mat(int r, int c, int type) : rows(r), cols(c), type_(type) {
    step_ = (size_t)c * esz();
    buf_ = std::make_shared<std::vector<unsigned char> >((size_t)r * step_, (unsigned char)0);
    data_ = buf_->data();
  }
  // copies the rows out of foreign memory (the wrapper's way in)
  Mat(int r, int c, int type, const void* src) : Mat(r, c, type) {
    if (r * c) std::memcpy(data_, src, (size_t)r * step_);
  }

  bool empty() const { return data_ == nullptr || rows == 0 || cols == 0; }
  int type() const { return type_; }
  Mat clone() const {
    Mat m(rows, cols, type_);
    for (int r = 0; r < rows; r++) std::memcpy(m.data_ + r * m.step_, data_ + r * step_, (size_t)cols * esz());
    return m;
  }

  Mat rowRange(int a, int b) const { return view(a, b, 0, cols); }
  Mat colRange(int a, int b) const { return view(0, rows, a, b); }
  Mat row(int r) const { return view(r, r + 1, 0, cols); }
  Mat col(int c) const { return view(0, rows, c, c + 1); }

  template <typename T> T* ptr(int r = 0) { return reinterpret_cast<T*>(data_ + r * step_); }
  template <typename T> const T* ptr(int r = 0) const { return reinterpret_cast<const T*>(data_ + r * step_); }
  template <typename T> T& at(int r, int c) { return ptr<T>(r)[c]; }
  template <typename T> const T& at(int r, int c) const { return ptr<T>(r)[c]; }
  // one index: the i-th element of a vector (a column or a row), else of the row-major matrix
  template <typename T> T& at(int i) { return cols == 1 ? at<T>(i, 0) : rows == 1 ? at<T>(0, i) : at<T>(i / cols, i % cols); }
  template <typename T> const T& at(int i) const {
    return cols == 1 ? at<T>(i, 0) : rows == 1 ? at<T>(0, i) : at<T>(i / cols, i % cols);
  }

  struct Transposed;   // A.t()
  Transposed t() const;
  double dot(const Mat& m) const {   // vectors of three floats
    float a[3], b[3];
    gather3(a);
    m.gather3(b);
    return cvDot3(a, b);
  }

  // the contiguous copies the shared arithmetic takes
  void gather3(float v[3]) const {
    assert(type_ == CV_32F && rows * cols == 3);
    for (int i = 0; i < 3; i++) v[i] = at<float>(i);
  }
  void gather9(float A[9]) const {
    assert(type_ == CV_32F && rows == 3 && cols == 3);
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) A[3 * r + c] = at<float>(r, c);
  }
  static Mat vec3(const float v[3]) { return Mat(3, 1, CV_32F, v); }

 private:
  size_t esz() const { return type_ == CV_32F ? sizeof(float) : 1; }
  Mat view(int r0, int r1, int c0, int c1) const {
    assert(0 <= r0 && r0 <= r1 && r1 <= rows && 0 <= c0 && c0 <= c1 && c1 <= cols);
    Mat m;
    m.rows = r1 - r0; m.cols = c1 - c0; m.type_ = type_; m.step_ = step_; m.buf_ = buf_;
    m.data_ = data_ + r0 * step_ + (size_t)c0 * esz();
    return m;
  }
  int type_;
  size_t step_;
  std::shared_ptr<std::vector<unsigned char> > buf_;
  unsigned char* data_;
};

// ---- expression types ---------------------------------------------------------------------------------------------------------
struct Mat::Transposed {   // A.t()
  Mat a;
  operator Mat() const {
    Mat m(a.cols, a.rows, CV_32F);
    for (int r = 0; r < a.rows; r++)
      for (int c = 0; c < a.cols; c++) m.at<float>(c, r) = a.at<float>(r, c);
    return m;
  }
};
inline Mat::Transposed Mat::t() const { Transposed e; e.a = *this; return e; }

struct ScaledExpr {   // alpha * A  or  alpha * A.t()
  Mat a;
  double alpha;
  bool trans;
  operator Mat() const {   // a float scale (convertTo)
    const Mat src = trans ? (Mat)Mat::Transposed{a} : a;
    const float s = cvScaleMul(alpha);
    Mat m(src.rows, src.cols, CV_32F);
    for (int r = 0; r < src.rows; r++)
      for (int c = 0; c < src.cols; c++) m.at<float>(r, c) = src.at<float>(r, c) * s;
    return m;
  }
};

struct GemmExpr {   // alpha * op(A) * b [+ c]
  Mat a, b, c;
  double alpha;
  bool trans, has_c;
  operator Mat() const {
    float A[9], x[3], y[3], d[3];
    a.gather9(A);
    b.gather3(x);
    if (trans) {
      assert(!has_c);
      cvGemmT3(A, x, alpha, d);
    } else {
      if (has_c) c.gather3(y);
      cvGemm3(A, x, alpha, has_c ? y : nullptr, has_c ? 1.0 : 0.0, d);
    }
    return Mat::vec3(d);
  }
};

inline ScaledExpr operator-(const Mat& a) { return ScaledExpr{a, -1.0, false}; }
inline ScaledExpr operator-(const Mat::Transposed& t) { return ScaledExpr{t.a, -1.0, true}; }
inline ScaledExpr operator*(double s, const Mat::Transposed& t) { return ScaledExpr{t.a, s, true}; }
inline Mat operator*(double s, const Mat& a) { return ScaledExpr{a, s, false}; }
inline Mat operator/(const Mat& a, double s) {
  const float f = cvScaleDiv(s);
  Mat m(a.rows, a.cols, CV_32F);
  for (int r = 0; r < a.rows; r++)
    for (int c = 0; c < a.cols; c++) m.at<float>(r, c) = a.at<float>(r, c) * f;
  return m;
}
inline GemmExpr operator*(const Mat& a, const Mat& b) { return GemmExpr{a, b, Mat(), 1.0, false, false}; }
inline GemmExpr operator*(const Mat::Transposed& t, const Mat& b) { return GemmExpr{t.a, b, Mat(), 1.0, true, false}; }
inline GemmExpr operator*(const ScaledExpr& s, const Mat& b) { return GemmExpr{s.a, b, Mat(), s.alpha, s.trans, false}; }
inline GemmExpr operator+(const GemmExpr& g, const Mat& c) {
  assert(!g.has_c);
  return GemmExpr{g.a, g.b, c, g.alpha, g.trans, true};
}
inline Mat operator-(const Mat& a, const Mat& b) {
  assert(a.rows == b.rows && a.cols == b.cols);
  Mat m(a.rows, a.cols, CV_32F);
  for (int r = 0; r < a.rows; r++)
    for (int c = 0; c < a.cols; c++) m.at<float>(r, c) = a.at<float>(r, c) - b.at<float>(r, c);
  return m;
}

inline double norm(const Mat& v) {
  float x[3];
  v.gather3(x);
  return cvNorm3(x);
}

}  // namespace cv
#endif
