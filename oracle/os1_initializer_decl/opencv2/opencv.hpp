/* Stand-in for <opencv2/opencv.hpp>, written for one purpose: to compile the reference's src/Initializer.cc, unmodified and where it
 * lies, into oracle/_ref/libos1_initializer.so (oracle/Makefile).  Our own text; no OpenCV text in it.
 *
 * Only Initializer::CheckHomography and ::CheckFundamental are ever reached (oracle/os1_initializer_wrap.cpp), and of OpenCV they
 * touch nothing but cv::Mat::at<float>(r, c) on 3x3 matrices and cv::KeyPoint::pt; the constructor adds cv::Mat::clone.  Those are
 * real here: a Mat is a reference-counted row-major float buffer.  Everything else the file's unreached members name -- the matrix
 * operators, t(), inv(), the views, copyTo, dot, eye / zeros / diag, cv::SVD, cv::SVDecomp, cv::determinant, cv::norm -- is a STUB:
 * it increments the exported counter os1init_stub_calls and returns zeros.  The tests assert that the counter stays 0.
 * The matcher's stand-in (os1_decl/opencv2/core/core.hpp) is not reused: its operators are working arithmetic behind expression
 * types (A*b+c as one gemm), where this file needs every operator form of Initializer.cc to compile and none to compute.
 * TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_INITIALIZER_DECL_OPENCV2_OPENCV_HPP_
#define OS1_INITIALIZER_DECL_OPENCV2_OPENCV_HPP_
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <functional>
#include <memory>
#include <vector>

#ifndef CV_32F
#define CV_8U 0
#define CV_32F 5
#endif
#ifndef CV_PI
#define CV_PI 3.1415926535897932384626433832795
#endif

extern "C" int os1init_stub_calls;

namespace cv {

struct Point2f {
  float x, y;
  Point2f() : x(0), y(0) {}
  Point2f(float x_, float y_) : x(x_), y(y_) {}
};
struct Point3f {
  float x, y, z;
  Point3f() : x(0), y(0), z(0) {}
  Point3f(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};
struct KeyPoint {   // OpenCV's 28-byte layout
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
  KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};
struct Scalar {
  double v;
  Scalar(double v_ = 0) : v(v_) {}
};

class Mat {
 public:
  int rows, cols;

  // ---- real ----
  Mat() : rows(0), cols(0) {}
  Mat(int r, int c, int /*type*/) : rows(r), cols(c), buf_(std::make_shared<std::vector<float> >((size_t)r * c, 0.f)) {}
  Mat(int r, int c, int type, const Scalar& s) : Mat(r, c, type) { std::fill(buf_->begin(), buf_->end(), (float)s.v); }
  Mat(int r, int c, int type, const float* src) : Mat(r, c, type) { std::copy(src, src + (size_t)r * c, buf_->begin()); }
  Mat clone() const {
    Mat m;
    m.rows = rows; m.cols = cols;
    if (buf_) m.buf_ = std::make_shared<std::vector<float> >(*buf_);
    return m;
  }
  template <typename T> T& at(int r, int c) { return reinterpret_cast<T*>(buf_->data())[(size_t)r * cols + c]; }
  template <typename T> const T& at(int r, int c) const { return reinterpret_cast<const T*>(buf_->data())[(size_t)r * cols + c]; }
  template <typename T> T& at(int i) { return reinterpret_cast<T*>(buf_->data())[i]; }
  template <typename T> const T& at(int i) const { return reinterpret_cast<const T*>(buf_->data())[i]; }

  // ---- stubs: counted, never reached ----
  static Mat stub(int r = 3, int c = 3) { os1init_stub_calls++; return Mat(r, c, CV_32F); }
  Mat t() const { return stub(cols, rows); }
  Mat inv() const { return stub(rows, cols); }
  Mat row(int) const { return stub(1, cols); }
  Mat col(int) const { return stub(rows, 1); }
  Mat rowRange(int a, int b) const { return stub(b - a, cols); }
  Mat colRange(int a, int b) const { return stub(rows, b - a); }
  Mat reshape(int, int r) const { return stub(r, r ? rows * cols / r : 0); }
  void copyTo(const Mat&) const { os1init_stub_calls++; }
  double dot(const Mat&) const { os1init_stub_calls++; return 0; }
  Mat& operator*=(double) { os1init_stub_calls++; return *this; }
  static Mat eye(int r, int c, int) { return stub(r, c); }
  static Mat zeros(int r, int c, int) { return stub(r, c); }
  static Mat diag(const Mat& d) { return stub(d.rows * d.cols, d.rows * d.cols); }

 private:
  std::shared_ptr<std::vector<float> > buf_;
};

inline Mat operator*(const Mat& a, const Mat& b) { return Mat::stub(a.rows, b.cols); }
inline Mat operator*(double, const Mat& a) { return Mat::stub(a.rows, a.cols); }
inline Mat operator*(const Mat& a, double) { return Mat::stub(a.rows, a.cols); }
inline Mat operator/(const Mat& a, double) { return Mat::stub(a.rows, a.cols); }
inline Mat operator+(const Mat& a, const Mat&) { return Mat::stub(a.rows, a.cols); }
inline Mat operator-(const Mat& a, const Mat&) { return Mat::stub(a.rows, a.cols); }
inline Mat operator-(const Mat& a) { return Mat::stub(a.rows, a.cols); }

struct SVD {
  enum { MODIFY_A = 1, NO_UV = 2, FULL_UV = 4 };
  static void compute(const Mat&, Mat& w, Mat& u, Mat& vt, int = 0) {
    w = Mat::stub(3, 1);
    u = Mat::stub();
    vt = Mat::stub(9, 9);
  }
};
inline void SVDecomp(const Mat& a, Mat& w, Mat& u, Mat& vt, int flags = 0) { SVD::compute(a, w, u, vt, flags); }
inline double determinant(const Mat&) { os1init_stub_calls++; return 0; }
inline double norm(const Mat&) { os1init_stub_calls++; return 0; }

}  // namespace cv
#endif
