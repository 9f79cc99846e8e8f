// TEST INFRASTRUCTURE ONLY -- a small WORKING stand-in for the part of cv::Mat that include/orbfe/MapPointRefresh.h touches
// (element access, row views, clone), so that tests/cpp/map_point_refresh_test.cpp can run on a machine without OpenCV.
// Rows are dense; a row() view shares the storage of its parent, clone() copies.  In a real build OpenCV's own header is used.
#pragma once
#include <cstddef>
#include <cstring>
#include <memory>
#include <vector>
#define CV_8U 0
#define CV_32F 5
namespace cv {
class Mat {
 public:
  Mat() : data(nullptr), rows(0), cols(0), type_(0) {}
  Mat(int r, int c, int type) : rows(r), cols(c), type_(type) {
    store_ = std::make_shared<std::vector<unsigned char> >((size_t)r * c * elem(), 0);
    data = store_->data();
  }
  unsigned char* data;
  int rows, cols;
  int type() const { return type_; }
  bool empty() const { return !data || !rows || !cols; }
  unsigned char* ptr(int r = 0) { return data + (size_t)r * cols * elem(); }
  const unsigned char* ptr(int r = 0) const { return data + (size_t)r * cols * elem(); }
  template <class T> T& at(int r) { return reinterpret_cast<T*>(data)[r]; }
  template <class T> const T& at(int r) const { return reinterpret_cast<const T*>(data)[r]; }
  template <class T> T& at(int r, int c) { return reinterpret_cast<T*>(data)[(size_t)r * cols + c]; }
  template <class T> const T& at(int r, int c) const { return reinterpret_cast<const T*>(data)[(size_t)r * cols + c]; }
  Mat row(int r) const {
    Mat m;
    m.store_ = store_; m.rows = 1; m.cols = cols; m.type_ = type_;
    m.data = data + (size_t)r * cols * elem();
    return m;
  }
  Mat clone() const {
    Mat m(rows, cols, type_);
    if (!empty()) std::memcpy(m.data, data, (size_t)rows * cols * elem());
    return m;
  }

 private:
  size_t elem() const { return type_ == CV_32F ? 4 : 1; }
  std::shared_ptr<std::vector<unsigned char> > store_;
  int type_;
};
}  // namespace cv
