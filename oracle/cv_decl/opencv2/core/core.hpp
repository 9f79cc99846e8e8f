// oracle/cv_decl/opencv2/core/core.hpp -- TEST INFRASTRUCTURE ONLY.
// A declaration-only stand-in for the one OpenCV header DBoW2's TemplatedVocabulary.h includes, so that oracle/Makefile can
// compile the reference's vocabulary template with plain g++ into oracle/_ref/libdbow2_voc.so.  The template only NAMES
// cv::FileStorage / cv::FileNode, in its YAML save / load, which nothing in this project calls.  Everything here is this project's
// own text: the two class names with the members that template spells, every body an abort().  The bodies are inline so
// that no undefined cv:: symbol remains in the shared object (ctypes opens it with RTLD_NOW).
// The real header also brings in <cmath> and <sstream>, which the template relies on without including them.
#ifndef ORACLE_CV_DECL_CORE_HPP
#define ORACLE_CV_DECL_CORE_HPP

#include <cmath>
#include <cstdlib>
#include <sstream>
#include <string>

namespace cv {

class FileNode {
 public:
  FileNode() {}
  FileNode operator[](const std::string&) const { std::abort(); }
  FileNode operator[](const char*) const { std::abort(); }
  FileNode operator[](int) const { std::abort(); }
  size_t size() const { std::abort(); }
  operator int() const { std::abort(); }
  operator double() const { std::abort(); }
  operator std::string() const { std::abort(); }
};

class FileStorage {
 public:
  enum Mode { READ = 0, WRITE = 1 };
  FileStorage(const std::string&, int) { std::abort(); }
  bool isOpened() const { std::abort(); }
  FileNode operator[](const std::string&) const { std::abort(); }
  FileNode operator[](const char*) const { std::abort(); }
};

template <class T>
inline FileStorage& operator<<(FileStorage&, const T&) { std::abort(); }

}  // namespace cv

#endif
