// Our own 32-byte descriptor class in place of the reference's FORB (which needs cv::Mat), for DBoW2::TemplatedVocabulary<>: a
// descriptor is a row of 32 bytes, the distance is the Hamming distance (an exact integer, so any correct bit count gives the values
// FORB::distance gives).  Shared by dbow2_voc_wrap.cpp and os1_kfdb_decl/ORBVocabulary.h.  TEST INFRASTRUCTURE ONLY.
#ifndef ORACLE_ROW32_H_
#define ORACLE_ROW32_H_
#include <string.h>

#include <string>
#include <vector>

struct Row32 {
  unsigned char b[32];
};

struct Row32Ops {
  typedef Row32 TDescriptor;
  typedef const TDescriptor* pDescriptor;
  static const int L = 32;
  static int distance(const TDescriptor& a, const TDescriptor& b) {
    int d = 0;
    for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a.b[i] ^ b.b[i]));
    return d;
  }
  static void fromArray(TDescriptor& a, const unsigned char* p) { memcpy(a.b, p, 32); }
  // the three below are named by the template's training and text-file code only, which nothing here calls
  static void meanValue(const std::vector<pDescriptor>& rows, TDescriptor& mean) {
    memset(mean.b, 0, 32);
    if (!rows.empty()) mean = *rows[0];
  }
  static std::string toString(const TDescriptor&) { return std::string(); }
  static void fromString(TDescriptor& a, const std::string&) { memset(a.b, 0, 32); }
};

#endif
