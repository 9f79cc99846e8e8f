/* Stand-in for the reference's ORBVocabulary.h for oracle/_ref/libos1_kfdb.so: the reference's own TemplatedVocabulary (found on the
 * include path, compiled where it lies) over our 32-byte descriptor class in place of FORB, which needs cv::Mat.  mpVoc->score and
 * mpVoc->size, the two members src/KeyFrameDatabase.cc calls, are therefore the reference's code.  TEST INFRASTRUCTURE ONLY. */
#ifndef OS1_KFDB_DECL_ORBVOCABULARY_H_
#define OS1_KFDB_DECL_ORBVOCABULARY_H_
#include "TemplatedVocabulary.h"
#include "row32.h"

namespace ORB_SLAM2 {

typedef DBoW2::TemplatedVocabulary<Row32, Row32Ops> ORBVocabulary;

}  // namespace ORB_SLAM2
#endif
