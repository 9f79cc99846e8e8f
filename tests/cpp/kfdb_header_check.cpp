// kfdb_header_check.cpp -- include/orbfe/KeyFrameDatabase.h compiles against the reference's names (tests/cpp/kfdb_stub) and
// has the reference's signatures (include/KeyFrameDatabase.h:48-114): every member is taken by a pointer of the reference's type.
#include "orbfe/KeyFrameDatabase.h"

using namespace ORB_SLAM2;
void (KeyFrameDatabase::*p_add)(KeyFrame*) = &KeyFrameDatabase::add;
void (KeyFrameDatabase::*p_erase)(KeyFrame*) = &KeyFrameDatabase::erase;
void (KeyFrameDatabase::*p_clear)() = &KeyFrameDatabase::clear;
void (KeyFrameDatabase::*p_resize)(size_t) = &KeyFrameDatabase::resizeInvertedFile;
std::vector<KeyFrame*> (KeyFrameDatabase::*p_loop)(KeyFrame*, float) = &KeyFrameDatabase::DetectLoopCandidates;
std::vector<KeyFrame*> (KeyFrameDatabase::*p_reloc)(Frame*) = &KeyFrameDatabase::DetectRelocalizationCandidates;
KeyFrameDatabase* make(const ORBVocabulary& voc) { return new KeyFrameDatabase(voc); }
