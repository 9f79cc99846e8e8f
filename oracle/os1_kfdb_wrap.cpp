// oracle/_ref/libos1_kfdb.so -- TEST INFRASTRUCTURE ONLY.
// C entry points over the REFERENCE'S OWN src/KeyFrameDatabase.cc, compiled unmodified and where it lies (oracle/Makefile) together
// with DBoW2's ScoringObject.cpp / BowVector.cpp / FeatureVector.cpp: add, erase, clear, DetectLoopCandidates and
// DetectRelocalizationCandidates are the reference's object code, and so are mpVoc->score and mpVoc->size (TemplatedVocabulary over
// our Row32 descriptor, os1_kfdb_decl/ORBVocabulary.h).  This file holds no reference code.  The entries have the shape of
// tests/cpp/kfdb_ref.cpp's: keyframes are named by their index of creation.
// The vocabulary of n_words words is made the way dbow2_voc_wrap.cpp gets one: the reference's loadFromBinaryFile reads an image,
// here of a root with n_words - 1 leaf records (the loader's `while(!eof)` loop appends a copy of the last record, so size() is the
// number of leaf records + 1), written to a temporary file.  Descriptors and weights are never used: the database scores BowVectors.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <iostream>
#include <vector>

#include "KeyFrameDatabase.h"
#include "Frame.h"
#include "KeyFrame.h"

using ORB_SLAM2::Frame;
using ORB_SLAM2::KeyFrame;
using ORB_SLAM2::KeyFrameDatabase;
using ORB_SLAM2::ORBVocabulary;

namespace {

struct Db {
  ORBVocabulary voc;
  KeyFrameDatabase* db = nullptr;
  std::vector<KeyFrame*> kfs;
  ~Db() {
    delete db;
    for (KeyFrame* k : kfs) delete k;
  }
};

DBoW2::BowVector bow(const unsigned* words, const double* values, int n) {
  DBoW2::BowVector v;
  for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair((DBoW2::WordId)words[i], (DBoW2::WordValue)values[i]));
  return v;
}

int put(const std::vector<KeyFrame*>& r, int* out, int cap) {
  for (size_t i = 0; i < r.size() && (int)i < cap; i++) out[i] = r[i]->index;
  return (int)r.size();
}

// k = 10, L = 5: the loader reserves (k^(L+1) - 1) / (k - 1) = 111 111 nodes, above every n_words the tests use, so the node vector
// never moves under the word pointers
bool loadVocabulary(ORBVocabulary& voc, int n_words, int scoring) {
  if (n_words < 2 || n_words > 111000 || scoring < 0 || scoring > 5) return false;
  char path[] = "/tmp/os1kfdb_voc_XXXXXX";
  const int fd = mkstemp(path);
  if (fd < 0) return false;
  FILE* f = fdopen(fd, "wb");
  const unsigned char head[4] = {10, 5, (unsigned char)scoring, 0};
  fwrite(head, 1, 4, f);
  unsigned char rec[45];
  memset(rec, 0, sizeof rec);   // parent 0 (the root), descriptor 0
  rec[4] = 1;                   // a leaf
  const double w = 1.0;
  memcpy(rec + 37, &w, 8);
  for (int i = 0; i < n_words - 1; i++) fwrite(rec, 1, 45, f);
  fclose(f);
  std::cout.setstate(std::ios_base::failbit);   // the loader prints a line per load
  const bool ok = voc.loadFromBinaryFile(path);
  std::cout.clear();
  unlink(path);
  return ok && (int)voc.size() == n_words;
}

}  // namespace

extern "C" {

int os1kfdb_is_reference_build() { return 1; }

void* os1kfdb_create(int n_words, int scoring) {
  Db* d = new Db;
  if (!loadVocabulary(d->voc, n_words, scoring)) {
    delete d;
    return 0;
  }
  d->db = new KeyFrameDatabase(d->voc);
  return d;
}
void os1kfdb_destroy(void* h) { delete (Db*)h; }
int os1kfdb_voc_size(void* h) { return (int)((Db*)h)->voc.size(); }

int os1kfdb_new_kf(void* h, uint64_t mnId, const unsigned* words, const double* values, int n) {
  Db* d = (Db*)h;
  KeyFrame* k = new KeyFrame;
  k->mnId = (long unsigned int)mnId;
  k->mBowVec = bow(words, values, n);
  k->index = (int)d->kfs.size();
  d->kfs.push_back(k);
  return k->index;
}
void os1kfdb_set_connected(void* h, int kf, const int* others, int n) {
  Db* d = (Db*)h;
  d->kfs[kf]->connected.clear();
  for (int i = 0; i < n; i++) d->kfs[kf]->connected.insert(d->kfs[others[i]]);
}
void os1kfdb_set_covisible(void* h, int kf, const int* others, int n) {
  Db* d = (Db*)h;
  d->kfs[kf]->covisible.clear();
  for (int i = 0; i < n; i++) d->kfs[kf]->covisible.push_back(d->kfs[others[i]]);
}
void os1kfdb_set_bad(void* h, int kf, int bad) { ((Db*)h)->kfs[kf]->bad = bad != 0; }
void os1kfdb_add(void* h, int kf) { Db* d = (Db*)h; d->db->add(d->kfs[kf]); }
void os1kfdb_erase(void* h, int kf) { Db* d = (Db*)h; d->db->erase(d->kfs[kf]); }
void os1kfdb_clear(void* h) { ((Db*)h)->db->clear(); }
int os1kfdb_detect_loop(void* h, int kf, float minScore, int* out, int cap) {
  Db* d = (Db*)h;
  return put(d->db->DetectLoopCandidates(d->kfs[kf], minScore), out, cap);
}
int os1kfdb_detect_reloc(void* h, uint64_t frame_id, const unsigned* words, const double* values, int n, int* out, int cap) {
  Db* d = (Db*)h;
  Frame F;
  F.mnId = (long unsigned int)frame_id;
  F.mBowVec = bow(words, values, n);
  return put(d->db->DetectRelocalizationCandidates(&F), out, cap);
}
// The minimum score the loop closer passes (LoopClosing.cc's loop over the covisible keyframes, not part of KeyFrameDatabase.cc):
// our own loop, the reference's score
float os1kfdb_min_covisible_score(void* h, int kf) {
  Db* d = (Db*)h;
  KeyFrame* cur = d->kfs[kf];
  float minScore = 1;
  for (size_t i = 0; i < cur->covisible.size(); i++) {
    KeyFrame* k = cur->covisible[i];
    if (k->bad) continue;
    float score = d->voc.score(cur->mBowVec, k->mBowVec);
    if (score < minScore) minScore = score;
  }
  return minScore;
}
// mpVoc->score(v, keyframe)
double os1kfdb_score(void* h, const unsigned* words, const double* values, int n, int kf) {
  Db* d = (Db*)h;
  return d->voc.score(bow(words, values, n), d->kfs[kf]->mBowVec);
}
// {mnLoopQuery, mnRelocQuery}, {mnLoopWords, mnRelocWords}, {mLoopScore, mRelocScore}
void os1kfdb_members(void* h, int kf, uint64_t* queries, int32_t* words, float* scores) {
  const KeyFrame* k = ((Db*)h)->kfs[kf];
  queries[0] = k->mnLoopQuery; queries[1] = k->mnRelocQuery;
  words[0] = k->mnLoopWords; words[1] = k->mnRelocWords;
  scores[0] = k->mLoopScore; scores[1] = k->mRelocScore;
}

}  // extern "C"
