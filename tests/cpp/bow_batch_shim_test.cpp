// bow_batch_shim_test.cpp -- the two map-load overloads of include/orbfe/orb_shim.hpp on a stub KeyFrame type:
//   orbfe::ComputeBoW(voc, std::vector<KeyFrame*>&)        against the one-keyframe overload, keyframe by keyframe; the
//                                                          `if(mBowVec.empty())` guard per keyframe (a computed keyframe keeps
//                                                          its vectors and is not sent); one keyframe's rows from its resident copy
//   orbfe::KeyFrameDatabaseT<KeyFrame>::add(vector)        against single adds: DetectRelocalizationCandidates returns the same list
//   default               links liborbfe.so, argv[1] = a binary vocabulary file (tests/test_gpu_bow_batch.py)
//   -DBOWB_HOST_BACKEND   the C calls the two overloads make are defined HERE on the host (a toy vocabulary: word = first byte
//                         modulo 32, node = word / 4; the database as a plain list), so that the shim's marshalling runs on a
//                         machine without a GPU (tests/test_bow_batch.py); it also counts the calls
// Prints PASS; exit code 0 iff every comparison is exact.
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <vector>

#include "orbfe/orb_shim.hpp"

typedef std::map<unsigned int, double> BowVector;
typedef std::map<unsigned int, std::vector<unsigned int> > FeatureVector;
struct Mat {   // the members of cv::Mat the shim reads
  unsigned char* data = nullptr;
  size_t step = 32;
  int rows = 0;
  std::vector<unsigned char> store;
};
struct KeyFrame {
  long unsigned int mnId = 0;
  Mat mDescriptors;
  std::vector<OrbfeKeyPoint> mvKeys, mvKeysUn;   // (mvKeys stays empty: no extractor produced these keyframes)
  int mnMinX = 0, mnMaxX = 640, mnMinY = 0, mnMaxY = 480;
  BowVector mBowVec;
  FeatureVector mFeatVec;
  long unsigned int mnLoopQuery = 0, mnRelocQuery = 0;
  int mnLoopWords = 0, mnRelocWords = 0;
  float mLoopScore = 0, mRelocScore = 0;
  int index = 0;
  std::set<KeyFrame*> GetConnectedKeyFrames() { return std::set<KeyFrame*>(); }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return std::vector<KeyFrame*>(); }
  std::vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int&) { return std::vector<KeyFrame*>(); }
  bool isBad() { return false; }
};
struct Frame {
  long unsigned int mnId = 0;
  BowVector mBowVec;
};

#ifdef BOWB_HOST_BACKEND
static int g_singles = 0, g_batches = 0, g_batchSets = 0, g_addSingles = 0, g_addBatches = 0;
struct orbfe_vocabulary { int unused; };
struct HostKf { uint64_t key; std::vector<uint32_t> w; std::vector<double> v; };
struct orbfe_kfdb { std::vector<HostKf> kfs; };
struct orbfe_frame { int unused; };
extern "C" {
const char* orbfe_last_error(void) { return "host back end"; }
unsigned long long orbfe_resident_epoch(void) { return 0; }
const uint8_t* orbfe_frame_descriptors_device(orbfe_frame*) { return nullptr; }
int orbfe_vocabulary_create_from_image(int, const void*, size_t, orbfe_vocabulary** out) { *out = new orbfe_vocabulary; return ORBFE_OK; }
void orbfe_vocabulary_destroy(orbfe_vocabulary* v) { delete v; }
int orbfe_bow_transform(orbfe_vocabulary*, const uint8_t* desc, int n, int, int, uint32_t* bow_ids, double* bow_values, int* n_words,
                        uint32_t* fv_nodes, uint32_t* fv_offsets, uint32_t* fv_features, int* n_fv_nodes, uint32_t*, uint32_t*) {
  g_singles++;
  std::map<uint32_t, double> bow;
  std::map<uint32_t, std::vector<uint32_t> > fv;
  for (int i = 0; i < n; i++) { const uint32_t w = desc[32 * (size_t)i] % 32u; bow[w] += 1.0 / n; fv[w / 4].push_back((uint32_t)i); }
  *n_words = 0;
  for (auto& e : bow) { bow_ids[*n_words] = e.first; bow_values[*n_words] = e.second; ++*n_words; }
  *n_fv_nodes = 0;
  uint32_t at = 0;
  fv_offsets[0] = 0;
  for (auto& e : fv) {
    fv_nodes[*n_fv_nodes] = e.first;
    for (uint32_t f : e.second) fv_features[at++] = f;
    fv_offsets[++*n_fv_nodes] = at;
  }
  return ORBFE_OK;
}
int orbfe_bow_transform_batch(orbfe_vocabulary* v, int levelsup, int n_sets, const uint8_t* const* desc, const int* n, const int* capacity,
                              uint32_t* const* bow_ids, double* const* bow_values, int* n_words, uint32_t* const* fv_nodes,
                              uint32_t* const* fv_offsets, uint32_t* const* fv_features, int* n_fv_nodes, uint32_t* const*, uint32_t* const*) {
  g_batches++;
  g_batchSets += n_sets;
  for (int s = 0; s < n_sets; s++) if (capacity[s] < n[s]) return ORBFE_ERR_OVERFLOW;
  for (int s = 0; s < n_sets; s++) {
    orbfe_bow_transform(v, desc[s], n[s], 0, levelsup, bow_ids[s], bow_values[s], &n_words[s], fv_nodes[s], fv_offsets[s], fv_features[s],
                        &n_fv_nodes[s], nullptr, nullptr);
    g_singles--;
  }
  return ORBFE_OK;
}
int orbfe_kfdb_create(int, int, int, int, int, orbfe_kfdb** out) { *out = new orbfe_kfdb; return ORBFE_OK; }
void orbfe_kfdb_destroy(orbfe_kfdb* db) { delete db; }
int orbfe_kfdb_add(orbfe_kfdb* db, uint64_t key, const uint32_t* words, const double* values, int n) {
  g_addSingles++;
  for (auto& k : db->kfs) if (k.key == key) return ORBFE_ERR_INVALID;
  db->kfs.push_back(HostKf{key, std::vector<uint32_t>(words, words + n), std::vector<double>(values, values + n)});
  return ORBFE_OK;
}
int orbfe_kfdb_add_batch(orbfe_kfdb* db, int n, const uint64_t* keys, const uint32_t* const* words, const double* const* values,
                         const int* n_words) {
  g_addBatches++;
  for (int j = 0; j < n; j++) {
    for (auto& k : db->kfs) if (k.key == keys[j]) return ORBFE_ERR_INVALID;
    for (int i = 0; i < j; i++) if (keys[i] == keys[j]) return ORBFE_ERR_INVALID;
  }
  for (int j = 0; j < n; j++) { orbfe_kfdb_add(db, keys[j], words[j], values[j], n_words[j]); g_addSingles--; }
  return ORBFE_OK;
}
int orbfe_kfdb_erase(orbfe_kfdb*, uint64_t) { return ORBFE_OK; }
int orbfe_kfdb_clear(orbfe_kfdb* db) { db->kfs.clear(); return ORBFE_OK; }
int orbfe_kfdb_size(orbfe_kfdb* db, int* nk, int* ne) {
  if (nk) *nk = (int)db->kfs.size();
  if (ne) { *ne = 0; for (auto& k : db->kfs) *ne += (int)k.w.size(); }
  return ORBFE_OK;
}
int orbfe_kfdb_score(orbfe_kfdb*, const uint32_t*, const double*, int, const uint64_t*, int, double*) { return ORBFE_ERR_INVALID; }
// every keyframe with a common word, by (first common word, add order); L1 score (ScoringObject.cpp:34-65)
int orbfe_kfdb_query(orbfe_kfdb* db, const uint32_t* qw, const double* qv, int nq, uint64_t* keys, int32_t* common, double* scores, int cap,
                     int* n_out) {
  struct Rec { uint32_t first; size_t seq; int common; double score; };
  std::vector<Rec> recs;
  for (size_t k = 0; k < db->kfs.size(); k++) {
    Rec r = {0, k, 0, 0.0};
    for (int i = 0; i < nq; i++)
      for (size_t j = 0; j < db->kfs[k].w.size(); j++)
        if (db->kfs[k].w[j] == qw[i]) {
          if (!r.common) r.first = qw[i];
          r.common++;
          const double vi = qv[i], wi = db->kfs[k].v[j];
          r.score += std::fabs(vi - wi) - std::fabs(vi) - std::fabs(wi);
        }
    r.score = -r.score / 2.0;
    if (r.common) recs.push_back(r);
  }
  std::sort(recs.begin(), recs.end(), [](const Rec& a, const Rec& b) { return a.first != b.first ? a.first < b.first : a.seq < b.seq; });
  *n_out = (int)recs.size();
  for (int i = 0; i < (int)recs.size() && i < cap; i++) { keys[i] = db->kfs[recs[i].seq].key; common[i] = recs[i].common; scores[i] = recs[i].score; }
  return (int)recs.size() > cap ? ORBFE_ERR_OVERFLOW : ORBFE_OK;
}
}
#endif

#define CHECK(cond)                                                                       \
  do {                                                                                    \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static uint32_t g_state = 777u;
static uint32_t rnd() { g_state = g_state * 1664525u + 1013904223u; return g_state >> 8; }

static void fill(KeyFrame& k, int index, int n) {
  k.index = index;
  k.mnId = 10 + (unsigned long)index;
  k.mDescriptors.store.assign((size_t)n * 32 + 1, 0);
  for (auto& b : k.mDescriptors.store) b = (unsigned char)rnd();
  k.mDescriptors.data = k.mDescriptors.store.data();
  k.mDescriptors.rows = n;
  k.mvKeysUn.assign(n, OrbfeKeyPoint());
  for (int i = 0; i < n; i++) { k.mvKeysUn[i].x = (float)(rnd() % 640); k.mvKeysUn[i].y = (float)(rnd() % 480); k.mvKeysUn[i].octave = (int)(rnd() % 8); }
}

int main(int argc, char** argv) {
  try {
    orbfe::Vocabulary voc(0);
#ifdef BOWB_HOST_BACKEND
    CHECK(voc.loadFromBinaryFile(argv[0]));   // (any readable file: the host back end ignores the image)
#else
    CHECK(argc > 1 && voc.loadFromBinaryFile(argv[1]));
#endif
    (void)argc;
    const int sizes[4] = {65, 200, 1, 63};
    KeyFrame a[4], b[4];   // a: one call for all; b: the one-keyframe overload
    for (int i = 0; i < 4; i++) {
      fill(a[i], i, sizes[i]);
      b[i] = a[i];
      b[i].mDescriptors.data = b[i].mDescriptors.store.data();
    }
    // keyframe 2 has its vectors already: a sentinel no transform produces, which must survive
    a[2].mBowVec[7] = 0.5; a[2].mFeatVec[3].push_back(0);
    b[2].mBowVec = a[2].mBowVec; b[2].mFeatVec = a[2].mFeatVec;
    std::vector<KeyFrame*> va, vb;
    for (int i = 0; i < 4; i++) { va.push_back(&a[i]); vb.push_back(&b[i]); }
#ifndef BOWB_HOST_BACKEND
    orbfe::MatcherContext ctx(0);
    CHECK(ctx.resident(a[1], 1) != nullptr);            // keyframe 1's rows are on the device: the batch reads them there
    CHECK(ctx.residentIfHeld(a[1]) != nullptr && ctx.residentIfHeld(a[0]) == nullptr);
    orbfe::ComputeBoW(voc, va, &ctx);
    CHECK(ctx.residentFrames() == 1);                   // the batch call created no resident copy of its own
#else
    orbfe::ComputeBoW(voc, va);
    CHECK(g_batches == 1 && g_batchSets == 3 && g_singles == 0);   // the computed keyframe was not sent
#endif
    for (int i = 0; i < 4; i++) orbfe::ComputeBoW(voc, b[i]);
    for (int i = 0; i < 4; i++) {
      CHECK(a[i].mBowVec == b[i].mBowVec && a[i].mFeatVec == b[i].mFeatVec);
      if (i != 2) CHECK(!a[i].mBowVec.empty() && !a[i].mFeatVec.empty());
      for (auto& e : a[i].mBowVec) CHECK(std::memcmp(&e.second, &b[i].mBowVec[e.first], 8) == 0);
    }
    CHECK(a[2].mBowVec.size() == 1 && a[2].mBowVec[7] == 0.5 && a[2].mFeatVec.size() == 1);
    // a second call finds every keyframe computed and sends nothing; an empty vector is fine
    const std::vector<KeyFrame*> none;
    orbfe::ComputeBoW(voc, none);
    orbfe::ComputeBoW(voc, va);
#ifdef BOWB_HOST_BACKEND
    CHECK(g_batches == 1 && g_batchSets == 3);
#endif

    // ---- KeyFrameDatabaseT::add(vector) ----
    orbfe::KeyFrameDatabaseT<KeyFrame> dbA(0, 1u << 20, 0, 2, 64), dbB(0, 1u << 20, 0, 2, 64);   // tight: the pool has to grow
    dbA.add(va);
    for (int i = 0; i < 4; i++) dbB.add(vb[i]);
    CHECK(dbA.size() == 4 && dbB.size() == 4);
#ifdef BOWB_HOST_BACKEND
    CHECK(g_addBatches >= 1);
#endif
    bool thrown = false;
    try { dbA.add(va); } catch (const std::runtime_error&) { thrown = true; }
    CHECK(thrown && dbA.size() == 4);
    int listed = 0;
    for (int q = 0; q < 4; q++) {
      Frame FA, FB;
      FA.mnId = FB.mnId = 100 + (unsigned long)q;
      FA.mBowVec = FB.mBowVec = a[q].mBowVec;
      const std::vector<KeyFrame*> ca = dbA.DetectRelocalizationCandidates(&FA), cb = dbB.DetectRelocalizationCandidates(&FB);
      CHECK(ca.size() == cb.size());
      for (size_t i = 0; i < ca.size(); i++) CHECK(ca[i]->index == cb[i]->index);
      for (int i = 0; i < 4; i++)
        CHECK(a[i].mnRelocWords == b[i].mnRelocWords && std::memcmp(&a[i].mRelocScore, &b[i].mRelocScore, 4) == 0);
      listed += (int)ca.size();
    }
    CHECK(listed >= 4);
  } catch (const std::exception& e) {
    std::printf("FAIL: %s\n", e.what());
    return 1;
  }
  std::printf("PASS\n");
  return 0;
}
