// oracle/_ref/libdbow2_voc.so -- TEST INFRASTRUCTURE ONLY.
// A C entry point over the REFERENCE'S OWN DBoW2 vocabulary: TemplatedVocabulary<>::loadFromBinaryFile, transform(features, v, fv,
// levelsup), the single-feature transform(feature, id, weight, &nid, levelsup) and score(v1, v2) through the scoring object the
// loader created.  This file holds no reference code: oracle/Makefile compiles it together with the reference's
// TemplatedVocabulary.h, ScoringObject.cpp, BowVector.cpp, FeatureVector.cpp and DUtils/Random.cpp / Timestamp.cpp where they lie,
// with oracle/cv_decl/ standing in for the OpenCV header the template includes (declarations only), output into oracle/_ref/
// (git-ignored).
// The template's F parameter is Row32Ops below, in place of the reference's FORB (which needs cv::Mat): a descriptor is a row of
// 32 bytes, the distance is the Hamming distance.  That distance is an exact integer, so any correct bit count gives the values
// FORB::distance gives; what is pinned is everything the template does with them: the loader, the strict `<` over the children in
// stored order, the levelsup cut, the weighting and normalisation set-up, the accumulation and the scores.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "TemplatedVocabulary.h"
#include "row32.h"   // Row32 / Row32Ops

namespace {

// the single-feature transform with the node id is a protected member
struct Voc : public DBoW2::TemplatedVocabulary<Row32, Row32Ops> {
  typedef DBoW2::TemplatedVocabulary<Row32, Row32Ops> Base;
  void one(const Row32& f, DBoW2::WordId& id, DBoW2::WordValue& w, DBoW2::NodeId* nid, int levelsup) const {
    Base::transform(f, id, w, nid, levelsup);
  }
  unsigned nodes() const { return (unsigned)m_nodes.size(); }
};

DBoW2::BowVector bow(const uint32_t* ids, const double* vals, int n) {
  DBoW2::BowVector v;
  for (int i = 0; i < n; i++) v.insert(v.end(), std::make_pair((DBoW2::WordId)ids[i], (DBoW2::WordValue)vals[i]));
  return v;
}

}  // namespace

extern "C" {

// NULL where the reference's loader refuses the file
void* dbow2voc_open(const char* path) {
  Voc* v = new Voc;
  if (!v->loadFromBinaryFile(path)) {
    delete v;
    return 0;
  }
  return v;
}

void dbow2voc_close(void* h) { delete (Voc*)h; }

// size(), k, L, scoring type, weighting type as the object holds them, and the number of tree nodes (root included)
void dbow2voc_info(void* h, int* out) {
  const Voc& v = *(Voc*)h;
  out[0] = (int)v.size();
  out[1] = v.getBranchingFactor();
  out[2] = v.getDepthLevels();
  out[3] = (int)v.getScoringType();
  out[4] = (int)v.getWeightingType();
  out[5] = (int)v.nodes();
}

// transform(features, v, fv, levelsup); per feature the single-feature transform's word and node.  Same output layout as the
// oracle's orc_bow_transform: bow_ids / bow_vals / fv_nodes / fv_feat / word_of / node_of hold n entries, fv_off n + 1.
// The single-feature transform writes *nid only if the descent passes level L - levelsup (or that level is <= 0): a feature whose
// word lies above that level leaves it untouched, and node_of then holds the value it is preset to here, 0xffffffff.  (The batch
// transform reads an uninitialised variable for such a feature, so its FeatureVector entry for it is indeterminate.)
int dbow2voc_transform(void* h, const uint8_t* desc, int n, int levelsup, uint32_t* bow_ids, double* bow_vals, int* n_words,
                       uint32_t* fv_nodes, uint32_t* fv_off, uint32_t* fv_feat, int* n_fv, uint32_t* word_of, uint32_t* node_of) {
  const Voc& V = *(Voc*)h;
  std::vector<Row32> features(n);
  for (int i = 0; i < n; i++) memcpy(features[i].b, desc + 32 * (size_t)i, 32);
  DBoW2::BowVector v;
  DBoW2::FeatureVector fv;
  V.transform(features, v, fv, levelsup);
  for (int i = 0; i < n; i++) {
    DBoW2::WordId id = 0;
    DBoW2::WordValue w = 0;
    DBoW2::NodeId nid = 0xffffffffu;
    V.one(features[i], id, w, &nid, levelsup);
    word_of[i] = id;
    node_of[i] = nid;
  }
  int nw = 0;
  for (DBoW2::BowVector::const_iterator it = v.begin(); it != v.end(); ++it) {
    bow_ids[nw] = it->first;
    bow_vals[nw] = it->second;
    nw++;
  }
  *n_words = nw;
  int nn = 0, pos = 0;
  for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
    fv_nodes[nn] = it->first;
    fv_off[nn] = pos;
    for (size_t j = 0; j < it->second.size(); j++) fv_feat[pos++] = it->second[j];
    nn++;
  }
  fv_off[nn] = pos;
  *n_fv = nn;
  return 0;
}

// score(v1, v2) through the vocabulary's own scoring object; ids ascending
double dbow2voc_score(void* h, const uint32_t* ids1, const double* vals1, int n1, const uint32_t* ids2, const double* vals2, int n2) {
  return ((Voc*)h)->score(bow(ids1, vals1, n1), bow(ids2, vals2, n2));
}

}  // extern "C"
