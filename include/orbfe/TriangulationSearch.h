// TriangulationSearch.h -- the SearchForTriangulation loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:207-232) as
// ONE GPU call for all neighbours (orbfe_search_for_triangulation_frames_batch), then one host step per neighbour at the moment
// the loop reaches it (orbfe_triangulation_finish):
//
//     orbfe::TriangulationSearch<KeyFrame> S(ctx, mbCheckOrientation, mpCurrentKeyFrame, vpNeigh, vF12);   // in front of the loop
//     for (size_t i = 0; i < vpNeigh.size(); i++) {
//       int n = S.pairs(i, vMatchedIndices);          // what matcher.SearchForTriangulation(mpCurrentKeyFrame, vpNeigh[i], vF12[i], ...) returns NOW
//       /* ... triangulate, mpCurrentKeyFrame->AddMapPoint(pMP, idx1) ... */
//     }
//
// vpNeigh are the neighbours that passed the baseline test (:212-223), vF12[i] = ComputeF12(mpCurrentKeyFrame, vpNeigh[i]) (:226):
// both depend on poses only and move in front of the loop.  The constructor computes every neighbour's epipole as
// ORBmatcher.cc:657-666 does, takes the keyframes' resident copies from the context's cache (a keyframe it does not hold is made
// resident first) and makes the one call with the MapPoint flags as they stand.  pairs(i, ...) reads pKF1->GetMapPoint(idx1) NOW:
// keypoints that got a MapPoint since are dropped before the orientation histogram, which is what the reference's search would do.
// The contract: during the loop the current keyframe's flags only grow, and a neighbour's own flags change only in its own iteration.
// If a flag of the current keyframe was CLEARED meanwhile (ORBFE_ERR_STALE), pairs(i, ...) runs the existing single search,
// orbfe::SearchForTriangulation, for that neighbour; so it does for every neighbour when the context's frame cache cannot hold
// the current keyframe and all neighbours at once (capacity below vpNeigh.size() + 1, or 0 = off).
//
// KeyFrameT: N, mvKeysUn, mDescriptors, mFeatVec, mvScaleFactors, mvLevelSigma2, mnMinX .. mnMaxY, fx, fy, cx, cy, GetMapPoint(i),
// GetCameraCenter(), GetRotation(), GetTranslation() (the last three as cv::Mat, or anything with operator*, operator+ and
// at<float>(i)).  MatT (F12): at<float>(r, c).  cv-free like orb_shim.hpp.
#pragma once
#include <utility>
#include <vector>

#include "orb_shim.hpp"

namespace orbfe {

template <class KeyFrameT>
class TriangulationSearch {
 public:
  template <class MatT>
  TriangulationSearch(MatcherContext& ctx, bool mbCheckOrientation, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeigh,
                      const std::vector<MatT>& vF12)
      : ctx_(ctx), ori_(mbCheckOrientation), kf1_(pKF1), nb_(vpNeigh), n1_((int)pKF1->N) {
    if (vF12.size() != vpNeigh.size()) throw std::runtime_error("orbfe: TriangulationSearch needs one F12 per neighbour");
    const size_t K = vpNeigh.size();
    geo_.resize(K);
    for (size_t k = 0; k < K; k++) {
      Geo& g = geo_[k];
      for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) g.F.v[3 * r + c] = vF12[k].template at<float>(r, c);
      // epipole of camera 1 in image 2 (ORBmatcher.cc:657-666)
      auto Cw = pKF1->GetCameraCenter();
      auto R2w = vpNeigh[k]->GetRotation();
      auto t2w = vpNeigh[k]->GetTranslation();
      decltype(Cw) C2 = R2w * Cw + t2w;
      const float invz = 1.0f / C2.template at<float>(2);
      g.ex = vpNeigh[k]->fx * C2.template at<float>(0) * invz + vpNeigh[k]->cx;
      g.ey = vpNeigh[k]->fy * C2.template at<float>(1) * invz + vpNeigh[k]->cy;
    }
    batched_ = K > 0 && ctx.frameCacheCapacity() >= K + 1;
    if (!batched_) return;
    has1_.assign(n1_ > 0 ? n1_ : 1, 0);
    for (int i = 0; i < n1_; i++) has1_[i] = pKF1->GetMapPoint(i) ? 1 : 0;   // ORBmatcher.cc:704-709
    std::vector<uint32_t> n1v, o1v, f1v;
    detail::flattenFeatureVector(pKF1->mFeatVec, n1v, o1v, f1v);
    struct Side { std::vector<uint8_t> has; std::vector<uint32_t> nodes, offs, feats; };
    std::vector<Side> side(K);
    std::vector<OrbfeTriangulationNeighbour> nb(K);
    // a look-up may create a frame and evict the least recently used one; the frames looked up here are the most recently used
    // ones, and the capacity test above says that all K + 1 fit: none of them is evicted before the call below returns
    frame1_ = ctx.resident(*pKF1, 1);
    for (size_t k = 0; k < K; k++) nb[k].frame2 = ctx.resident(*vpNeigh[k], 1);
    for (size_t k = 0; k < K; k++) {
      KeyFrameT* p2 = vpNeigh[k];
      Side& s = side[k];
      const int n2 = (int)p2->N;
      s.has.assign(n2 > 0 ? n2 : 1, 0);
      for (int i = 0; i < n2; i++) s.has[i] = p2->GetMapPoint(i) ? 1 : 0;    // :723-727
      detail::flattenFeatureVector(p2->mFeatVec, s.nodes, s.offs, s.feats);
      OrbfeTriangulationNeighbour& t = nb[k];
      t.has_mp2 = s.has.data();
      t.fv2_nodes = s.nodes.data(); t.fv2_offsets = s.offs.data(); t.fv2_features = s.feats.data(); t.n_fv2 = (int)s.nodes.size();
      for (int i = 0; i < 9; i++) t.F12[i] = geo_[k].F.v[i];
      t.ex = geo_[k].ex; t.ey = geo_[k].ey;
      t.scale_factors2 = p2->mvScaleFactors.data(); t.level_sigma2_2 = p2->mvLevelSigma2.data(); t.nlevels2 = (int)p2->mvScaleFactors.size();
    }
    raw_.assign(K * (size_t)(n1_ > 0 ? n1_ : 1), -1);
    check(orbfe_search_for_triangulation_frames_batch(ctx.get(), frame1_, has1_.data(), n1v.data(), o1v.data(), f1v.data(), (int)n1v.size(),
                                                      (int)K, nb.data(), raw_.data()));
  }

  size_t size() const { return nb_.size(); }
  bool batched() const { return batched_; }        // false: every pairs() call is the single search (see the head of this file)
  int fallbacks() const { return fallbacks_; }     // pairs() calls that took the single search
  float ex(size_t i) const { return geo_[i].ex; }
  float ey(size_t i) const { return geo_[i].ey; }

  // int ORBmatcher::SearchForTriangulation(pKF1, vpNeigh[i], vF12[i], vMatchedPairs) with pKF1's MapPoints as they are NOW
  int pairs(size_t i, std::vector<std::pair<size_t, size_t> >& vMatchedPairs) {
    KeyFrameT* p2 = nb_.at(i);
    if (batched_) {
      std::vector<uint8_t> now(n1_ > 0 ? n1_ : 1, 0);
      for (int j = 0; j < n1_; j++) now[j] = kf1_->GetMapPoint(j) ? 1 : 0;
      std::vector<int32_t> out((size_t)(n1_ > 0 ? n1_ : 1) * 2, -1);
      int n = 0;
      const int rc = orbfe_triangulation_finish(&raw_[i * (size_t)(n1_ > 0 ? n1_ : 1)], n1_, has1_.data(), now.data(), ori_ ? 1 : 0,
                                                reinterpret_cast<const OrbfeKeyPoint*>(kf1_->mvKeysUn.data()),
                                                reinterpret_cast<const OrbfeKeyPoint*>(p2->mvKeysUn.data()), (int)p2->N, out.data(), &n);
      if (rc == ORBFE_OK) {
        vMatchedPairs.clear();
        vMatchedPairs.reserve(n);
        for (int j = 0; j < n; j++) vMatchedPairs.push_back(std::make_pair((size_t)out[2 * j], (size_t)out[2 * j + 1]));
        return n;
      }
      if (rc != ORBFE_ERR_STALE) check(rc);
    }
    fallbacks_++;
    return SearchForTriangulation(ctx_, ori_, kf1_, p2, geo_[i].F, geo_[i].ex, geo_[i].ey, vMatchedPairs);
  }

 private:
  struct Mat33 {   // F12 as the single search reads it
    float v[9];
    template <class T> T at(int r, int c) const { return v[3 * r + c]; }
  };
  struct Geo { Mat33 F; float ex = 0, ey = 0; };
  MatcherContext& ctx_;
  bool ori_, batched_ = false;
  KeyFrameT* kf1_;
  std::vector<KeyFrameT*> nb_;
  int n1_, fallbacks_ = 0;
  orbfe_frame* frame1_ = nullptr;
  std::vector<Geo> geo_;
  std::vector<uint8_t> has1_;
  std::vector<int32_t> raw_;
};

}  // namespace orbfe
