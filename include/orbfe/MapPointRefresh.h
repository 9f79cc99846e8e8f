// MapPointRefresh.h -- MapPoint::ComputeDistinctiveDescriptors() and MapPoint::UpdateNormalAndDepth() (reference
// src/MapPoint.cc:227-292, :315-356) for a whole vector of MapPoints in one GPU call (orbfe_local_map_refresh_rows,
// include/orbfe.h): the descriptors are gathered from the observing keyframes' RESIDENT copies, the chosen descriptor, the
// normal and the depth range are written into the rows of the local map's device table where the searches read them, and the
// same values are written back into the host objects, which then hold what the two reference functions would have left.
//
// Where LocalMapping / the map initialisation run
//     for (MapPoint* pMP : vpMPs) { pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth(); }
// write
//     orbfe::RefreshMapPoints(matcher, map, vpMPs, rows, [&](KeyFrame* pKF) { return residentFrameOf(pKF); });
// with rows[i] = the table row of vpMPs[i] and the callback returning the orbfe_frame built from pKF's mvKeysUn / mDescriptors.
//
// Needs the reference's own MapPoint.h / KeyFrame.h.  mNormalVector, mDescriptor, mfMinDistance and mfMaxDistance are protected
// there: add `friend struct orbfe::MapPointRefreshAccess;` to class MapPoint (or pass an Access type of your own with the same
// three static functions).  The fields are written under the mutexes the reference functions take.
#pragma once
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "../orbfe.h"

namespace orbfe {

struct MapPointRefreshAccess {
  template <class MP, class Mat>
  static void setDescriptor(MP* p, const Mat& d) {                        // MapPoint.cc:288-291
    std::unique_lock<std::mutex> lock(p->mMutexFeatures);
    p->mDescriptor = d;
  }
  template <class MP>
  static void setNormalAndDepth(MP* p, const float normal[3], float minRaw, float maxRaw) {   // MapPoint.cc:350-355
    std::unique_lock<std::mutex> lock(p->mMutexPos);
    p->mfMaxDistance = maxRaw;
    p->mfMinDistance = minRaw;
    auto nv = p->mWorldPos.clone();                                       // a 3x1 CV_32F of its own
    for (int k = 0; k < 3; k++) nv.template at<float>(k) = normal[k];
    p->mNormalVector = nv;
  }
};

// MapPoints that are bad or have no observation are left alone, as both reference functions return at once for them.
// what: ORBFE_REFRESH_DESCRIPTOR | ORBFE_REFRESH_NORMAL_DEPTH.  uploadPosition: send GetWorldPos() of every refreshed MapPoint
// to its row first (12 bytes each; pass false when the rows' positions are current).  The scale factors are the first reference
// keyframe's (one ORBextractor serves every keyframe of a map).  Returns ORBFE_OK or the failing call's error code
// (orbfe_last_error() tells why); on an error no host object has been changed.
template <class MapPointT, class FrameOfFn, class Access = MapPointRefreshAccess>
inline int RefreshMapPoints(orbfe_matcher* m, orbfe_local_map* map, const std::vector<MapPointT*>& vpMP, const std::vector<int32_t>& rows,
                            FrameOfFn frameOf, int what = ORBFE_REFRESH_DESCRIPTOR | ORBFE_REFRESH_NORMAL_DEPTH,
                            bool uploadPosition = true) {
  typedef decltype(vpMP[0]->GetReferenceKeyFrame()) KeyFramePtr;
  const bool geom = (what & ORBFE_REFRESH_NORMAL_DEPTH) != 0;
  std::map<KeyFramePtr, int> slotOf;
  std::vector<KeyFramePtr> kfs;
  std::vector<uint8_t> kfBad, kfNeeded;
  std::vector<MapPointT*> mps;
  std::vector<int32_t> mpRow, offs(1, 0), obsKf, obsKp, refKf, refKp;
  std::vector<uint8_t> obsFlags;
  std::vector<float> pos;
  auto slot = [&](KeyFramePtr pKF) {
    auto it = slotOf.find(pKF);
    if (it != slotOf.end()) return it->second;
    const int s = (int)kfs.size();
    slotOf[pKF] = s;
    kfs.push_back(pKF);
    kfBad.push_back(pKF->isBad() ? 1 : 0);
    kfNeeded.push_back(0);
    return s;
  };
  for (size_t i = 0; i < vpMP.size(); i++) {
    MapPointT* pMP = vpMP[i];
    if (!pMP || pMP->isBad()) continue;
    const auto observations = pMP->GetObservations();
    if (observations.empty()) continue;
    KeyFramePtr pRefKF = pMP->GetReferenceKeyFrame();
    for (auto mit = observations.begin(); mit != observations.end(); ++mit) {
      const int s = slot(mit->first);
      obsKf.push_back(s);
      obsKp.push_back((int32_t)mit->second);
      obsFlags.push_back(kfBad[s] ? ORBFE_OBS_KF_BAD : 0);
      if (!kfBad[s]) kfNeeded[s] = 1;
    }
    if (geom) {
      const int s = slot(pRefKF);
      kfNeeded[s] = 1;
      const auto it = observations.find(pRefKF);             // observations[pRefKF]: 0 when pRefKF is not among them
      refKf.push_back(s);
      refKp.push_back(it == observations.end() ? 0 : (int32_t)it->second);
    }
    offs.push_back((int32_t)obsKf.size());
    mps.push_back(pMP);
    mpRow.push_back(rows[i]);
    if (uploadPosition) {
      const auto P = pMP->GetWorldPos();
      for (int k = 0; k < 3; k++) pos.push_back(P.template at<float>(k));
    }
  }
  const int nmp = (int)mps.size(), nkf = (int)kfs.size();
  if (nmp == 0) return ORBFE_OK;
  std::vector<orbfe_frame*> frames(nkf, nullptr);
  std::vector<float> Ow(3 * (size_t)nkf);
  for (int s = 0; s < nkf; s++) {
    if (kfNeeded[s]) frames[s] = frameOf(kfs[s]);
    const auto C = kfs[s]->GetCameraCenter();
    for (int k = 0; k < 3; k++) Ow[3 * (size_t)s + k] = C.template at<float>(k);
  }
  std::vector<float> sf(1, 1.0f);
  int nlevels = 1;
  if (geom) {
    KeyFramePtr pRefKF = kfs[refKf[0]];
    sf.assign(pRefKF->mvScaleFactors.begin(), pRefKF->mvScaleFactors.end());
    nlevels = pRefKF->mnScaleLevels;
  }
  int rc;
  if (uploadPosition && (rc = orbfe_local_map_set_rows(map, nmp, mpRow.data(), pos.data(), nullptr, nullptr, nullptr, nullptr))) return rc;
  std::vector<int32_t> best(nmp);
  std::vector<float> normal(3 * (size_t)nmp), minRaw(nmp), maxRaw(nmp);
  if ((rc = orbfe_local_map_refresh_rows(m, map, what, nkf, frames.data(), Ow.data(), sf.data(), nlevels, nmp, mpRow.data(), offs.data(),
                                         obsKf.data(), obsKp.data(), obsFlags.data(), geom ? refKf.data() : nullptr,
                                         geom ? refKp.data() : nullptr, best.data(), normal.data(), minRaw.data(), maxRaw.data())))
    return rc;
  for (int p = 0; p < nmp; p++) {
    if ((what & ORBFE_REFRESH_DESCRIPTOR) && best[p] >= 0) {
      const int o = offs[p] + best[p];
      Access::setDescriptor(mps[p], kfs[obsKf[o]]->mDescriptors.row(obsKp[o]).clone());   // mDescriptor = vDescriptors[BestIdx].clone()
    }
    if (geom) Access::setNormalAndDepth(mps[p], &normal[3 * (size_t)p], minRaw[p], maxRaw[p]);
  }
  return ORBFE_OK;
}

}  // namespace orbfe
