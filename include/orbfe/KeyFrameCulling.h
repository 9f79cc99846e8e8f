// KeyFrameCulling.h -- LocalMapping::KeyFrameCulling() (reference src/LocalMapping.cc:556-603) with the counting loop of ALL local
// keyframes in one GPU call (orbfe_redundant_observations, include/orbfe.h).  Every MapPoint of the given keyframes is walked ONCE
// on the host to write down who observes it and at which octave; the per-keyframe, per-MapPoint, per-observer counting -- with the
// reference's copy of the observation std::map per (keyframe, MapPoint) -- runs on the device; the verdicts are replayed here on
// the real pointers, in the vector's order.
//
// The counts depend on the observation graph, and SetBadFlag() changes it.  Until a keyframe actually goes bad every count of the
// batch is what the sequential loop would read, so the verdicts are applied in order up to the first keyframe that goes bad; the
// keyframes after it are counted again on the changed graph, and so on: 1 + (keyframes culled) calls at the most, and the
// reference's result in every case.  A keyframe held by mbNotErase only notes mbToBeErased and changes nothing: no recount.
//
// In LocalMapping::KeyFrameCulling, after
//     vector<KeyFrame*> vpLocalKeyFrames = mpCurrentKeyFrame->GetVectorCovisibleKeyFrames();
// the loop :564-602 becomes
//     orbfe::KeyFrameCulling(matcher, vpLocalKeyFrames);
//
// Needs the reference's own KeyFrame.h / MapPoint.h; only public members are used (mnId, mvKeysUn, GetMapPointMatches, isBad,
// SetBadFlag; GetObservations, Observations, isBad).  KeyFrameCullingWith takes the counter as an argument -- anything callable
// like orbfe_redundant_observations without the matcher -- so that the sequential logic can run on a CPU.
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <set>
#include <type_traits>
#include <utility>
#include <vector>

#include "../orbfe.h"
#include "Covisibility.h"

namespace orbfe {

struct KeyFrameCullingStats {
  int calls;      // counting calls made: 1, plus one per cull that left keyframes to judge
  int culled;     // keyframes that went bad
  int subjects;   // subjects of all calls together
};

// The arrays of one orbfe_redundant_observations call: CovisibilityCsr's, plus the octave of every observation and every entry and
// Observations() per MapPoint.  ok turns false on an octave outside [0, 255].
template <class KF, class MP>
struct KeyFrameCullingCsr : CovisibilityCsr<KF, MP> {
  std::vector<uint8_t> obsLevel, subjLevel;
  std::vector<int32_t> mpNobs;
  bool ok = true;

  uint8_t level(int octave) {
    if (octave < 0 || octave > 255) { ok = false; return 0; }
    return (uint8_t)octave;
  }
  // one subject, in slot `self`; keyframe 0 is never judged (LocalMapping.cc:567) and brings no entries.  To CovisibilityCsr's
  // walk this adds the octave of every observation and Observations() when a MapPoint is first seen, and the octave of every entry.
  void subject(int32_t self, KF* pKF) {
    CovisibilityCsr<KF, MP>::subject(
        self, -1, pKF->mnId != 0 ? pKF->GetMapPointMatches() : std::vector<MP*>(), [](MP* pMP) { return !pMP || pMP->isBad(); },   // LocalMapping.cc:576
        [this](MP* pMP, const std::map<KF*, size_t>& observations) {
          for (typename std::map<KF*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit)
            obsLevel.push_back(level(mit->first->mvKeysUn[mit->second].octave));
          mpNobs.push_back((int32_t)pMP->Observations());
        },
        [this, pKF](size_t i, int32_t p) { subjLevel.push_back(p < 0 ? 0 : level(pKF->mvKeysUn[i].octave)); });
  }
};

// One round: the counts nMPs / nRedundantObservations of vpLocalKeyFrames[start..], from the objects as they are now.  Changes no
// object.  ORBFE_OK, ORBFE_ERR_INVALID for an octave outside [0, 255], or the counter's error code.
template <class KeyFrameT, class Counter>
inline int KeyFrameCullingCount(Counter&& count, const std::vector<KeyFrameT*>& vpLocalKeyFrames, size_t start, std::vector<int32_t>& nMPs,
                                std::vector<int32_t>& nRedundant) {
  typedef decltype(vpLocalKeyFrames[0]->GetMapPointMatches()) MapPointVector;
  typedef typename std::remove_pointer<typename MapPointVector::value_type>::type MapPointT;
  const int thObs = 3;
  KeyFrameCullingCsr<KeyFrameT, MapPointT> csr;
  for (size_t k = start; k < vpLocalKeyFrames.size(); k++) csr.slot(vpLocalKeyFrames[k]);          // subjects first: slot == k - start
  for (size_t k = start; k < vpLocalKeyFrames.size(); k++) csr.subject((int32_t)(k - start), vpLocalKeyFrames[k]);
  if (!csr.ok) return ORBFE_ERR_INVALID;
  const int n = csr.nSubjects();
  nMPs.assign((size_t)n, 0);
  nRedundant.assign((size_t)n, 0);
  return count((int)csr.kfs.size(), (int)csr.obsOffsets.size() - 1, csr.obsOffsets.data(), csr.obsKf.data(), csr.obsLevel.data(), csr.mpNobs.data(), n,
               csr.subjSelf.data(), csr.subjOffsets.data(), csr.subjMp.data(), csr.subjLevel.data(), thObs, nMPs.data(), nRedundant.data());
}

// LocalMapping::KeyFrameCulling's loop over vpLocalKeyFrames, the counting done by `count`.  A keyframe must not appear twice
// (ORBFE_ERR_INVALID, nothing changed).  Returns ORBFE_OK or the error code of the round that failed: that round changes no
// object; the culls of the rounds before it stand.
template <class KeyFrameT, class Counter>
inline int KeyFrameCullingWith(Counter&& count, const std::vector<KeyFrameT*>& vpLocalKeyFrames, KeyFrameCullingStats* stats = nullptr) {
  KeyFrameCullingStats st = {0, 0, 0};
  if (stats) *stats = st;
  if (std::set<KeyFrameT*>(vpLocalKeyFrames.begin(), vpLocalKeyFrames.end()).size() != vpLocalKeyFrames.size()) return ORBFE_ERR_INVALID;
  int rc = ORBFE_OK;
  std::vector<int32_t> nMPs, nRedundant;
  for (size_t start = 0; start < vpLocalKeyFrames.size();) {
    rc = KeyFrameCullingCount(count, vpLocalKeyFrames, start, nMPs, nRedundant);
    if (rc) break;
    st.calls++;
    st.subjects += (int)(vpLocalKeyFrames.size() - start);
    size_t k = start;
    for (; k < vpLocalKeyFrames.size(); k++) {
      KeyFrameT* pKF = vpLocalKeyFrames[k];
      if (pKF->mnId == 0) continue;                                               // LocalMapping.cc:567
      const int nRedundantObservations = nRedundant[k - start], nMPsK = nMPs[k - start];
      if (nRedundantObservations > 0.9 * nMPsK) {                                 // :600, an int against a double
        const bool wasBad = pKF->isBad();
        pKF->SetBadFlag();
        if (!wasBad && pKF->isBad()) { st.culled++; break; }                      // the graph has changed: the counts after k are stale
      }
    }
    start = k + 1;                                                                // (past the end when nobody went bad)
  }
  if (stats) *stats = st;
  return rc;
}

// The loop with the counting on the GPU, on the matcher's stream.
template <class KeyFrameT>
inline int KeyFrameCulling(orbfe_matcher* m, const std::vector<KeyFrameT*>& vpLocalKeyFrames, KeyFrameCullingStats* stats = nullptr) {
  return KeyFrameCullingWith(
      [m](int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs, int n_subj,
          const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level, int th_obs, int32_t* out_n_mps,
          int32_t* out_n_redundant) {
        return orbfe_redundant_observations(m, n_kf, n_mp, obs_offsets, obs_kf, obs_level, mp_nobs, n_subj, subj_self, subj_offsets, subj_mp, subj_level,
                                            th_obs, out_n_mps, out_n_redundant);
      },
      vpLocalKeyFrames, stats);
}

}  // namespace orbfe
