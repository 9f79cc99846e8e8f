// TEST REFERENCE -- restated, not pinned.  The counting of LocalMapping::KeyFrameCulling (reference src/LocalMapping.cc:574-598)
// written again, single core: what orbfe_redundant_observations (include/orbfe.h) must return, and the host loop
// tools/keyframe_culling_bench.py times.  Nothing here is compiled from the reference; tests/cpp/keyframe_culling_facade_test.cpp
// checks the whole function on stub objects.
//
// kfcull_ref_counts reads the C call's arrays as they are.  kfcull_ref_loop_ms first builds plain structs with a
// std::map<Kf*, size_t> per MapPoint from them, so that the timed loop pays what the reference's pays: a copy of that map per
// (keyframe, MapPoint), and an indirection into the observer's keypoints per observation.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace {

struct KeyPt {
  int octave = 0;
};
struct Kf {
  std::vector<KeyPt> mvKeysUn;
};
struct Mp {
  std::map<Kf*, size_t> mObservations;
  int nObs = 0;
  std::map<Kf*, size_t> GetObservations() const { return mObservations; }   // a copy, as the reference returns one
  int Observations() const { return nObs; }
};
struct Subject {
  Kf* self = nullptr;              // null: nobody is excluded
  std::vector<Mp*> mvpMapPoints;   // null where the caller marked the entry skipped
  std::vector<KeyPt> mvKeysUn;
};
struct World {
  std::vector<Kf> kf;
  std::vector<Mp> mp;
  std::vector<Subject> subj;
};

// false: a MapPoint names one observer twice, which a std::map<KeyFrame*, size_t> cannot hold
bool build(World& W, int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs,
           int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level) {
  W.kf.resize((size_t)n_kf);
  W.mp.resize((size_t)n_mp);
  for (int p = 0; p < n_mp; p++) {
    for (int o = obs_offsets[p]; o < obs_offsets[p + 1]; o++) {
      Kf& K = W.kf[obs_kf[o]];
      KeyPt kp;
      kp.octave = obs_level[o];
      if (!W.mp[p].mObservations.emplace(&K, K.mvKeysUn.size()).second) return false;
      K.mvKeysUn.push_back(kp);
    }
    W.mp[p].nObs = mp_nobs ? mp_nobs[p] : obs_offsets[p + 1] - obs_offsets[p];
  }
  W.subj.resize((size_t)n_subj);
  for (int s = 0; s < n_subj; s++) {
    W.subj[s].self = subj_self[s] < 0 ? nullptr : &W.kf[subj_self[s]];
    for (int e = subj_offsets[s]; e < subj_offsets[s + 1]; e++) {
      KeyPt kp;
      kp.octave = subj_level[e];
      W.subj[s].mvpMapPoints.push_back(subj_mp[e] < 0 ? nullptr : &W.mp[subj_mp[e]]);
      W.subj[s].mvKeysUn.push_back(kp);
    }
  }
  return true;
}

// LocalMapping.cc:574-598 on the structs
void count(const Subject& S, int thObs, int& nMPs, int& nRedundantObservations) {
  nMPs = 0;
  nRedundantObservations = 0;
  for (size_t i = 0; i < S.mvpMapPoints.size(); i++) {
    Mp* pMP = S.mvpMapPoints[i];
    if (!pMP) continue;
    nMPs++;
    if (pMP->Observations() <= thObs) continue;
    const int scaleLevel = S.mvKeysUn[i].octave;
    const std::map<Kf*, size_t> observations = pMP->GetObservations();
    int nObs = 0;
    for (std::map<Kf*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) {
      if (mit->first == S.self) continue;
      if (mit->first->mvKeysUn[mit->second].octave <= scaleLevel + 1 && ++nObs >= thObs) break;
    }
    if (nObs >= thObs) nRedundantObservations++;
  }
}

}  // namespace

extern "C" {

// as orbfe_redundant_observations without the matcher and without its argument check, over the arrays themselves
int kfcull_ref_counts(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs, int n_subj,
                      const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level, int th_obs,
                      int32_t* out_n_mps, int32_t* out_n_redundant) {
  (void)n_kf;
  (void)n_mp;
  for (int s = 0; s < n_subj; s++) {
    int nMPs = 0, nRedundant = 0;
    for (int e = subj_offsets[s]; e < subj_offsets[s + 1]; e++) {
      const int p = subj_mp[e];
      if (p < 0) continue;                                                  // !pMP || pMP->isBad()
      nMPs++;
      const int observations = mp_nobs ? mp_nobs[p] : obs_offsets[p + 1] - obs_offsets[p];
      if (observations <= th_obs) continue;
      const int scaleLevel = subj_level[e];
      int nObs = 0;
      for (int o = obs_offsets[p]; o < obs_offsets[p + 1]; o++) {
        if (obs_kf[o] == subj_self[s]) continue;
        const int scaleLeveli = obs_level[o];
        if (scaleLeveli <= scaleLevel + 1) {
          nObs++;
          if (nObs >= th_obs) break;
        }
      }
      if (nObs >= th_obs) nRedundant++;
    }
    out_n_mps[s] = nMPs;
    out_n_redundant[s] = nRedundant;
  }
  return 0;
}

// The same counts from the structs (std::map per MapPoint): 0, or -1 where a MapPoint names one observer twice.
int kfcull_ref_counts_structs(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs,
                              int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level,
                              int th_obs, int32_t* out_n_mps, int32_t* out_n_redundant) {
  World W;
  if (!build(W, n_kf, n_mp, obs_offsets, obs_kf, obs_level, mp_nobs, n_subj, subj_self, subj_offsets, subj_mp, subj_level)) return -1;
  for (int s = 0; s < n_subj; s++) {
    int a = 0, b = 0;
    count(W.subj[s], th_obs, a, b);
    out_n_mps[s] = a;
    out_n_redundant[s] = b;
  }
  return 0;
}

// The host loop alone, timed: every subject, one after the other, `reps` rounds; the median round in ms.  The structs are built
// beforehand; *checksum (the sum of nRedundantObservations of the last round) keeps the loop from being optimised away.
double kfcull_ref_loop_ms(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs,
                          int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level,
                          int th_obs, int reps, long long* checksum) {
  World W;
  if (!build(W, n_kf, n_mp, obs_offsets, obs_kf, obs_level, mp_nobs, n_subj, subj_self, subj_offsets, subj_mp, subj_level) || reps < 1) return -1.0;
  std::vector<double> ms;
  for (int r = 0; r < reps; r++) {
    long long sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < n_subj; s++) {
      int a = 0, b = 0;
      count(W.subj[s], th_obs, a, b);
      sum += b;
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (checksum) *checksum = sum;
  }
  std::sort(ms.begin(), ms.end());
  return ms[ms.size() / 2];
}

// The write-down alone, timed: from the structs to the arrays of one call, the way include/orbfe/KeyFrameCulling.h does it on the
// real objects -- a std::map from MapPoint to index and from keyframe to slot, every distinct MapPoint's observation map copied and
// read once (slot, octave, Observations()), one index and one octave per entry.  The median of `reps` rounds in ms; *checksum is the
// number of observations written in the last round.
double kfcull_ref_writedown_ms(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, const uint8_t* obs_level, const int32_t* mp_nobs,
                               int n_subj, const int32_t* subj_self, const int32_t* subj_offsets, const int32_t* subj_mp, const uint8_t* subj_level,
                               int reps, long long* checksum) {
  World W;
  if (!build(W, n_kf, n_mp, obs_offsets, obs_kf, obs_level, mp_nobs, n_subj, subj_self, subj_offsets, subj_mp, subj_level) || reps < 1) return -1.0;
  std::vector<double> ms;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    std::map<Kf*, int32_t> slotOf;
    std::map<Mp*, int32_t> indexOf;
    std::vector<int32_t> oOffs(1, 0), oKf, nobs, sSelf, sOffs(1, 0), sMp;
    std::vector<uint8_t> oLevel, sLevel;
    for (int s = 0; s < n_subj; s++)
      if (W.subj[s].self) slotOf.emplace(W.subj[s].self, (int32_t)slotOf.size());
    for (int s = 0; s < n_subj; s++) {
      const Subject& S = W.subj[s];
      const std::vector<Mp*> vpMapPoints = S.mvpMapPoints;                // GetMapPointMatches() returns a copy
      for (size_t i = 0; i < vpMapPoints.size(); i++) {
        Mp* pMP = vpMapPoints[i];
        int32_t p = -1;
        if (pMP) {
          std::map<Mp*, int32_t>::iterator it = indexOf.find(pMP);
          if (it != indexOf.end()) p = it->second;
          else {
            p = (int32_t)oOffs.size() - 1;
            indexOf[pMP] = p;
            const std::map<Kf*, size_t> observations = pMP->GetObservations();
            for (std::map<Kf*, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); ++mit) {
              oKf.push_back(slotOf.emplace(mit->first, (int32_t)slotOf.size()).first->second);
              oLevel.push_back((uint8_t)mit->first->mvKeysUn[mit->second].octave);
            }
            oOffs.push_back((int32_t)oKf.size());
            nobs.push_back(pMP->Observations());
          }
        }
        sMp.push_back(p);
        sLevel.push_back(pMP ? (uint8_t)S.mvKeysUn[i].octave : 0);
      }
      sSelf.push_back(S.self ? slotOf[S.self] : -1);
      sOffs.push_back((int32_t)sMp.size());
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (checksum) *checksum = (long long)oKf.size();
  }
  std::sort(ms.begin(), ms.end());
  return ms[ms.size() / 2];
}

}  // extern "C"
