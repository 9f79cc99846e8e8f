// TEST REFERENCE -- restated, not pinned.  The counting loops of KeyFrame::UpdateConnections (reference src/KeyFrame.cc:305-331)
// and Tracking::UpdateLocalKeyFrames (src/Tracking.cc:862-879), written again on plain structs with std::map, single core: what
// orbfe_covisibility_counts (include/orbfe.h) must return, and the host loop tools/covisibility_bench.py times.  Nothing here is
// compiled from the reference; tests/cpp/covisibility_test.cpp checks the whole function on stub objects.
//
// The structs are built from the C call's arrays: keyframe slot j becomes kf[j] of ONE vector, so that pointer order -- the order
// std::map<Kf*, ...> iterates in -- is slot order, and a counter read front to back is the call's ascending-slot segment.
// subj_limit has no counterpart in the reference function: it stands for the state of Osmap's rebuild, in which the keyframes
// >= limit have not added their observations yet, so those are left out of the MapPoints' maps as the subject sees them.
#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <map>
#include <vector>

namespace {

struct Kf {
  long unsigned int mnId = 0;
};
struct Mp {
  std::map<Kf*, size_t> mObservations;
  std::map<Kf*, size_t> GetObservations() const { return mObservations; }   // a copy, as the reference returns one
};
struct Subject {
  long mnId = -1;                  // -1: a Frame (Tracking), which excludes nobody
  int limit = 0;
  std::vector<Mp*> mvpMapPoints;   // null where the caller marked the entry skipped
};
struct World {
  std::vector<Kf> kf;
  std::vector<Mp> mp;
  std::vector<Subject> subj;
};

// false: a MapPoint names one observer twice, which a std::map<KeyFrame*, size_t> cannot hold
bool build(World& W, int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj, const int32_t* subj_self,
           const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp) {
  W.kf.resize((size_t)n_kf);
  for (int j = 0; j < n_kf; j++) W.kf[j].mnId = (long unsigned int)j;
  W.mp.resize((size_t)n_mp);
  for (int p = 0; p < n_mp; p++)
    for (int o = obs_offsets[p]; o < obs_offsets[p + 1]; o++)
      if (!W.mp[p].mObservations.emplace(&W.kf[obs_kf[o]], (size_t)(o - obs_offsets[p])).second) return false;
  W.subj.resize((size_t)n_subj);
  for (int s = 0; s < n_subj; s++) {
    W.subj[s].mnId = subj_self[s];
    W.subj[s].limit = subj_limit ? subj_limit[s] : n_kf;
    for (int e = subj_offsets[s]; e < subj_offsets[s + 1]; e++) W.subj[s].mvpMapPoints.push_back(subj_mp[e] < 0 ? nullptr : &W.mp[subj_mp[e]]);
  }
  return true;
}

// KeyFrame.cc:305-331 (self >= 0) and Tracking.cc:862-879 (self < 0)
void count(const Subject& S, std::map<Kf*, int>& KFcounter) {
  for (std::vector<Mp*>::const_iterator vit = S.mvpMapPoints.begin(); vit != S.mvpMapPoints.end(); ++vit) {
    Mp* pMP = *vit;
    if (!pMP) continue;
    std::map<Kf*, size_t> observations = pMP->GetObservations();
    for (std::map<Kf*, size_t>::iterator mit = observations.begin(); mit != observations.end(); ++mit) {
      if ((long)mit->first->mnId >= (long)S.limit) continue;          // has not added its observation yet (see above)
      if (S.mnId >= 0 && (long)mit->first->mnId == S.mnId) continue;
      KFcounter[mit->first]++;
    }
  }
}

}  // namespace

extern "C" {

// as orbfe_covisibility_counts without the matcher: 0, -5 with *n_needed set when cap is too small, -1 for a duplicate observer
int covis_ref_counts(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj, const int32_t* subj_self,
                     const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp, int32_t* out_offsets, int32_t* out_kf,
                     int32_t* out_count, int cap, int* n_needed) {
  World W;
  if (!build(W, n_kf, n_mp, obs_offsets, obs_kf, n_subj, subj_self, subj_limit, subj_offsets, subj_mp)) return -1;
  long long at = 0;
  for (int s = 0; s < n_subj; s++) {
    std::map<Kf*, int> KFcounter;
    count(W.subj[s], KFcounter);
    out_offsets[s] = (int32_t)at;
    for (std::map<Kf*, int>::iterator it = KFcounter.begin(); it != KFcounter.end(); ++it, ++at)
      if (at < cap) { out_kf[at] = (int32_t)(it->first - W.kf.data()); out_count[at] = it->second; }
  }
  out_offsets[n_subj] = (int32_t)at;
  *n_needed = (int)at;
  return at > cap ? -5 : 0;
}

// The host loop alone, timed: the counter of every subject, one after the other, `reps` rounds; the median round in ms.  The
// structs are built beforehand; *checksum (the sum of all counters of the last round) keeps the loop from being optimised away.
double covis_ref_loop_ms(int n_kf, int n_mp, const int32_t* obs_offsets, const int32_t* obs_kf, int n_subj, const int32_t* subj_self,
                         const int32_t* subj_limit, const int32_t* subj_offsets, const int32_t* subj_mp, int reps, long long* checksum) {
  World W;
  if (!build(W, n_kf, n_mp, obs_offsets, obs_kf, n_subj, subj_self, subj_limit, subj_offsets, subj_mp) || reps < 1) return -1.0;
  std::vector<double> ms;
  for (int r = 0; r < reps; r++) {
    long long sum = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int s = 0; s < n_subj; s++) {
      std::map<Kf*, int> KFcounter;
      count(W.subj[s], KFcounter);
      for (std::map<Kf*, int>::iterator it = KFcounter.begin(); it != KFcounter.end(); ++it) sum += it->second;
    }
    ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (checksum) *checksum = sum;
  }
  std::sort(ms.begin(), ms.end());
  return ms[ms.size() / 2];
}

}  // extern "C"
